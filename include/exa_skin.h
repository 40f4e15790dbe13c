/*
 * exa_skin.h -- C ABI of the MI355X-native linear blend skinning (ExAvatar's get_transform_mat_vertex + lbs).
 *
 * This is the native boundary under the skinning that poses the Gaussians of the reference's HumanGaussian
 * (avatar/common/nets/module.py:413-422, called at 548-556): per-vertex transforms blended from the joint transforms by
 * the skinning weights of each vertex's nearest template vertex, applied to both point sets (mean_3d and
 * mean_3d_refined), the translation added, and the optional camera -> world step.  The Python drop-in over it is
 * `exavatar_release_amd.skinning.skin_points`.  It lives in the same `libexa_raster.so` as include/exa_raster.h,
 * include/exa_mesh.h, include/exa_knn.h and include/exa_triplane.h.
 *
 * Inputs.  V vertices and S point sets (1 <= S <= EXA_SKIN_MAX_SETS), each [V, 3].  weights [Vw, J], J joints.  idx [V]
 * int64 selects the weight row of every vertex (`nn_vertex_idxs`), or NULL for the identity (Vw == V).  T [J, 4, 4] the
 * joint transforms (rows 0-2 are read), trans [3], and optionally Rinv [3, 3] and t [3] (both or neither).
 *
 * Forward.  With w_j = weights[idx[v], j] and every operation rounded in fp32 with no fused multiply-add:
 *     A[r][c] = (((+0 + w_0 * T[0][r][c]) + w_1 * T[1][r][c]) + ...) + w_{J-1} * T[J-1][r][c]     r < 3, c < 4
 *         all J terms, zero weights included (0 * inf stays NaN), computed once per vertex and applied to every set;
 *     q_r = ((A[r][0] * x + A[r][1] * y) + A[r][2] * z) + A[r][3]
 *     p_r = q_r + trans_r
 *     out_r = p_r                                                              without the camera step, or
 *     out_r = (Rinv[r][0] * d_0 + Rinv[r][1] * d_1) + Rinv[r][2] * d_2,  d_c = p_c - t_c     with it.
 *
 * Backward.  From the per-set output gradients g_s [V, 3]:
 *     g'_c = (Rinv[0][c] * g_0 + Rinv[1][c] * g_1) + Rinv[2][c] * g_2     (Rinv^T g; g' = g without the camera step)
 *     grad_x_c = (A[0][c] * g'_0 + A[1][c] * g'_1) + A[2][c] * g'_2        c < 3, per set
 *     G_v[r][c] = (((+0 + g'_{0,r} * x~_{0,c}) + g'_{1,r} * x~_{1,c}) + ...)   in set order, x~ = (x, y, z, 1)
 *     grad_T[j][r][c] = sum over v of fl(w_{v,j} * G_v[r][c])              r < 3; row 3 of grad_T is written as +0
 *     grad_trans[r]   = sum over v of G_v[r][3]
 * Both vertex sums use one fixed two-level order: the vertices are cut into chunks of EXA_SKIN_CHUNK in ascending order,
 * each chunk is summed sequentially from +0 in ascending v, and the chunk partials are summed sequentially from +0 in
 * chunk order.  The constant fixes the result; the launch shape does not change it.  The backward uses no atomics and no
 * memsets: the same inputs give the same bits on every call.
 *
 * Out-of-range indices.  A vertex whose idx lies outside [0, Vw) reads no weight row: its weights are all NaN, so its
 * outputs, its point gradients and every element of grad_T are NaN (the error shows instead of passing silently).
 *
 * Conventions (those of exa_knn.h / exa_triplane.h)
 *   - plain C types only: device pointers, sizes, a `hipStream_t` passed as `void*`.  `points`, `out`, `grad_out` and
 *     `grad_points` are HOST arrays of S device pointers, so separate tensors need no stacking copy.
 *   - every pointer marked [dev] is a device pointer owned by the caller; the library allocates nothing and keeps no
 *     state between calls.  The backward's workspace size follows from (V, J) alone (exa_skin_workspace_size); every
 *     byte of it the backward reads, it has written first.
 *   - fp32 points, weights and transforms; int64 indices; contiguous row-major arrays.
 *   - work is enqueued on `stream`; no call synchronises the device, so a call can be captured into a hipGraph.
 *   - return value: 0 = ok; < 0 = invalid argument (EXA_SKIN_E_*), checked before any GPU work; > 0 = HIP error code.
 */
#ifndef EXA_SKIN_H
#define EXA_SKIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EXA_SKIN_VERSION 100            /* 0.1.0.0: first version */
#define EXA_SKIN_MAX_JOINTS 64          /* 1 <= J <= EXA_SKIN_MAX_JOINTS (SMPL-X has 55) */
#define EXA_SKIN_MAX_SETS 4             /* 1 <= S <= EXA_SKIN_MAX_SETS (the reference uses 2) */
#define EXA_SKIN_MAX_POINTS (1 << 28)   /* V, Vw */
#define EXA_SKIN_CHUNK 256              /* vertices per chunk of the backward's two-level sums */

#define EXA_SKIN_E_INVALID (-1)
#define EXA_SKIN_E_NULLPTR (-2)

int exa_skin_version(void);
/* Message of the most recent failing call of this thread ("" if none). */
const char* exa_skin_last_error(void);

/* Bytes of the backward's workspace: ceil(V / EXA_SKIN_CHUNK) * (12 J + 3) fp32 chunk partials (0 when V == 0). */
int exa_skin_workspace_size(int32_t V, int32_t J, uint64_t* out_bytes);

/* The posed points of every set.
 *   points   host array of S [dev] pointers, each [V, 3].
 *   weights  [dev] [Vw, J].
 *   idx      [dev] [V] int64 weight rows, or NULL (then Vw must equal V).
 *   T        [dev] [J, 4, 4].
 *   trans    [dev] [3].
 *   Rinv, t  [dev] [3, 3] and [3], or both NULL (no camera step).
 *   out      host array of S [dev] pointers, each [V, 3], fully written. */
int exa_skin_forward(int32_t V, int32_t S, int32_t J, int32_t Vw, const float* const* points, const float* weights,
                     const int64_t* idx, const float* T, const float* trans, const float* Rinv, const float* t,
                     float* const* out, void* stream);

/* Gradients of the forward (the header's orders, no atomics).
 *   points, weights, idx, T, Vw, Rinv  as in the forward (Rinv NULL = no camera step).
 *   grad_out     host array of S [dev] pointers, each [V, 3].
 *   grad_points  host array of S pointers, each [dev] [V, 3] or NULL (that set's point gradient is not written).
 *   grad_T       [dev] [J, 4, 4] or NULL; fully written (row 3 = +0).
 *   grad_trans   [dev] [3] or NULL.
 *   workspace    [dev] at least exa_skin_workspace_size(V, J) bytes (may be NULL when V == 0). */
int exa_skin_backward(int32_t V, int32_t S, int32_t J, int32_t Vw, const float* const* points, const float* weights,
                      const int64_t* idx, const float* T, const float* Rinv, const float* const* grad_out,
                      float* const* grad_points, float* grad_T, float* grad_trans, void* workspace,
                      uint64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EXA_SKIN_H */
