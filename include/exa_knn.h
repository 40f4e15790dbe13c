/*
 * exa_knn.h -- C ABI of the MI355X-native K-nearest-neighbour search (pytorch3d `knn_points`, squared L2, D = 3).
 *
 * This is the native boundary under ExAvatar's per-frame nearest-vertex search (reference avatar/common/nets/module.py:543,
 * K = 1 of the upsampled Gaussian centres against the template vertices) and the init-time scene scale (module.py:86, a
 * K = 4 self-query).  The Python drop-in over it is `exavatar_release_amd.knn.knn_points`.  It lives in the same
 * `libexa_raster.so` as include/exa_raster.h and include/exa_mesh.h.
 *
 * Semantics.  For batch element n and query i, the result is the K smallest pairs (d(i, j), j) over the refs j in
 * LEXICOGRAPHIC order: ascending d, ties to the lower j.  d is the fp32 squared distance evaluated as
 *     dx = a.x - b.x; dy = a.y - b.y; dz = a.z - b.z; d = (dx * dx + dy * dy) + dz * dz
 * with every operation rounded in fp32 and no fused multiply-add (a = p1[n, i], b = p2[n, j]).  `dists` is that d bit for
 * bit.  The order is total, so the result does not depend on the order in which candidates are visited: culled and
 * unculled searches return the same bits.  Inputs must be finite.
 *
 * Conventions (those of exa_raster.h / exa_mesh.h)
 *   - plain C types only: device pointers, sizes, a `hipStream_t` passed as `void*`.
 *   - every pointer marked [dev] is a device pointer owned by the caller; the library allocates nothing and keeps no
 *     state between calls.  The workspace size follows from (N, P1, P2, K) alone (exa_knn_workspace_size).
 *   - fp32 points, int64 indices; contiguous row-major arrays.
 *   - work is enqueued on `stream`; no call synchronises the device, so a call can be captured into a hipGraph.
 *   - return value: 0 = ok; < 0 = invalid argument (EXA_KNN_E_*), checked before any GPU work; > 0 = HIP error code.
 *   - the backward is atomic-free and bit-deterministic: the same inputs give the same bits on every call.
 */
#ifndef EXA_KNN_H
#define EXA_KNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EXA_KNN_VERSION 100             /* 0.1.0.0: first version */
#define EXA_KNN_MAX_K 32                /* 1 <= K <= EXA_KNN_MAX_K */
#define EXA_KNN_MAX_POINTS (1 << 28)    /* P1, P2 per batch element */

#define EXA_KNN_NO_CULL 1u              /* flags: visit every ref (brute force); the result is the same */

#define EXA_KNN_E_INVALID (-1)
#define EXA_KNN_E_NULLPTR (-2)

int exa_knn_version(void);
/* Message of the most recent failing call of this thread ("" if none). */
const char* exa_knn_last_error(void);

/* Bytes of the forward's workspace for N batch elements of P1 queries and P2 refs (0 when there is nothing to search). */
int exa_knn_workspace_size(int32_t N, int32_t P1, int32_t P2, int32_t K, uint64_t* out_bytes);

/* The K nearest refs of every query.
 *   p1          [dev] [N, P1, 3] queries.
 *   p2          [dev] [N, P2, 3] refs.
 *   K           1 .. EXA_KNN_MAX_K, and K <= P2 whenever N * P1 > 0.
 *   flags       0 or EXA_KNN_NO_CULL.
 *   workspace   [dev] at least exa_knn_workspace_size bytes (unused with EXA_KNN_NO_CULL); every byte it reads, the call
 *               has written first.
 *   dists       [dev] [N, P1, K] ascending squared distances.
 *   idx         [dev] [N, P1, K] int64 ref indices in [0, P2).
 *   wave_refs   [dev] [N, ceil(P1 / 64)] or NULL: diagnostics, the number of refs each group of 64 queries compared
 *               against (groups in the search's own query order).  Not written when NULL. */
int exa_knn_forward(int32_t N, int32_t P1, int32_t P2, int32_t K, const float* p1, const float* p2, uint32_t flags,
                    void* workspace, uint64_t workspace_bytes, float* dists, int64_t* idx, uint32_t* wave_refs,
                    void* stream);

/* Gradients of the forward's outputs dists and knn = p2[idx] with respect to both point sets:
 *   grad_p1[n, i] = sum_k 2 g[n, i, k] (p1[n, i] - p2[n, idx[n, i, k]])                                 (k ascending)
 *   grad_p2[n, j] = sum over entries e = i * K + k with idx[n, i, k] = j, in the order of `order`, of
 *                   -2 g[n, i, k] (p1[n, i] - p2[n, j]) + grad_knn[n, i, k]
 * No floating-point atomics: every output element is one thread's sum in a fixed order.
 *   idx         [dev] [N, P1, K] int64: the forward's result.
 *   grad_dists  [dev] [N, P1, K] or NULL (zero).
 *   grad_knn    [dev] [N, P1, K, 3] or NULL (zero).
 *   sorted_idx  [dev] [N, P1 * K] int64: idx[n] flattened and sorted ascending, per batch element.
 *   order       [dev] [N, P1 * K] int64: the entries e of idx[n] in that sorted order, a STABLE sort (equal indices keep
 *               ascending e), e.g. torch.sort(idx.view(N, -1), dim=1, stable=True).
 *   grad_p1     [dev] [N, P1, 3], fully written.
 *   grad_p2     [dev] [N, P2, 3], fully written (refs no query chose get 0). */
int exa_knn_backward(int32_t N, int32_t P1, int32_t P2, int32_t K, const float* p1, const float* p2, const int64_t* idx,
                     const float* grad_dists, const float* grad_knn, const int64_t* sorted_idx, const int64_t* order,
                     float* grad_p1, float* grad_p2, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EXA_KNN_H */
