/*
 * exa_triplane.h -- C ABI of the MI355X-native triplane feature lookup (ExAvatar's `extract_tri_feature`).
 *
 * This is the native boundary under the per-sample triplane lookup of the reference's HumanGaussian
 * (avatar/common/nets/module.py:424-457): three bilinear `F.grid_sample`s per plane set, a body set and a face set, whose
 * results are concatenated per vertex.  The Python drop-in over it is `exavatar_release_amd.triplane.TriplaneFeatures`.
 * It lives in the same `libexa_raster.so` as include/exa_raster.h, include/exa_mesh.h and include/exa_knn.h.
 *
 * Inputs.  Two plane sets, `body` and `face`, each [3, C, H, W] fp32 (the same shape).  N rows, each with a normalised
 * coordinate g = (gx, gy, gz) fp32 and a selector: row i reads the face set if is_face[i] != 0, else the body set.  Plane
 * k samples (u, v) = (gx, gy), (gx, gz), (gy, gz) for k = 0, 1, 2; u indexes W and v indexes H.
 *
 * Forward.  F.grid_sample, bilinear, padding_mode='zeros', align_corners=False, evaluated operation by operation in fp32
 * with no fused multiply-add:
 *     ix = ((u + 1) * W - 1) / 2          iy = ((v + 1) * H - 1) / 2
 *     x0 = floor(ix), x1 = x0 + 1, y0 = floor(iy), y1 = y0 + 1
 *     nw = (x1 - ix) * (y1 - iy)   ne = (ix - x0) * (y1 - iy)   sw = (x1 - ix) * (iy - y0)   se = (ix - x0) * (iy - y0)
 *     out[i, k*C + c] = (((0 + P[y0,x0]*nw) + P[y0,x1]*ne) + P[y1,x0]*sw) + P[y1,x1]*se
 * where P = set[k, c] and a term is present only when its texel lies in [0, W) x [0, H).  `out` is [N, 3C] row-major.
 * The taps of a row are numbered t = 0..3 in that order: (x0, y0), (x1, y0), (x0, y1), (x1, y1).
 *
 * Backward.  For every element of both sets, with L(k, y, x) the list of the (row i, tap t) pairs of that set whose tap t
 * on plane k lies on texel (x, y), in ascending i (a row has at most one tap on a texel):
 *     grad_set[k, c, y, x] = sum over L, in the fixed two-level order below, of fl(g[i, k*C + c] * w(i, k, t))
 * with w the weight above.  The list is cut into consecutive segments of S entries (the last one shorter; S is the plan's
 * segment length, a power of two >= 32).  Each segment's partial is the sequential fp32 sum of its products from +0, and
 * the gradient is the sequential fp32 sum of the partials from +0 in segment order.  A list of at most S entries is
 * therefore the plain sequential sum.  Every element of both gradients is written: texels no row touches get exactly 0.
 * Rows of one set add nothing to the other set.  The coordinates get no gradient.
 *
 * The plan.  The coordinates are constant for the life of a model, so the lists are built once:
 *   1. exa_triplane_plan_keys writes one key per (row, plane, tap), entry e = (i * 3 + k) * 4 + t:
 *        key = s * 3HW + k * HW + y * W + x   (s = 1 for a face row, 0 for a body row; texel space T = 6HW)
 *      or T when the tap is out of bounds.
 *   2. The caller sorts the keys STABLY (equal keys keep ascending e, hence ascending i), e.g.
 *      torch.sort(keys, stable=True), and keeps the sorted entry ids `entries` (int32) and `offsets` [T + 1], the CSR of
 *      each texel's run in the sorted keys (the out-of-bounds tail past offsets[T] is never read).
 *   3. The caller cuts each texel's run into segments of S entries: seg_entry [NSEG + 1] holds the first entry position
 *      of every segment in texel order, and seg_entry[NSEG] = offsets[T]; tex_seg [T + 1] holds each texel's first segment
 *      (texel t owns segments [tex_seg[t], tex_seg[t + 1]), none when its list is empty).
 *   4. The caller packs consecutive texels into workgroups: wg_tex [num_wg + 1], with wg_tex[0] = 0 and
 *      wg_tex[num_wg] = T, workgroup w owning texels [wg_tex[w], wg_tex[w + 1]).  A workgroup holds at most
 *      max_wg_segments segments (its partials live in LDS: max_wg_segments * C * 4 <= EXA_TRIPLANE_MAX_LDS bytes).
 *   exavatar_release_amd/triplane.py builds the plan exactly so.  The tables change the order of nothing but the
 *   segments; S fixes the result.
 *
 * Conventions (those of exa_knn.h)
 *   - plain C types only: device pointers, sizes, a `hipStream_t` passed as `void*`.
 *   - every pointer marked [dev] is a device pointer owned by the caller; the library allocates nothing and keeps no
 *     state between calls.
 *   - fp32 planes, coordinates and gradients; int32 plan tables; uint8 selectors; contiguous row-major arrays.
 *   - work is enqueued on `stream`; no call synchronises the device, so a call can be captured into a hipGraph.
 *   - return value: 0 = ok; < 0 = invalid argument (EXA_TRIPLANE_E_*), checked before any GPU work; > 0 = HIP error code.
 *   - the backward uses no atomics and no memsets: the same inputs give the same bits on every call.
 *   - coordinates must be finite.
 */
#ifndef EXA_TRIPLANE_H
#define EXA_TRIPLANE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EXA_TRIPLANE_VERSION 100            /* 0.1.0.0: first version */
#define EXA_TRIPLANE_MAX_C 1024             /* 1 <= C <= EXA_TRIPLANE_MAX_C */
#define EXA_TRIPLANE_MAX_ROWS (1 << 27)     /* N: the 12 N plan entries stay below 2^31 */
#define EXA_TRIPLANE_MAX_TEXELS (1 << 28)   /* 6 H W */
#define EXA_TRIPLANE_MAX_LDS 65536          /* bytes of one backward workgroup's partials */

#define EXA_TRIPLANE_E_INVALID (-1)
#define EXA_TRIPLANE_E_NULLPTR (-2)

int exa_triplane_version(void);
/* Message of the most recent failing call of this thread ("" if none). */
const char* exa_triplane_last_error(void);

/* Step 1 of the plan: the texel key of every (row, plane, tap).
 *   coords   [dev] [N, 3] normalised coordinates.
 *   is_face  [dev] [N] uint8, nonzero = face row.
 *   keys     [dev] [N * 12] int32, fully written. */
int exa_triplane_plan_keys(int32_t N, int32_t H, int32_t W, const float* coords, const uint8_t* is_face, int32_t* keys,
                           void* stream);

/* The lookup.
 *   body, face  [dev] [3, C, H, W] each.
 *   coords      [dev] [N, 3].
 *   is_face     [dev] [N] uint8.
 *   out         [dev] [N, 3C], fully written. */
int exa_triplane_forward(int32_t N, int32_t C, int32_t H, int32_t W, const float* body, const float* face,
                         const float* coords, const uint8_t* is_face, float* out, void* stream);

/* Gradients of both plane sets from grad_out [N, 3C] (the header's two-level order, no atomics).
 *   coords       [dev] [N, 3], the coordinates the plan was built from.
 *   grad_out     [dev] [N, 3C].
 *   entries      [dev] [>= seg_entry[NSEG]] int32 sorted entry ids (plan step 2).
 *   seg_entry    [dev] [NSEG + 1] int32 (plan step 3).
 *   tex_seg      [dev] [6 H W + 1] int32 (plan step 3).
 *   wg_tex       [dev] [num_wg + 1] int32 (plan step 4); num_wg >= 1.
 *   max_wg_segments  the most segments any workgroup holds (>= 1; max_wg_segments * C * 4 <= EXA_TRIPLANE_MAX_LDS).
 *   grad_body, grad_face  [dev] [3, C, H, W] each, fully written. */
int exa_triplane_backward(int32_t N, int32_t C, int32_t H, int32_t W, const float* coords, const float* grad_out,
                          const int32_t* entries, const int32_t* seg_entry, const int32_t* tex_seg,
                          const int32_t* wg_tex, int32_t num_wg, int32_t max_wg_segments, float* grad_body,
                          float* grad_face, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EXA_TRIPLANE_H */
