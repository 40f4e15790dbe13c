/*
 * exa_mlp.h -- C ABI of the MI355X-native fused MLP (ExAvatar's make_linear_layers(..., use_gn=True) trunks + heads).
 *
 * This is the native boundary under the four MLPs of the reference's HumanGaussian (avatar/common/nets/module.py:279-287,
 * called at 459-509 and 524-528): L trunk layers Linear -> GroupNorm(G, 128) -> ReLU, 128 wide, followed by 1-4 plain
 * Linear heads read from the last trunk activation.  The Python drop-in over it is `exavatar_release_amd.mlp.FusedMLP`.
 * It lives in the same `libexa_raster.so` as the other exa_*.h headers.
 *
 * Notation.  N rows.  x [N, K0] the per-row input (1 <= K0 <= EXA_MLP_MAX_IN), p [S] an optional shared block (the same
 * for every row), W_0 [128, K0] the per-row columns and Ws [128, S] the shared columns of the first layer's weight,
 * W_l [128, 128] (l >= 1), b_l, gamma_l, beta_l [128], Wh [nh, 128] and bh [nh] the heads stacked in order
 * (1 <= nh <= EXA_MLP_MAX_OUT).  fl() is one fp32 rounding to nearest even; fma(a, b, c) is fp32 fmaf (one rounding).
 * Every operation below is one fp32 operation in the order written; there is no other contraction (the kernels are
 * compiled with -ffp-contract=off).
 *
 * The k order.  Every Linear (and every product with a weight in the backward) sums over its k index in the order
 *     pi(K) = for q = 0 .. Kp/8 - 1, for j = 0 .. 3:  8q + j, 8q + j + 4
 * i.e. 0, 4, 1, 5, 2, 6, 3, 7, 8, 12, 9, 13, ...  over K zero-padded to Kp = ceil(K / 8) * 8: the padded terms are
 * fma(+0, +0, acc) (they only turn an exact -0 into +0).  This is the order of v_mfma_f32_32x32x2_f32 chains whose B
 * operand is a previous accumulator.
 *
 * Forward, per row (every row independently; the result bits do not depend on N or on the row's position):
 *   folded bias   b'_j = fma(Ws[j][S-1], p[S-1], ... fma(Ws[j][1], p[1], fma(Ws[j][0], p[0], b_0[j])))   (b' = b_0 if S=0)
 *                 c ascending, once per call: the shared block enters the first layer as its bias.
 *   Linear        z_j = acc over k in pi(K) of acc = fma(W[j][k], in[k], acc), from acc = b'_j (layer 0) or b_l[j].
 *   GroupNorm     channels 32t + c of 128 are held as 4 tiles t; G groups of n = 128 / G channels (G in {1, 2, 4}), group
 *                 g = tiles g*4/G .. (g+1)*4/G - 1.  Within a tile the channel of register r (0..15) of lane half h is
 *                 ch(r, h) = (r & 3) + 8 (r >> 2) + 4 h.  For each group:
 *                   S_h   = (((+0 + z_a) + z_b) + ...)   over the group's tiles ascending, r ascending, channels ch(r, h)
 *                   mean  = fl(S_0 + S_1) / n
 *                   d_c   = z_c - mean
 *                   V_h   = (((+0 + fl(d_a * d_a)) + fl(d_b * d_b)) + ...)   same order
 *                   var   = fl(V_0 + V_1) / n
 *                   rstd  = 1 / sqrtf(var + eps)           (correctly rounded sqrt and divide, no rsqrt)
 *                   xhat_c = d_c * rstd
 *                   y_c   = fl(xhat_c * gamma_c) + beta_c
 *   ReLU          a_c = y_c if y_c > 0 or y_c is NaN, else +0 (torch.relu).
 *   Heads         out_o = acc over k in pi(128) of fma(Wh[o][k], a_k, acc), from bh[o].
 *
 * Backward, per row, from the head gradients g [N, nh] (a head without a gradient counts as zeros):
 *   dA_k   = acc over o in pi(nh) of fma(Wh[o][k], g_o, acc), from +0
 *   then for l = L-1 .. 0, with xhat, rstd of the forward (recomputed bit-identically):
 *     dY_c   = dA_c if y_c > 0 else +0      (the gradient passes where the ReLU's output is > 0)
 *     e_c    = dY_c * gamma_c
 *     m1     = fl(E1_0 + E1_1) / n,  E1_h = (((+0 + e_a) + e_b) + ...)                 the GroupNorm order above
 *     m2     = fl(E2_0 + E2_1) / n,  E2_h = (((+0 + fl(e_a * xhat_a)) + ...)
 *     dZ_c   = rstd * ((e_c - m1) - fl(xhat_c * m2))
 *     dIn_k  = acc over c in pi(128) of fma(W_l[c][k], dZ_c, acc), from +0   (dA of layer l-1, or the input gradient
 *              dx for l = 0; dx covers x's K0 columns only: the shared block gets no gradient)
 * Parameter gradients are sums over rows of per-row terms:
 *     grad W_l[j][k] = sum of fma-chained dZ_j * in_k      grad b_l[j] = sum of dZ_j
 *     grad gamma_l[c] = sum of fl(dY_c * xhat_c)           grad beta_l[c] = sum of dY_c
 *     grad Wh[o][k] = sum of fma-chained g_o * a_k          grad bh[o] = sum of g_o
 * where in_k is x (l = 0) or the previous layer's activation a.  Every such sum uses one fixed two-level order: the rows
 * are cut into chunks of EXA_MLP_CHUNK in ascending order; each chunk is summed from +0 in ascending row order (the
 * weight gradients as acc = fma(dZ_j, in_k, acc); a chunk with an odd number of rows gets one trailing zero row,
 * fma(+0, +0, acc)); then the chunk partials are summed from +0 in chunk order (plain additions).  The shared block's
 * weight gradient is
 *     grad Ws[j][c] = fl(p[c] * grad b_0[j])
 * with grad b_0[j] the two-level sum above.  No atomics and no memsets: every output element is one thread's sum, so
 * the same inputs give the same bits on every call.  N = 0 gives exact-zero parameter gradients.
 *
 * Conventions (those of exa_knn.h / exa_skin.h)
 *   - plain C types only: device pointers, sizes, a `hipStream_t` passed as `void*`.
 *   - every pointer marked [dev] is a device pointer owned by the caller; the library allocates nothing and keeps no
 *     state between calls.  The backward's workspace size follows from the net's shape and N alone; every byte of it
 *     the backward reads, it has written first.
 *   - fp32, contiguous row-major arrays (W_0 and Ws with the row strides given in the net).
 *   - work is enqueued on `stream`; no call synchronises the device, so a call can be captured into a hipGraph.
 *   - return value: 0 = ok; < 0 = invalid argument (EXA_MLP_E_*), checked before any GPU work; > 0 = HIP error code.
 */
#ifndef EXA_MLP_H
#define EXA_MLP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EXA_MLP_VERSION 100            /* 0.1.0.0: first version */
#define EXA_MLP_HIDDEN 128             /* trunk width */
#define EXA_MLP_MAX_LAYERS 4           /* 1 <= L (the reference uses 3) */
#define EXA_MLP_MAX_IN 256             /* per-row input columns K0 */
#define EXA_MLP_MAX_SHARED 1024        /* shared columns S */
#define EXA_MLP_MAX_HEADS 4
#define EXA_MLP_MAX_OUT 32             /* total head width nh */
#define EXA_MLP_MAX_ROWS (1 << 26)
#define EXA_MLP_CHUNK 512              /* rows per chunk of the backward's two-level sums */

#define EXA_MLP_E_INVALID (-1)
#define EXA_MLP_E_NULLPTR (-2)

typedef struct exa_mlp_net {
    int32_t n_layers;                          /* L */
    int32_t in_width;                          /* K0 */
    int32_t shared_width;                      /* S (0: no shared block) */
    int32_t groups;                            /* G: 1, 2 or 4 */
    int32_t n_heads;                           /* 1 .. EXA_MLP_MAX_HEADS */
    int32_t head_width[EXA_MLP_MAX_HEADS];     /* each >= 1; their sum nh <= EXA_MLP_MAX_OUT */
    int32_t ld_w0;                             /* row stride of W_0 (>= K0) */
    int32_t ld_ws;                             /* row stride of Ws (>= S) */
    float eps[EXA_MLP_MAX_LAYERS];
    const float* W[EXA_MLP_MAX_LAYERS];        /* [dev] W_0 [128, ld_w0], W_l [128, 128] */
    const float* b[EXA_MLP_MAX_LAYERS];        /* [dev] [128] */
    const float* gamma[EXA_MLP_MAX_LAYERS];    /* [dev] [128] */
    const float* beta[EXA_MLP_MAX_LAYERS];     /* [dev] [128] */
    const float* Ws;                           /* [dev] [128, ld_ws], NULL when S == 0 */
    const float* shared;                       /* [dev] [S], NULL when S == 0 */
    const float* Wh;                           /* [dev] [nh, 128] */
    const float* bh;                           /* [dev] [nh] */
} exa_mlp_net;

int exa_mlp_version(void);
/* Message of the most recent failing call of this thread ("" if none). */
const char* exa_mlp_last_error(void);

/* Number of fp32 elements of the flat parameter gradient: for l = 0 .. L-1 in turn W_l (128 K_l, K_0 = K0, else 128),
 * b_l, gamma_l, beta_l (128 each); then Wh (nh * 128) and bh (nh). */
int exa_mlp_param_count(const exa_mlp_net* net, int64_t* out_count);

/* Bytes of the backward's workspace: L N (256 + 12) fp32 per-row terms (xhat, dY and the group statistics of every
 * layer) plus ceil(N / EXA_MLP_CHUNK) * param_count fp32 chunk partials. */
int exa_mlp_workspace_size(const exa_mlp_net* net, int32_t N, uint64_t* out_bytes);

/* The heads.  x [dev] [N, K0]; out: host array of n_heads [dev] pointers, head i [N, head_width[i]], fully written. */
int exa_mlp_forward(const exa_mlp_net* net, int32_t N, const float* x, float* const* out, void* stream);

/* Gradients of the forward (the header's orders, no atomics).
 *   grad_out     host array of n_heads pointers, each [dev] [N, head_width[i]] or NULL (zero gradient).
 *   grad_x       [dev] [N, K0] or NULL (not written).
 *   grad_params  [dev] [param_count] or NULL (not written); the flat layout of exa_mlp_param_count.
 *   grad_ws      [dev] [128, S] (contiguous) or NULL.
 *   workspace    [dev] at least exa_mlp_workspace_size bytes (may be NULL when that is 0). */
int exa_mlp_backward(const exa_mlp_net* net, int32_t N, const float* x, const float* const* grad_out, float* grad_x,
                     float* grad_params, float* grad_ws, void* workspace, uint64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EXA_MLP_H */
