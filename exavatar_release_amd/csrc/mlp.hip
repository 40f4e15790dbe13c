// Fused Linear -> GroupNorm -> ReLU MLP (include/exa_mlp.h): the trunks and heads of ExAvatar's four per-Gaussian MLPs
// (reference module.py:279-287, 459-509, 524-528) and a reproducible, atomic-free backward.  The semantics -- the k
// order of every product, the GroupNorm's summation order and the backward's two-level row sums -- are written out in
// the header; this file implements them.
//
//   mlp_fwd        one workgroup of 4 waves per 128 rows, one wave per 32 rows.  A layer is Z^T = W . X^T on
//                  v_mfma_f32_32x32x2_f32: a row is one accumulator column (lane & 31), its 128 channels sit in the
//                  four 16-register tiles of the two lane halves, so GroupNorm needs only one exchange between lane l
//                  and l + 32, and the next layer takes the accumulator registers as its B operand with no LDS round
//                  trip.  The weights are staged in LDS per layer (64 KiB, in fragment order: one ds_read_b128 per
//                  lane gives four k steps of one tile).  The heads run in the same launch.
//   mlp_bwd_rows   the same tiling.  It recomputes the forward, writing every layer's xhat and rstd to the workspace,
//                  then runs the backward layer by layer (dY, the GroupNorm backward, dIn = W^T dZ with W^T staged in
//                  LDS), writing dY and the group means m1, m2, and finally the input gradient.
//   mlp_bwd_chunk  one workgroup per (chunk of EXA_MLP_CHUNK rows, layer or head).  Wave w accumulates the weight
//                  gradient tiles of output rows 32w .. 32w+31 over the chunk's rows in ascending order (the rows are
//                  the MFMA's k), rebuilding dZ and the layer input from the workspace; threads 0 .. 127 add the
//                  bias, gamma and beta terms in ascending row order.  Partials go to the workspace.
//   mlp_bwd_sum    one thread per parameter gradient element: the chunk partials in chunk order; the shared block's
//                  weight gradient as p[c] * grad b_0[j].
// No atomics, no memsets: every output element is one thread's sum in the header's order.
// Compiled with -ffp-contract=off (build.py): the VALU arithmetic is exactly the header's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/exa_mlp.h"
#include "abi_status.h"

namespace exa_mlp_impl {

using exa::ceil_div;

constexpr int H = EXA_MLP_HIDDEN;
constexpr int MAXL = EXA_MLP_MAX_LAYERS;
constexpr int MAXH = EXA_MLP_MAX_HEADS;
constexpr int MAXO = EXA_MLP_MAX_OUT;
constexpr int CHUNK = EXA_MLP_CHUNK;
constexpr int BLOCK = 256;                   // 4 waves
constexpr int ROWS = 128;                    // rows per workgroup of mlp_fwd / mlp_bwd_rows (32 per wave)
constexpr int SLAB = 128;                    // k columns (or output columns) per LDS stage: 128 x 128 floats = 64 KiB
constexpr int IMG = SLAB * H;                // floats of one staged image
constexpr int STAT = 12;                     // per row and layer: rstd[4], m1[4], m2[4]
constexpr int BATCH = 8;                     // rows (or k steps) whose loads mlp_bwd_chunk issues together
static_assert(CHUNK % 2 == 0, "the chunk is a whole number of MFMA k steps");

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Params {
    exa_mlp_net net;
    int32_t N;
    int32_t nh;
    int32_t head_off[MAXH + 1];
    const float* x;
    float* out[MAXH];
    const float* gout[MAXH];
    float* gx;
    float* xhat;                              // [L][N][128]
    float* dy;                                // [L][N][128]
    float* stat;                              // [L][N][STAT]
    float* part;                              // [nchunks][P]
    float* gparams;                           // [P]
    float* gws;                               // [128][S]
    int64_t P;
    int64_t off_w[MAXL], off_b[MAXL], off_g[MAXL], off_be[MAXL], off_wh, off_bh;
    int32_t nchunks;
};

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// channel (within a 32-channel tile) of accumulator register r in lane half h
__device__ __forceinline__ int chan(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ float relu(float y) { return (y > 0.f || y != y) ? y : 0.f; }

__device__ __forceinline__ float other_half(float v) { return __shfl_xor(v, 32); }

// Stage rows [0, M) x columns [k0, k0 + kn) of a row-major [M, ld] matrix as the A image of Out^T = A . B:
// img[((q * T + t) * 64 + lane) * 4 + j] = A[32 t + (lane & 31)][k0 + 8 q + j + 4 (lane >> 5)], zero outside.
// T = ceil(M / 32) tiles; kn is padded to 8.
__device__ void stage_a(float* img, const float* A, int ld, int M, int k0, int kn, int K, int T, int tid) {
    const int kp = (kn + 7) & ~7;
    const int tot = T * 32 * kp;
    for (int e = tid; e < tot; e += BLOCK) {
        const int o = e / kp, kk = e - o * kp;
        const int k = k0 + kk;
        const float v = (o < M && kk < kn && k < K) ? A[(int64_t)o * ld + k] : 0.f;
        const int q = kk >> 3, hh = (kk >> 2) & 1, j = kk & 3, t = o >> 5, lane = (o & 31) + 32 * hh;
        img[((q * T + t) * 64 + lane) * 4 + j] = v;
    }
}

// Stage the transpose: the A image of Out^T = W^T . B for W [M, ld] (M rows = the k of this product, padded to 8),
// output columns [i0, i0 + 128) of W:  img[((q * 4 + t) * 64 + lane) * 4 + j] = W[8q + j + 4 (lane >> 5)][i0 + 32 t + (lane & 31)].
__device__ void stage_at(float* img, const float* W, int ld, int M, int i0, int Kw, int tid) {
    const int mp = (M + 7) & ~7;
    const int tot = mp * SLAB;
    for (int e = tid; e < tot; e += BLOCK) {
        const int c = e / SLAB, ii = e - c * SLAB;
        const int i = i0 + ii;
        const float v = (c < M && i < Kw) ? W[(int64_t)c * ld + i] : 0.f;
        const int q = c >> 3, hh = (c >> 2) & 1, j = c & 3, t = ii >> 5, lane = (ii & 31) + 32 * hh;
        img[((q * 4 + t) * 64 + lane) * 4 + j] = v;
    }
}

// acc[t] += A(img) . in over kq q-steps, the B operand taken from in[] by the caller's functor
template <int T, class Load>
__device__ __forceinline__ void chain(const float* img, int nq, int lane, f32x16* acc, Load load) {
    for (int q = 0; q < nq; ++q) {
        float4 a[T];
#pragma unroll
        for (int t = 0; t < T; ++t) a[t] = *reinterpret_cast<const float4*>(img + ((q * T + t) * 64 + lane) * 4);
        float b[4];
        load(q, b);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            acc[t] = mfma(a[t].x, b[0], acc[t]);
            acc[t] = mfma(a[t].y, b[1], acc[t]);
            acc[t] = mfma(a[t].z, b[2], acc[t]);
            acc[t] = mfma(a[t].w, b[3], acc[t]);
        }
    }
}

// The same with the B operand an accumulator image src[4] (the 128 channels of the lane's row): q = 4 ts + rq.
template <int T>
__device__ __forceinline__ void chain_regs(const float* img, int lane, f32x16* acc, const f32x16* src) {
#pragma unroll
    for (int ts = 0; ts < 4; ++ts) {
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            const int q = 4 * ts + rq;
            float4 a[T];
#pragma unroll
            for (int t = 0; t < T; ++t) a[t] = *reinterpret_cast<const float4*>(img + ((q * T + t) * 64 + lane) * 4);
#pragma unroll
            for (int t = 0; t < T; ++t) {
                acc[t] = mfma(a[t].x, src[ts][4 * rq + 0], acc[t]);
                acc[t] = mfma(a[t].y, src[ts][4 * rq + 1], acc[t]);
                acc[t] = mfma(a[t].z, src[ts][4 * rq + 2], acc[t]);
                acc[t] = mfma(a[t].w, src[ts][4 * rq + 3], acc[t]);
            }
        }
    }
}

// Per-group sums in the header's order: S_h over the group's tiles ascending, r ascending, then S_0 + S_1.
// F(t, r) gives the term.  TPG = tiles per group (4 / G).  out[t] = the total of tile t's group.
template <int TPG, class F>
__device__ __forceinline__ void group_sums(float* out, F term) {
#pragma unroll
    for (int g = 0; g < 4 / TPG; ++g) {
        float s = 0.f;
#pragma unroll
        for (int u = 0; u < TPG; ++u) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s = s + term(g * TPG + u, r);
        }
        s = s + other_half(s);
#pragma unroll
        for (int u = 0; u < TPG; ++u) out[g * TPG + u] = s;
    }
}

// GroupNorm + ReLU in place on acc (-> a); xh gets xhat, rs[t] the rstd of tile t's group.
template <int TPG>
__device__ __forceinline__ void gn_relu(f32x16* acc, f32x16* xh, float* rs, const float* gamma, const float* beta,
                                        float eps, int h) {
    const float n = (float)(32 * TPG);
    float mean[4], var[4];
    group_sums<TPG>(mean, [&](int t, int r) { return acc[t][r]; });
#pragma unroll
    for (int t = 0; t < 4; ++t) mean[t] = mean[t] / n;
    group_sums<TPG>(var, [&](int t, int r) { const float d = acc[t][r] - mean[t]; return d * d; });
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float v = var[t] / n;
        rs[t] = 1.0f / sqrtf(v + eps);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = 32 * t + chan(r, h);
            const float x = (acc[t][r] - mean[t]) * rs[t];
            xh[t][r] = x;
            acc[t][r] = relu(x * gamma[c] + beta[c]);
        }
    }
}

__device__ __forceinline__ float load_gout(const Params& P, int64_t row, int o) {
    if (o >= P.nh) return 0.f;
    int hd = 0;
#pragma unroll
    for (int i = 1; i < MAXH; ++i) hd += (o >= P.head_off[i]) ? 1 : 0;
    const float* g = P.gout[hd];
    const int w = P.head_off[hd + 1] - P.head_off[hd];
    return g ? g[row * w + (o - P.head_off[hd])] : 0.f;
}

// folded first-layer bias b'_j into bl[0..127]
__device__ __forceinline__ void fold_bias(const Params& P, float* bl, int tid) {
    const exa_mlp_net& n = P.net;
    if (tid < H) {
        float acc = n.b[0][tid];
        for (int c = 0; c < n.shared_width; ++c) acc = fmaf(n.Ws[(int64_t)tid * n.ld_ws + c], n.shared[c], acc);
        bl[tid] = acc;
    }
}

// The trunk's forward for the wave's 32 rows; optionally records xhat and rstd (backward).  Leaves a in acc.
template <int TPG, bool SAVE>
__device__ void trunk_fwd(const Params& P, float* img, const float* bl, f32x16* acc, int64_t row, bool valid, int lane,
                          int h, int tid) {
    const exa_mlp_net& n = P.net;
    const int K0 = n.in_width;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = bl[32 * t + chan(r, h)];
    for (int k0 = 0; k0 < K0; k0 += SLAB) {
        const int kn = min(SLAB, K0 - k0);
        __syncthreads();
        stage_a(img, n.W[0], n.ld_w0, H, k0, kn, K0, 4, tid);
        __syncthreads();
        const float* xr = P.x + row * K0;
        chain<4>(img, (kn + 7) >> 3, lane, acc, [&](int q, float* b) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + 8 * q + j + 4 * h;
                b[j] = (valid && k < K0) ? xr[k] : 0.f;
            }
        });
    }
    for (int l = 0; l < n.n_layers; ++l) {
        if (l > 0) {
            f32x16 a[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                a[t] = acc[t];
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = n.b[l][32 * t + chan(r, h)];
            }
            __syncthreads();
            stage_a(img, n.W[l], H, H, 0, H, H, 4, tid);
            __syncthreads();
            chain_regs<4>(img, lane, acc, a);
        }
        f32x16 xh[4];
        float rs[4];
        gn_relu<TPG>(acc, xh, rs, n.gamma[l], n.beta[l], n.eps[l], h);
        if (SAVE && valid) {
            float* xo = P.xhat + ((int64_t)l * P.N + row) * H;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq)
                    *reinterpret_cast<float4*>(xo + 32 * t + 8 * rq + 4 * h) =
                        make_float4(xh[t][4 * rq], xh[t][4 * rq + 1], xh[t][4 * rq + 2], xh[t][4 * rq + 3]);
            if (h == 0) {
                float* so = P.stat + ((int64_t)l * P.N + row) * STAT;
                for (int g = 0; g < 4 / TPG; ++g) so[g] = rs[g * TPG];
            }
        }
    }
}

template <int TPG>
__global__ void __launch_bounds__(BLOCK) mlp_fwd(Params P) {
    __shared__ float4 img4[IMG / 4];
    __shared__ float bl[H];
    float* img = reinterpret_cast<float*>(img4);
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
    const int64_t row = (int64_t)blockIdx.x * ROWS + (tid >> 6) * 32 + (lane & 31);
    const bool valid = row < P.N;
    fold_bias(P, bl, tid);
    __syncthreads();
    f32x16 acc[4];
    trunk_fwd<TPG, false>(P, img, bl, acc, row, valid, lane, h, tid);
    // heads: one 32-wide tile
    f32x16 o[1];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int c = chan(r, h);
        o[0][r] = c < P.nh ? P.net.bh[c] : 0.f;
    }
    __syncthreads();
    stage_a(img, P.net.Wh, H, P.nh, 0, H, H, 1, tid);
    __syncthreads();
    chain_regs<1>(img, lane, o, acc);
    if (valid) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = chan(r, h);
            if (c < P.nh) {
                int hd = 0;
#pragma unroll
                for (int i = 1; i < MAXH; ++i) hd += (c >= P.head_off[i]) ? 1 : 0;
                const int w = P.head_off[hd + 1] - P.head_off[hd];
                P.out[hd][row * w + (c - P.head_off[hd])] = o[0][r];
            }
        }
    }
}

template <int TPG>
__global__ void __launch_bounds__(BLOCK) mlp_bwd_rows(Params P) {
    __shared__ float4 img4[IMG / 4];
    __shared__ float bl[H];
    float* img = reinterpret_cast<float*>(img4);
    const exa_mlp_net& n = P.net;
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
    const int64_t row = (int64_t)blockIdx.x * ROWS + (tid >> 6) * 32 + (lane & 31);
    const bool valid = row < P.N;
    const float nf = (float)(32 * TPG);
    fold_bias(P, bl, tid);
    __syncthreads();
    f32x16 acc[4];
    trunk_fwd<TPG, true>(P, img, bl, acc, row, valid, lane, h, tid);
    // dA of the last layer = Wh^T g
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x16(0.f);
    __syncthreads();
    stage_at(img, n.Wh, H, P.nh, 0, H, tid);
    __syncthreads();
    chain<4>(img, (P.nh + 7) >> 3, lane, acc, [&](int q, float* b) {
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = valid ? load_gout(P, row, 8 * q + j + 4 * h) : 0.f;
    });
    for (int l = n.n_layers - 1; l >= 0; --l) {
        f32x16 xh[4], dz[4];
        float rs[4];
        const float* xi = P.xhat + ((int64_t)l * P.N + (valid ? row : 0)) * H;
        float* so = P.stat + ((int64_t)l * P.N + (valid ? row : 0)) * STAT;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                float4 v = valid ? *reinterpret_cast<const float4*>(xi + 32 * t + 8 * rq + 4 * h) : make_float4(0.f, 0.f, 0.f, 0.f);
                xh[t][4 * rq] = v.x; xh[t][4 * rq + 1] = v.y; xh[t][4 * rq + 2] = v.z; xh[t][4 * rq + 3] = v.w;
            }
            // half 0 stored the row's rstd (trunk_fwd); it reads back its own store and hands it to half 1
            const float own = (valid && h == 0) ? so[t / TPG] : 0.f;
            rs[t] = __shfl(own, lane & 31);
        }
        const float* gm = n.gamma[l];
        const float* bt = n.beta[l];
        // dY (stored) and e = dY * gamma (in dz)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = 32 * t + chan(r, h);
                const float y = xh[t][r] * gm[c] + bt[c];
                const float d = y > 0.f ? acc[t][r] : 0.f;
                acc[t][r] = d;
                dz[t][r] = d * gm[c];
            }
        if (valid) {
            float* dyo = P.dy + ((int64_t)l * P.N + row) * H;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq)
                    *reinterpret_cast<float4*>(dyo + 32 * t + 8 * rq + 4 * h) =
                        make_float4(acc[t][4 * rq], acc[t][4 * rq + 1], acc[t][4 * rq + 2], acc[t][4 * rq + 3]);
        }
        float m1[4], m2[4];
        group_sums<TPG>(m1, [&](int t, int r) { return dz[t][r]; });
        group_sums<TPG>(m2, [&](int t, int r) { return dz[t][r] * xh[t][r]; });
#pragma unroll
        for (int t = 0; t < 4; ++t) { m1[t] = m1[t] / nf; m2[t] = m2[t] / nf; }
        if (valid && h == 0) {
            for (int g = 0; g < 4 / TPG; ++g) { so[4 + g] = m1[g * TPG]; so[8 + g] = m2[g * TPG]; }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) dz[t][r] = rs[t] * ((dz[t][r] - m1[t]) - xh[t][r] * m2[t]);
        if (l > 0) {
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = f32x16(0.f);
            __syncthreads();
            stage_at(img, n.W[l], H, H, 0, H, tid);
            __syncthreads();
            chain_regs<4>(img, lane, acc, dz);
        } else if (P.gx) {
            const int K0 = n.in_width;
            for (int i0 = 0; i0 < K0; i0 += SLAB) {
                f32x16 g[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) g[t] = f32x16(0.f);
                __syncthreads();
                stage_at(img, n.W[0], n.ld_w0, H, i0, K0, tid);
                __syncthreads();
                chain_regs<4>(img, lane, g, dz);
                if (valid) {
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int i = i0 + 32 * t + chan(r, h);
                            if (i < K0) P.gx[row * K0 + i] = g[t][r];
                        }
                }
            }
        }
    }
}

// dZ of layer l at (row, c), rebuilt from the workspace exactly as mlp_bwd_rows formed it
template <int TPG>
__device__ __forceinline__ float dz_at(const Params& P, int l, int64_t row, int c, float* dyo, float* xho) {
    const int64_t base = ((int64_t)l * P.N + row);
    const float dy = P.dy[base * H + c];
    const float xh = P.xhat[base * H + c];
    const float* s = P.stat + base * STAT;
    const int g = c / (32 * TPG);
    const float e = dy * P.net.gamma[l][c];
    *dyo = dy;
    *xho = xh;
    return s[g] * ((e - s[4 + g]) - xh * s[8 + g]);
}

__device__ __forceinline__ float act_at(const Params& P, int l, int64_t row, int c) {
    const float xh = P.xhat[((int64_t)l * P.N + row) * H + c];
    return relu(xh * P.net.gamma[l][c] + P.net.beta[l][c]);
}

template <int TPG>
__global__ void __launch_bounds__(BLOCK) mlp_bwd_chunk(Params P) {
    const exa_mlp_net& n = P.net;
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, w = tid >> 6, i = lane & 31;
    const int z = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * CHUNK;
    const int64_t r1 = min((int64_t)P.N, r0 + CHUNK);
    const int nsteps = (int)((r1 - r0 + 1) / 2);
    float* part = P.part + (int64_t)blockIdx.x * P.P;
    if (z < n.n_layers) {
        const int l = z;
        const int K = l == 0 ? n.in_width : H;
        const int TI = (K + 31) / 32;
        f32x16 acc[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] = f32x16(0.f);
        const int c = 32 * w + i;
        // BATCH k steps' operands are loaded before their MFMAs, so that their loads are in flight together; the chain
        // itself runs step by step in order and stops at nsteps
        for (int s0 = 0; s0 < nsteps; s0 += BATCH) {
            float av[BATCH], bv[BATCH][8];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int64_t row = r0 + 2 * (s0 + u) + h;
                const bool valid = s0 + u < nsteps && row < r1;
                float dy, xh;
                av[u] = valid ? dz_at<TPG>(P, l, row, c, &dy, &xh) : 0.f;
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const int k = 32 * t + i;
                    bv[u][t] = (t < TI && valid && k < K) ? (l == 0 ? P.x[row * K + k] : act_at(P, l - 1, row, k)) : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                if (s0 + u < nsteps) {
#pragma unroll
                    for (int t = 0; t < 8; ++t)
                        if (t < TI) acc[t] = mfma(av[u], bv[u][t], acc[t]);
                }
            }
        }
        float* pw = part + P.off_w[l];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            if (t < TI) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int o = 32 * w + chan(r, h), k = 32 * t + i;
                    if (k < K) pw[(int64_t)o * K + k] = acc[t][r];
                }
            }
        }
        if (tid < H) {
            float sb = 0.f, sg = 0.f, sbe = 0.f;
            for (int64_t r = r0; r < r1; r += BATCH) {
                float dv[BATCH], yv[BATCH], xv[BATCH];
#pragma unroll
                for (int u = 0; u < BATCH; ++u) {
                    dv[u] = yv[u] = xv[u] = 0.f;
                    if (r + u < r1) dv[u] = dz_at<TPG>(P, l, r + u, tid, &yv[u], &xv[u]);
                }
#pragma unroll
                for (int u = 0; u < BATCH; ++u) {
                    if (r + u < r1) {
                        sb = sb + dv[u];
                        sg = sg + yv[u] * xv[u];
                        sbe = sbe + yv[u];
                    }
                }
            }
            part[P.off_b[l] + tid] = sb;
            part[P.off_g[l] + tid] = sg;
            part[P.off_be[l] + tid] = sbe;
        }
    } else {
        // heads: wave w holds the tile of input channels 32w .. 32w+31
        const int L = n.n_layers;
        f32x16 acc[1];
        acc[0] = f32x16(0.f);
        for (int s0 = 0; s0 < nsteps; s0 += BATCH) {
            float av[BATCH], bv[BATCH];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int64_t row = r0 + 2 * (s0 + u) + h;
                const bool valid = s0 + u < nsteps && row < r1;
                av[u] = valid ? load_gout(P, row, i) : 0.f;
                bv[u] = valid ? act_at(P, L - 1, row, 32 * w + i) : 0.f;
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u)
                if (s0 + u < nsteps) acc[0] = mfma(av[u], bv[u], acc[0]);
        }
        float* pw = part + P.off_wh;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = chan(r, h);
            if (o < P.nh) pw[o * H + 32 * w + i] = acc[0][r];
        }
        if (tid < P.nh) {
            float sb = 0.f;
            for (int64_t r = r0; r < r1; r += BATCH) {
                float gv[BATCH];
#pragma unroll
                for (int u = 0; u < BATCH; ++u) gv[u] = r + u < r1 ? load_gout(P, r + u, tid) : 0.f;
#pragma unroll
                for (int u = 0; u < BATCH; ++u)
                    if (r + u < r1) sb = sb + gv[u];
            }
            part[P.off_bh + tid] = sb;
        }
    }
}

__global__ void __launch_bounds__(BLOCK) mlp_bwd_sum(Params P) {
    const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int S = P.net.shared_width;
    if (e < P.P) {
        if (!P.gparams) return;
        float s = 0.f;
        for (int c0 = 0; c0 < P.nchunks; c0 += BATCH) {
            float v[BATCH];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) v[u] = c0 + u < P.nchunks ? P.part[(int64_t)(c0 + u) * P.P + e] : 0.f;
#pragma unroll
            for (int u = 0; u < BATCH; ++u)
                if (c0 + u < P.nchunks) s = s + v[u];
        }
        P.gparams[e] = s;
    } else if (e < P.P + (int64_t)H * S) {
        if (!P.gws) return;
        const int64_t f = e - P.P;
        const int j = (int)(f / S), c = (int)(f - (int64_t)j * S);
        float s = 0.f;
        for (int k = 0; k < P.nchunks; ++k) s = s + P.part[(int64_t)k * P.P + P.off_b[0] + j];
        P.gws[f] = P.net.shared[c] * s;
    }
}

EXA_ABI_STATUS("exa_mlp")

int check_net(const exa_mlp_net* n, int* nh_out) {
    if (!n) return fail(EXA_MLP_E_NULLPTR, "net is NULL");
    if (n->n_layers < 1 || n->n_layers > MAXL) return fail(EXA_MLP_E_INVALID, "n_layers must be 1 .. 4");
    if (n->in_width < 1 || n->in_width > EXA_MLP_MAX_IN) return fail(EXA_MLP_E_INVALID, "in_width must be 1 .. 256");
    if (n->shared_width < 0 || n->shared_width > EXA_MLP_MAX_SHARED)
        return fail(EXA_MLP_E_INVALID, "shared_width must be 0 .. 1024");
    if (n->groups != 1 && n->groups != 2 && n->groups != 4) return fail(EXA_MLP_E_INVALID, "groups must be 1, 2 or 4");
    if (n->n_heads < 1 || n->n_heads > MAXH) return fail(EXA_MLP_E_INVALID, "n_heads must be 1 .. 4");
    int nh = 0;
    for (int i = 0; i < n->n_heads; ++i) {
        if (n->head_width[i] < 1) return fail(EXA_MLP_E_INVALID, "every head_width must be >= 1");
        nh += n->head_width[i];
    }
    if (nh > MAXO) return fail(EXA_MLP_E_INVALID, "the heads' total width must be <= 32");
    if (n->ld_w0 < n->in_width) return fail(EXA_MLP_E_INVALID, "ld_w0 < in_width");
    if (n->shared_width > 0 && n->ld_ws < n->shared_width) return fail(EXA_MLP_E_INVALID, "ld_ws < shared_width");
    for (int l = 0; l < n->n_layers; ++l) {
        if (!n->W[l] || !n->b[l] || !n->gamma[l] || !n->beta[l])
            return fail(EXA_MLP_E_NULLPTR, "a trunk parameter is NULL");
        if (!(n->eps[l] >= 0.f)) return fail(EXA_MLP_E_INVALID, "eps must be >= 0");
    }
    if (n->shared_width > 0 && (!n->Ws || !n->shared)) return fail(EXA_MLP_E_NULLPTR, "Ws or shared is NULL");
    if (!n->Wh || !n->bh) return fail(EXA_MLP_E_NULLPTR, "Wh or bh is NULL");
    *nh_out = nh;
    return 0;
}

int64_t layout(const exa_mlp_net* n, int nh, Params* P) {
    int64_t o = 0;
    for (int l = 0; l < n->n_layers; ++l) {
        const int K = l == 0 ? n->in_width : H;
        if (P) P->off_w[l] = o;
        o += (int64_t)H * K;
        if (P) P->off_b[l] = o;
        o += H;
        if (P) P->off_g[l] = o;
        o += H;
        if (P) P->off_be[l] = o;
        o += H;
    }
    if (P) P->off_wh = o;
    o += (int64_t)nh * H;
    if (P) P->off_bh = o;
    o += nh;
    return o;
}

int64_t nchunks_for(int32_t N) { return ((int64_t)N + CHUNK - 1) / CHUNK; }

uint64_t ws_bytes(const exa_mlp_net* n, int nh, int32_t N) {
    return 4ull * ((uint64_t)n->n_layers * (uint64_t)N * (2 * H + STAT) + (uint64_t)nchunks_for(N) * layout(n, nh, nullptr));
}

int setup(const exa_mlp_net* net, int32_t N, Params& P) {
    int nh = 0;
    if (int rc = check_net(net, &nh)) return rc;
    if (N < 0 || N > EXA_MLP_MAX_ROWS) return fail(EXA_MLP_E_INVALID, "N must be 0 .. 2^26");
    memset(&P, 0, sizeof(P));
    P.net = *net;
    P.N = N;
    P.nh = nh;
    P.head_off[0] = 0;
    for (int i = 0; i < MAXH; ++i) P.head_off[i + 1] = P.head_off[i] + (i < net->n_heads ? net->head_width[i] : 0);
    for (int i = net->n_heads + 1; i <= MAXH; ++i) P.head_off[i] = 1 << 30;   // unused heads: never selected
    P.P = layout(net, nh, &P);
    P.nchunks = (int32_t)nchunks_for(N);
    return 0;
}

}  // namespace exa_mlp_impl

using namespace exa_mlp_impl;

#define EXA_MLP_DISPATCH(KERNEL, GRID, SHMEM)                                                                          \
    switch (4 / P.net.groups) {                                                                                        \
    case 1: hipLaunchKernelGGL(KERNEL<1>, GRID, dim3(BLOCK), SHMEM, st, P); break;                                     \
    case 2: hipLaunchKernelGGL(KERNEL<2>, GRID, dim3(BLOCK), SHMEM, st, P); break;                                     \
    default: hipLaunchKernelGGL(KERNEL<4>, GRID, dim3(BLOCK), SHMEM, st, P); break;                                    \
    }

extern "C" {

int exa_mlp_version(void) { return EXA_MLP_VERSION; }

const char* exa_mlp_last_error(void) { return g_err; }

int exa_mlp_param_count(const exa_mlp_net* net, int64_t* out_count) {
    int nh = 0;
    if (!out_count) return fail(EXA_MLP_E_NULLPTR, "out_count is NULL");
    if (int rc = check_net(net, &nh)) return rc;
    *out_count = layout(net, nh, nullptr);
    return 0;
}

int exa_mlp_workspace_size(const exa_mlp_net* net, int32_t N, uint64_t* out_bytes) {
    int nh = 0;
    if (!out_bytes) return fail(EXA_MLP_E_NULLPTR, "out_bytes is NULL");
    if (int rc = check_net(net, &nh)) return rc;
    if (N < 0 || N > EXA_MLP_MAX_ROWS) return fail(EXA_MLP_E_INVALID, "N must be 0 .. 2^26");
    *out_bytes = ws_bytes(net, nh, N);
    return 0;
}

int exa_mlp_forward(const exa_mlp_net* net, int32_t N, const float* x, float* const* out, void* stream) {
    Params P;
    if (int rc = setup(net, N, P)) return rc;
    if (N == 0) return 0;
    if (!x || !out) return fail(EXA_MLP_E_NULLPTR, "x or out is NULL");
    for (int i = 0; i < net->n_heads; ++i) {
        if (!out[i]) return fail(EXA_MLP_E_NULLPTR, "an out pointer is NULL");
        P.out[i] = out[i];
    }
    P.x = x;
    hipStream_t st = (hipStream_t)stream;
    EXA_MLP_DISPATCH(mlp_fwd, dim3(ceil_div(N, ROWS)), 0)
    return launched("mlp_fwd");
}

int exa_mlp_backward(const exa_mlp_net* net, int32_t N, const float* x, const float* const* grad_out, float* grad_x,
                     float* grad_params, float* grad_ws, void* workspace, uint64_t workspace_bytes, void* stream) {
    Params P;
    if (int rc = setup(net, N, P)) return rc;
    if (N > 0 && !x) return fail(EXA_MLP_E_NULLPTR, "x is NULL");
    if (!grad_out) return fail(EXA_MLP_E_NULLPTR, "grad_out is NULL");
    const uint64_t need = ws_bytes(net, P.nh, N);
    if (need > 0 && !workspace) return fail(EXA_MLP_E_NULLPTR, "workspace is NULL");
    if (workspace_bytes < need) return fail(EXA_MLP_E_INVALID, "workspace is smaller than exa_mlp_workspace_size");
    for (int i = 0; i < net->n_heads; ++i) P.gout[i] = grad_out[i];
    P.x = x;
    P.gx = grad_x;
    P.gparams = grad_params;
    P.gws = net->shared_width > 0 ? grad_ws : nullptr;
    float* ws = (float*)workspace;
    const uint64_t per = (uint64_t)net->n_layers * (uint64_t)N;
    P.xhat = ws;
    P.dy = ws + per * H;
    P.stat = ws + 2 * per * H;
    P.part = ws + per * (2 * H + STAT);
    hipStream_t st = (hipStream_t)stream;
    const bool params = grad_params || P.gws;
    if (N > 0 && (grad_x || params)) {
        EXA_MLP_DISPATCH(mlp_bwd_rows, dim3(ceil_div(N, ROWS)), 0)
        if (int rc = launched("mlp_bwd_rows")) return rc;
        if (params) {
            const dim3 g2((unsigned)P.nchunks, (unsigned)(net->n_layers + 1));
            EXA_MLP_DISPATCH(mlp_bwd_chunk, g2, 0)
            if (int rc = launched("mlp_bwd_chunk")) return rc;
        }
    }
    if (params) {
        const int64_t tot = P.P + (int64_t)H * net->shared_width;
        hipLaunchKernelGGL(mlp_bwd_sum, dim3(ceil_div(tot, BLOCK)), dim3(BLOCK), 0, st, P);
        if (int rc = launched("mlp_bwd_sum")) return rc;
    }
    return 0;
}

}  // extern "C"
