// LPIPS (VGG-16) perceptual distance, forward and input gradient (include/exa_raster.h, exa_lpips_*): reference
// avatar/common/nets/loss.py:77-95.  The operations and the order of every sum are written out in the header; this file
// is compiled with -ffp-contract=off, every fused multiply-add below is an explicit fmaf or an MFMA.
//
// Activations are channel-innermost, [image][row][column][channel].
//   lpips_prep        crop + input map, one thread per crop pixel.
//   lpips_conv1       the Cin = 3 convolution on the VALU (0.6 % of the MACs): one thread per pixel and 4 output channels.
//   lpips_conv<MODE>  every other 3x3 convolution, and every input gradient but the first layer's, as an implicit GEMM on
//                     v_mfma_f32_32x32x2_f32.  A workgroup of 4 waves owns a CONV_TILE x CONV_TILE = 16 x 16 pixel tile and
//                     64 output channels; a wave owns 4 rows of the tile (two 32-pixel MFMA tiles of 2 rows x 16 columns)
//                     and both 32-channel tiles: four accumulators.  The weights are the A operand (row = output channel),
//                     the pixels the B operand (column = pixel), so a lane ends with 4 x 4 consecutive channels of its
//                     pixel and stores them 16 bytes at a time.  Per chunk of CONV_KC = 16 input channels the 18 x 18
//                     halo and the 9 x 16 x 64 weights are staged in LDS (25.3 + 36 KiB); the 2 x 2 max-pool in front of
//                     a block is taken while the halo is staged.  K order: per chunk a chain over tap (row-major), then channel,
//                     from 0; the chunks' sums are added in ascending order.
//                     MODE FWD adds the bias and applies the ReLU; BWD_PLAIN multiplies by the ReLU mask of the saved
//                     activation; BWD_POOL routes through the pool, adds the head's gradient and multiplies by the mask.
//   lpips_conv1_bwd   the first layer's input gradient through the input map, written to the WHOLE image: zeros outside
//                     the crop come from this kernel.
//   lpips_normalize / lpips_head_fwd / lpips_head_reduce / lpips_head_bwd   the head, one thread per tap pixel.
#include "common.h"
#include "fixed_sum.h"
#include "image_checks.h"

namespace exa {

namespace {

constexpr int CONV_TILE = 16;
constexpr int CONV_KC = 16;
constexpr int HALO = CONV_TILE + 2;
constexpr int HALO_STRIDE = 20;           // floats per halo pixel: 16 channels + 4 of padding (conflict-free 16-byte reads)
constexpr int W_CHUNK = 9 * 2 * 64 * 8;   // floats of one (64 output channels, 16 input channels) weight image
constexpr float LPIPS_EPS = 1e-10f;

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int L_CIN[13] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int L_COUT[13] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int L_BLOCK[13] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};
constexpr int L_POOL[13] = {0, 0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0};      // a 2 x 2 max-pool in front of the layer
constexpr int TAP_LAYER[5] = {1, 3, 6, 9, 12};

struct Layout {
    int h[5], w[5];
    uint64_t act[13];          // float offsets of the 13 activations
    uint64_t x, g0, g1;        // the mapped input [B, h, w, 3] and the two gradient buffers
    uint64_t floats;
};

Layout make_layout(int B, int h, int w) {
    Layout L = {};
    for (int b = 0; b < 5; ++b) { L.h[b] = h >> b; L.w[b] = w >> b; }
    uint64_t o = 0;
    auto take = [&o](uint64_t n) { const uint64_t at = o; o += (n + 63) & ~uint64_t(63); return at; };      // 256-byte sections
    for (int l = 0; l < 13; ++l) L.act[l] = take((uint64_t)B * L.h[L_BLOCK[l]] * L.w[L_BLOCK[l]] * L_COUT[l]);
    L.x = take((uint64_t)B * h * w * 3);
    L.g0 = take((uint64_t)B * h * w * 64);
    L.g1 = take((uint64_t)B * h * w * 64);
    L.floats = o;
    return L;
}

__global__ __launch_bounds__(BLOCK) void lpips_prep(int B, int H, int W, int cx0, int cy0, int cw, int ch,
                                                    float sh0, float sh1, float sh2, float sc0, float sc1, float sc2,
                                                    const float* img, float* x) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (size_t)B * ch * cw) return;
    const int px = (int)(i % cw), py = (int)((i / cw) % ch), b = (int)(i / ((size_t)cw * ch));
    const size_t plane = (size_t)H * W, at = (size_t)(cy0 + py) * W + cx0 + px;
    const float shift[3] = {sh0, sh1, sh2}, scale[3] = {sc0, sc1, sc2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = img[((size_t)b * 3 + c) * plane + at] * 2.0f - 1.0f;
        x[i * 3 + c] = (v - shift[c]) / scale[c];
    }
}

// w1: [tap][ci][co] (27 x 64).  Thread i: pixel i / 16, output channels 4 (i % 16) .. + 3.  Per output: s = 0; taps
// row-major, channels ascending, s = fmaf(x, w, s) (a tap outside the crop is skipped: its x is the zero padding);
// then s + bias, ReLU.
__global__ __launch_bounds__(BLOCK) void lpips_conv1(int B, int h, int w, const float* x, const float* w1, const float* bias,
                                                     float* out) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (size_t)B * h * w * 16) return;
    const int q = (int)(i & 15);
    const size_t p = i >> 4;
    const int px = (int)(p % w), py = (int)((p / w) % h);
    const size_t img0 = (p / ((size_t)w * h)) * (size_t)h * w;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
            const int y = py + ky - 1, xx = px + kx - 1;
            if (y < 0 || y >= h || xx < 0 || xx >= w) continue;
            const float* xp = x + (img0 + (size_t)y * w + xx) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 wv = *reinterpret_cast<const float4*>(w1 + ((ky * 3 + kx) * 3 + c) * 64 + 4 * q);
                const float xv = xp[c];
                s[0] = fmaf(xv, wv.x, s[0]); s[1] = fmaf(xv, wv.y, s[1]);
                s[2] = fmaf(xv, wv.z, s[2]); s[3] = fmaf(xv, wv.w, s[3]);
            }
        }
    const float4 bv = *reinterpret_cast<const float4*>(bias + 4 * q);
    float4 o;
    o.x = fmaxf(s[0] + bv.x, 0.f); o.y = fmaxf(s[1] + bv.y, 0.f);
    o.z = fmaxf(s[2] + bv.z, 0.f); o.w = fmaxf(s[3] + bv.w, 0.f);
    *reinterpret_cast<float4*>(out + p * 64 + 4 * q) = o;
}

enum { FWD = 0, BWD_PLAIN = 1, BWD_POOL = 2 };

struct ConvArgs {
    const float* in;      // [B, Hs, Ws, Cin]
    int Hs, Ws, pool;     // the source array; pool: the convolution's input is its 2 x 2 max-pool
    int h, w, Cin, Cout;  // the convolution's resolution (h = Hs >> pool) and channels; Cin % 16 == 0, Cout % 64 == 0
    const float* wpk;     // [Cout / 64][Cin / 16][W_CHUNK]
    const float* bias;    // FWD
    float* out;           // FWD, BWD_PLAIN: [B, h, w, Cout]; BWD_POOL: [B, Ha, Wa, Cout]
    const float* act;     // BWD_*: the saved activation the output is the gradient of ([B, h, w, Cout] / [B, Ha, Wa, Cout])
    const float* hg;      // BWD_POOL: the head's gradient at that activation
    int Ha, Wa;           // BWD_POOL: h = Ha / 2, w = Wa / 2
    int tiles_x;
};

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 max4(float4 a, float4 b) {
    return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}
__device__ __forceinline__ float masked(float a, float g) { return a > 0.f ? g : 0.f; }
__device__ __forceinline__ float4 masked4(float4 a, float4 g) {
    return make_float4(masked(a.x, g.x), masked(a.y, g.y), masked(a.z, g.z), masked(a.w, g.w));
}

// BWD_POOL, one channel: the pooled pixel's gradient g goes to the first maximum (row-major) of a[0..3]
__device__ __forceinline__ int first_max(float a0, float a1, float a2, float a3) {
    int k = 0; float m = a0;
    if (a1 > m) { m = a1; k = 1; }
    if (a2 > m) { m = a2; k = 2; }
    if (a3 > m) { k = 3; }
    return k;
}

template <int MODE>
__global__ __launch_bounds__(BLOCK) void lpips_conv(ConvArgs a) {
    __shared__ __attribute__((aligned(16))) float s_in[HALO * HALO * HALO_STRIDE];
    __shared__ __attribute__((aligned(16))) float s_w[W_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, j = lane & 31, hh = lane >> 5;
    const int ty0 = (blockIdx.x / a.tiles_x) * CONV_TILE, tx0 = (blockIdx.x % a.tiles_x) * CONV_TILE;
    const int ct = blockIdx.y, b = blockIdx.z;
    const int nchunks = a.Cin / CONV_KC;
    const float* in = a.in + (size_t)b * a.Hs * a.Ws * a.Cin;
    // tot: the sum over the chunks so far; acc: the current chunk's 144-term chain, started at 0 (a K-term chain in one
    // accumulator would carry the rounding error of K = 4608 additions at the deep layers)
    f32x16 tot[2][2], acc[2][2];
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
        for (int pt = 0; pt < 2; ++pt)
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[c2][pt][r] = 0.f;

    for (int ck = 0; ck < nchunks; ++ck) {
        __syncthreads();
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
            for (int pt = 0; pt < 2; ++pt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[c2][pt][r] = 0.f;
        for (int idx = tid; idx < HALO * HALO * 4; idx += BLOCK) {
            const int pix = idx >> 2, q = idx & 3;
            const int y = ty0 + pix / HALO - 1, x = tx0 + pix % HALO - 1;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (y >= 0 && y < a.h && x >= 0 && x < a.w) {
                const int c = ck * CONV_KC + 4 * q;
                if (a.pool) {
                    const float* p = in + ((size_t)(2 * y) * a.Ws + 2 * x) * a.Cin + c;
                    v = max4(max4(ld4(p), ld4(p + a.Cin)), max4(ld4(p + (size_t)a.Ws * a.Cin), ld4(p + ((size_t)a.Ws + 1) * a.Cin)));
                } else {
                    v = ld4(in + ((size_t)y * a.Ws + x) * a.Cin + c);
                }
            }
            // channel c of an 8-group sits at (c & 1) * 4 + (c >> 1): lane half hh reads channels hh, 2 + hh, 4 + hh, 6 + hh at once
            float* d = s_in + pix * HALO_STRIDE + (q >> 1) * 8 + 2 * (q & 1);
            *reinterpret_cast<float2*>(d) = make_float2(v.x, v.z);
            *reinterpret_cast<float2*>(d + 4) = make_float2(v.y, v.w);
        }
        const float* wsrc = a.wpk + ((size_t)ct * nchunks + ck) * W_CHUNK;
        for (int idx = tid; idx < W_CHUNK / 4; idx += BLOCK) st4(s_w + 4 * idx, ld4(wsrc + 4 * idx));
        __syncthreads();
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap % 3;
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                float4 bv[2], av[2];
#pragma unroll
                for (int pt = 0; pt < 2; ++pt) {
                    const int row = 4 * wv + 2 * pt + (j >> 4), col = j & 15;
                    bv[pt] = ld4(s_in + ((row + ky) * HALO + col + kx) * HALO_STRIDE + g * 8 + 4 * hh);
                }
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2) av[c2] = ld4(s_w + ((tap * 2 + g) * 64 + c2 * 32 + j) * 8 + 4 * hh);
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
                    for (int pt = 0; pt < 2; ++pt) {
                        acc[c2][pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c2].x, bv[pt].x, acc[c2][pt], 0, 0, 0);
                        acc[c2][pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c2].y, bv[pt].y, acc[c2][pt], 0, 0, 0);
                        acc[c2][pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c2].z, bv[pt].z, acc[c2][pt], 0, 0, 0);
                        acc[c2][pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c2].w, bv[pt].w, acc[c2][pt], 0, 0, 0);
                    }
            }
        }
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) tot[c2][pt] = tot[c2][pt] + acc[c2][pt];
    }

#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
        const int y = ty0 + 4 * wv + 2 * pt + (j >> 4), x = tx0 + (j & 15);
        if (y >= a.h || x >= a.w) continue;
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const int co = ct * 64 + c2 * 32 + 8 * gq + 4 * hh;      // accumulator registers 4 gq .. 4 gq + 3
                const float4 s = make_float4(tot[c2][pt][4 * gq], tot[c2][pt][4 * gq + 1], tot[c2][pt][4 * gq + 2],
                                             tot[c2][pt][4 * gq + 3]);
                if (MODE == FWD) {
                    const float4 bi = ld4(a.bias + co);
                    st4(a.out + (((size_t)b * a.h + y) * a.w + x) * a.Cout + co,
                        make_float4(fmaxf(s.x + bi.x, 0.f), fmaxf(s.y + bi.y, 0.f), fmaxf(s.z + bi.z, 0.f), fmaxf(s.w + bi.w, 0.f)));
                } else if (MODE == BWD_PLAIN) {
                    const size_t o = (((size_t)b * a.h + y) * a.w + x) * a.Cout + co;
                    st4(a.out + o, masked4(ld4(a.act + o), s));
                } else {
                    // the 2 x 2 window of the pooled pixel, and the row / column an odd size drops (their pool gradient is 0)
                    const int ny = (y == a.h - 1 && (a.Ha & 1)) ? 3 : 2, nx = (x == a.w - 1 && (a.Wa & 1)) ? 3 : 2;
                    size_t o[3][3];
                    float4 av4[3][3];
                    for (int dy = 0; dy < ny; ++dy)
                        for (int dx = 0; dx < nx; ++dx) {
                            o[dy][dx] = (((size_t)b * a.Ha + 2 * y + dy) * a.Wa + 2 * x + dx) * a.Cout + co;
                            av4[dy][dx] = ld4(a.act + o[dy][dx]);
                        }
                    const int k0 = first_max(av4[0][0].x, av4[0][1].x, av4[1][0].x, av4[1][1].x);
                    const int k1 = first_max(av4[0][0].y, av4[0][1].y, av4[1][0].y, av4[1][1].y);
                    const int k2 = first_max(av4[0][0].z, av4[0][1].z, av4[1][0].z, av4[1][1].z);
                    const int k3 = first_max(av4[0][0].w, av4[0][1].w, av4[1][0].w, av4[1][1].w);
                    for (int dy = 0; dy < ny; ++dy)
                        for (int dx = 0; dx < nx; ++dx) {
                            const int k = (dy < 2 && dx < 2) ? 2 * dy + dx : -1;
                            const float4 hg = ld4(a.hg + o[dy][dx]);
                            const float4 g = make_float4((k == k0 ? s.x : 0.f) + hg.x, (k == k1 ? s.y : 0.f) + hg.y,
                                                         (k == k2 ? s.z : 0.f) + hg.z, (k == k3 ? s.w : 0.f) + hg.w);
                            st4(a.out + o[dy][dx], masked4(av4[dy][dx], g));
                        }
                }
            }
    }
}

// dZ1: [B, h, w, 64], the gradient at the first convolution's output before its ReLU mask is NOT meant: it is masked already.
// One thread per pixel of the WHOLE image.  Inside the crop, per input channel c: s = 0; taps row-major, output channels
// ascending: s = fmaf(dZ1[y - ky + 1][x - kx + 1][co], w1[tap][c][co], s); dimg = (s / scale_c) * 2.  Outside: 0.
__global__ __launch_bounds__(BLOCK) void lpips_conv1_bwd(int B, int H, int W, int cx0, int cy0, int cw, int ch,
                                                         float sc0, float sc1, float sc2, const float* dz, const float* w1,
                                                         float* dimg) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (size_t)B * H * W) return;
    const int X = (int)(i % W), Y = (int)((i / W) % H), b = (int)(i / ((size_t)W * H));
    const int px = X - cx0, py = Y - cy0;
    float s[3] = {0.f, 0.f, 0.f};
    if (px >= 0 && px < cw && py >= 0 && py < ch) {
        for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx) {
                const int y = py - ky + 1, x = px - kx + 1;
                if (y < 0 || y >= ch || x < 0 || x >= cw) continue;
                const float* g = dz + (((size_t)b * ch + y) * cw + x) * 64;
                const float* wt = w1 + (ky * 3 + kx) * 3 * 64;
                for (int co = 0; co < 64; co += 4) {
                    const float4 gv = ld4(g + co);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float4 wv4 = ld4(wt + c * 64 + co);
                        s[c] = fmaf(gv.x, wv4.x, s[c]); s[c] = fmaf(gv.y, wv4.y, s[c]);
                        s[c] = fmaf(gv.z, wv4.z, s[c]); s[c] = fmaf(gv.w, wv4.w, s[c]);
                    }
                }
            }
    }
    const float scale[3] = {sc0, sc1, sc2};
    const size_t plane = (size_t)H * W, at = (size_t)Y * W + X;
#pragma unroll
    for (int c = 0; c < 3; ++c) dimg[((size_t)b * 3 + c) * plane + at] = (s[c] / scale[c]) * 2.0f;
}

__global__ __launch_bounds__(BLOCK) void lpips_relu_mask(size_t n4, const float* act, const float* g, float* out) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n4) st4(out + 4 * i, masked4(ld4(act + 4 * i), ld4(g + 4 * i)));
}

// ---- the head.  Features [N, C] (N = images x pixels, channel-innermost), C % 4 == 0.

// sum_c f_c^2: four running sums over the channels c = k (mod 4), ascending, s_k = s_k + f * f; then (s_0 + s_1) + (s_2 + s_3)
__device__ __forceinline__ float sum_sq(const float* f, int C) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int c = 0; c < C; c += 4) {
        const float4 v = ld4(f + c);
        s0 = s0 + v.x * v.x; s1 = s1 + v.y * v.y; s2 = s2 + v.z * v.z; s3 = s3 + v.w * v.w;
    }
    return (s0 + s1) + (s2 + s3);
}

__global__ __launch_bounds__(BLOCK) void lpips_normalize(size_t N, int C, const float* f, float* out) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= N) return;
    const float* p = f + i * C;
    const float d = sqrtf(sum_sq(p, C)) + LPIPS_EPS;
    for (int c = 0; c < C; c += 4) {
        const float4 v = ld4(p + c);
        st4(out + i * C + c, make_float4(v.x / d, v.y / d, v.z / d, v.w / d));
    }
}

// grid (blocks per image, B): d = sum_c w_c * (fo_c / (|fo| + eps) - nt_c)^2 per pixel, in sum_sq's order
__global__ __launch_bounds__(BLOCK) void lpips_head_fwd(int npix, int C, const float* fo, const float* nt, const float* w,
                                                        float* dmap, float* partials) {
    const int i = blockIdx.x * BLOCK + threadIdx.x, b = blockIdx.y;
    float d = 0.f;
    if (i < npix) {
        const size_t at = ((size_t)b * npix + i) * C;
        const float den = sqrtf(sum_sq(fo + at, C)) + LPIPS_EPS;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        for (int c = 0; c < C; c += 4) {
            const float4 v = ld4(fo + at + c), t = ld4(nt + at + c), wc = ld4(w + c);
            const float e0 = v.x / den - t.x, e1 = v.y / den - t.y, e2 = v.z / den - t.z, e3 = v.w / den - t.w;
            s0 = s0 + wc.x * (e0 * e0); s1 = s1 + wc.y * (e1 * e1); s2 = s2 + wc.z * (e2 * e2); s3 = s3 + wc.w * (e3 * e3);
        }
        d = (s0 + s1) + (s2 + s3);
        if (dmap) dmap[(size_t)b * npix + i] = d;
    }
    d = block_sum<BLOCK / 64>(d);
    if (threadIdx.x == 0) partials[(size_t)b * gridDim.x + blockIdx.x] = d;
}

struct ReduceArgs {
    int n_taps;
    const float* partials[EXA_LPIPS_MAX_TAPS];
    int nblk[EXA_LPIPS_MAX_TAPS];
    float npix[EXA_LPIPS_MAX_TAPS];
    float* out;
};

// grid B: per tap, thread t adds the image's partials t, t + 256, .. in that order, the workgroup sum, / npix; the taps
// are added in ascending order
__global__ __launch_bounds__(BLOCK) void lpips_head_reduce(ReduceArgs a) {
    const int b = blockIdx.x;
    float total = 0.f;
    for (int l = 0; l < a.n_taps; ++l) {
        float s = strided_sum<BLOCK>(a.partials[l] + (size_t)b * a.nblk[l], a.nblk[l]);
        __syncthreads();                                   // (block_sum's LDS is reused per tap)
        s = block_sum<BLOCK / 64>(s);
        const float D = s / a.npix[l];
        total = l == 0 ? D : total + D;
    }
    if (threadIdx.x == 0) a.out[b] = total;
}

// dL/dfo for one tap: gd = gout[b] * (1 / npix); u_c = (2 w_c (no_c - nt_c)) gd; dot = sum_c u_c fo_c (sum_sq's order);
// dfo_c = u_c / (r + eps) - fo_c * (dot / (r (r + eps)^2)), the second term 0 where r = 0
__global__ __launch_bounds__(BLOCK) void lpips_head_bwd(int npix, int C, const float* fo, const float* nt, const float* w,
                                                        const float* gout, float* dfo) {
    const int i = blockIdx.x * BLOCK + threadIdx.x, b = blockIdx.y;
    if (i >= npix) return;
    const size_t at = ((size_t)b * npix + i) * C;
    const float gd = gout[b] * (1.0f / (float)npix);
    const float r = sqrtf(sum_sq(fo + at, C)), den = r + LPIPS_EPS;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int c = 0; c < C; c += 4) {
        const float4 v = ld4(fo + at + c), t = ld4(nt + at + c), wc = ld4(w + c);
        s0 = s0 + ((2.0f * wc.x) * (v.x / den - t.x)) * gd * v.x;
        s1 = s1 + ((2.0f * wc.y) * (v.y / den - t.y)) * gd * v.y;
        s2 = s2 + ((2.0f * wc.z) * (v.z / den - t.z)) * gd * v.z;
        s3 = s3 + ((2.0f * wc.w) * (v.w / den - t.w)) * gd * v.w;
    }
    const float dot = (s0 + s1) + (s2 + s3);
    const float k = r > 0.f ? dot / (r * (den * den)) : 0.f;
    for (int c = 0; c < C; c += 4) {
        const float4 v = ld4(fo + at + c), t = ld4(nt + at + c), wc = ld4(w + c);
        float4 g;
        g.x = ((2.0f * wc.x) * (v.x / den - t.x)) * gd / den - v.x * k;
        g.y = ((2.0f * wc.y) * (v.y / den - t.y)) * gd / den - v.y * k;
        g.z = ((2.0f * wc.z) * (v.z / den - t.z)) * gd / den - v.z * k;
        g.w = ((2.0f * wc.w) * (v.w / den - t.w)) * gd / den - v.w * k;
        st4(dfo + at + c, g);
    }
}

unsigned blocks_of(uint64_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

}  // namespace

}  // namespace exa

// ---- C entry points (include/exa_raster.h): checks, then the launches ------------------------------------------------------
namespace exa_raster_impl {

using namespace exa;

EXA_ABI_STATUS_SHARED("exa_raster")       // exa_raster_last_error() and its buffer are api.hip's

#define LP_CHECK(where)                              \
    do {                                             \
        if (int rc_ = launched(where)) return rc_;   \
    } while (0)

static int64_t head_blocks(int64_t npix) { return (npix + BLOCK - 1) / BLOCK; }

// B images, a crop of h x w: the sizes the LPIPS kernels index with 32 bits
static int check_lpips_sizes(int32_t B, int32_t h, int32_t w) {
    if (B < 0 || h < 0 || w < 0) return fail(EXA_RASTER_E_INVALID, "negative size");
    if (B > 0 && (h < EXA_LPIPS_MIN_CROP || w < EXA_LPIPS_MIN_CROP))
        return fail(EXA_RASTER_E_INVALID, "lpips: the crop is smaller than 16 x 16 (the fifth tap would be empty)");
    if (B > 65535 || (int64_t)B * h * w > 0x7fffffffLL / 16)
        return fail(EXA_RASTER_E_INVALID, "lpips: more than 65535 images or 2^27 - 1 crop pixels");
    return 0;
}

static int check_lpips_trunk(int32_t B, int32_t H, int32_t W, const int32_t* crop, uint64_t ws_bytes) {
    int rc = check_crop(B, 3, H, W, crop);
    if (rc) return rc;
    if ((int64_t)B * H * W > 0x7fffffffLL) return fail(EXA_RASTER_E_INVALID, "lpips: more than 2^31 - 1 image pixels");
    if ((rc = check_lpips_sizes(B, crop[3], crop[2]))) return rc;
    if (ws_bytes < make_layout(B, crop[3], crop[2]).floats * sizeof(float))
        return fail(EXA_RASTER_E_INVALID, "lpips: the workspace is smaller than exa_lpips_workspace_size()");
    return 0;
}

// the head's arrays: B images of npix pixels and C channels, indexed with 32 bits per image
static int check_lpips_head(int32_t B, int64_t npix, int32_t C) {
    if (B < 0 || npix < 0 || C < 0) return fail(EXA_RASTER_E_INVALID, "negative size");
    if (C % 4 != 0 || C == 0) return fail(EXA_RASTER_E_INVALID, "lpips head: C must be a positive multiple of 4");
    if (B > 65535 || npix > 0x7fffffffLL - 256)
        return fail(EXA_RASTER_E_INVALID, "lpips head: more than 65535 images or 2^31 - 257 pixels per image");
    return 0;
}

}  // namespace exa_raster_impl

using namespace exa_raster_impl;

extern "C" {

int exa_lpips_workspace_size(int32_t B, int32_t h, int32_t w, uint64_t* bytes) {
    if (!bytes) return fail(EXA_RASTER_E_NULLPTR, "lpips: bytes is NULL");
    if (int rc = check_lpips_sizes(B, h, w)) return rc;
    *bytes = make_layout(B, h, w).floats * sizeof(float);
    return 0;
}

int exa_lpips_tap_layout(int32_t B, int32_t h, int32_t w, int32_t tap, uint64_t* byte_offset, int32_t* shape) {
    if (!byte_offset || !shape) return fail(EXA_RASTER_E_NULLPTR, "lpips: NULL argument");
    if (tap < 0 || tap >= EXA_LPIPS_TAPS) return fail(EXA_RASTER_E_INVALID, "lpips: tap must be 0 .. 4");
    if (int rc = check_lpips_sizes(B, h, w)) return rc;
    *byte_offset = make_layout(B, h, w).act[TAP_LAYER[tap]] * sizeof(float);
    shape[0] = h >> tap; shape[1] = w >> tap; shape[2] = L_COUT[TAP_LAYER[tap]];
    return 0;
}

int exa_lpips_trunk_forward(int32_t B, int32_t H, int32_t W, const int32_t* crop, const float* img,
                            const float* shift_scale, const float* const* weights, const float* const* biases, void* ws_,
                            uint64_t ws_bytes, void* stream) {
    if (int rc = check_lpips_trunk(B, H, W, crop, ws_bytes)) return rc;
    if (B == 0) return 0;
    if (!img || !shift_scale || !weights || !biases || !ws_) return fail(EXA_RASTER_E_NULLPTR, "lpips: NULL argument");
    for (int l = 0; l < EXA_LPIPS_LAYERS; ++l)
        if (!weights[l] || !biases[l]) return fail(EXA_RASTER_E_NULLPTR, "lpips: NULL weight or bias");
    for (int c = 3; c < 6; ++c)
        if (!(shift_scale[c] != 0.0f)) return fail(EXA_RASTER_E_INVALID, "lpips: a scale of the input map is 0 or NaN");
    float* const ws = static_cast<float*>(ws_);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int cw = crop[2], ch = crop[3];
    const Layout L = make_layout(B, ch, cw);
    lpips_prep<<<blocks_of((uint64_t)B * ch * cw), BLOCK, 0, s>>>(B, H, W, crop[0], crop[1], cw, ch, shift_scale[0],
                                                                  shift_scale[1], shift_scale[2], shift_scale[3],
                                                                  shift_scale[4], shift_scale[5], img, ws + L.x);
    LP_CHECK("lpips_trunk_fwd");
    lpips_conv1<<<blocks_of((uint64_t)B * ch * cw * 16), BLOCK, 0, s>>>(B, ch, cw, ws + L.x, weights[0], biases[0],
                                                                        ws + L.act[0]);
    LP_CHECK("lpips_trunk_fwd");
    for (int l = 1; l < 13; ++l) {
        const int blk = L_BLOCK[l], src = L_BLOCK[l - 1];
        ConvArgs a = {};
        a.in = ws + L.act[l - 1]; a.Hs = L.h[src]; a.Ws = L.w[src]; a.pool = L_POOL[l];
        a.h = L.h[blk]; a.w = L.w[blk]; a.Cin = L_CIN[l]; a.Cout = L_COUT[l];
        a.wpk = weights[l]; a.bias = biases[l]; a.out = ws + L.act[l];
        a.tiles_x = (a.w + CONV_TILE - 1) / CONV_TILE;
        const dim3 grid(a.tiles_x * ((a.h + CONV_TILE - 1) / CONV_TILE), a.Cout / 64, B);
        lpips_conv<FWD><<<grid, BLOCK, 0, s>>>(a);
        LP_CHECK("lpips_trunk_fwd");
    }
    return 0;
}

// head_grads[t]: dL/d(tap t) [B, h_t, w_t, C_t] without the ReLU mask; weights_t[l]: the transposed, rotated weights of
// layer l (l = 1 .. 12) in the convolution's image; weights_t[0]: the first layer's [tap][ci][co]
int exa_lpips_trunk_backward(int32_t B, int32_t H, int32_t W, const int32_t* crop, const float* shift_scale,
                             const float* const* weights_t, const float* const* head_grads, void* ws_, uint64_t ws_bytes,
                             float* dL_dimg, void* stream) {
    if (int rc = check_lpips_trunk(B, H, W, crop, ws_bytes)) return rc;
    if (B == 0) return 0;
    if (!shift_scale || !weights_t || !head_grads || !ws_ || !dL_dimg) return fail(EXA_RASTER_E_NULLPTR, "lpips: NULL argument");
    for (int l = 0; l < EXA_LPIPS_LAYERS; ++l)
        if (!weights_t[l]) return fail(EXA_RASTER_E_NULLPTR, "lpips: NULL weight or bias");
    for (int t = 0; t < EXA_LPIPS_TAPS; ++t)
        if (!head_grads[t]) return fail(EXA_RASTER_E_NULLPTR, "lpips: NULL head gradient");
    for (int c = 3; c < 6; ++c)
        if (!(shift_scale[c] != 0.0f)) return fail(EXA_RASTER_E_INVALID, "lpips: a scale of the input map is 0 or NaN");
    float* const ws = static_cast<float*>(ws_);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int cw = crop[2], ch = crop[3];
    const Layout L = make_layout(B, ch, cw);
    float* g[2] = {ws + L.g0, ws + L.g1};
    int cur = 0;
    {
        const uint64_t n = (uint64_t)B * L.h[4] * L.w[4] * 512;
        lpips_relu_mask<<<blocks_of(n / 4), BLOCK, 0, s>>>((size_t)(n / 4), ws + L.act[12], head_grads[4], g[cur]);
        LP_CHECK("lpips_trunk_bwd");
    }
    for (int l = 12; l >= 1; --l) {      // dZ_l -> dZ_{l-1}
        const int blk = L_BLOCK[l], prev = L_BLOCK[l - 1];
        ConvArgs a = {};
        a.in = g[cur]; a.Hs = L.h[blk]; a.Ws = L.w[blk]; a.pool = 0;
        a.h = L.h[blk]; a.w = L.w[blk]; a.Cin = L_COUT[l]; a.Cout = L_CIN[l];
        a.wpk = weights_t[l]; a.out = g[cur ^ 1]; a.act = ws + L.act[l - 1];
        a.tiles_x = (a.w + CONV_TILE - 1) / CONV_TILE;
        const dim3 grid(a.tiles_x * ((a.h + CONV_TILE - 1) / CONV_TILE), a.Cout / 64, B);
        if (L_POOL[l]) {
            a.Ha = L.h[prev]; a.Wa = L.w[prev]; a.hg = head_grads[prev];
            lpips_conv<BWD_POOL><<<grid, BLOCK, 0, s>>>(a);
        } else {
            lpips_conv<BWD_PLAIN><<<grid, BLOCK, 0, s>>>(a);
        }
        LP_CHECK("lpips_trunk_bwd");
        cur ^= 1;
    }
    lpips_conv1_bwd<<<blocks_of((uint64_t)B * H * W), BLOCK, 0, s>>>(B, H, W, crop[0], crop[1], cw, ch, shift_scale[3],
                                                                    shift_scale[4], shift_scale[5], g[cur], weights_t[0],
                                                                    dL_dimg);
    return launched("lpips_trunk_bwd");
}

int exa_lpips_normalize(int64_t N, int32_t C, const float* f, float* out, void* stream) {
    if (N < 0 || C < 0) return fail(EXA_RASTER_E_INVALID, "negative size");
    if (C % 4 != 0 || C == 0) return fail(EXA_RASTER_E_INVALID, "lpips head: C must be a positive multiple of 4");
    if (N > 0x7fffffffLL * 256) return fail(EXA_RASTER_E_INVALID, "lpips head: more than 2^39 pixels");
    if (N > 0 && (!f || !out)) return fail(EXA_RASTER_E_NULLPTR, "lpips head: NULL argument");
    if (N == 0) return 0;
    lpips_normalize<<<blocks_of((uint64_t)N), BLOCK, 0, static_cast<hipStream_t>(stream)>>>((size_t)N, C, f, out);
    return launched("lpips_normalize");
}

int64_t exa_lpips_head_blocks(int64_t npix) { return npix <= 0 ? 0 : head_blocks(npix); }

int exa_lpips_head_forward(int32_t B, int64_t npix, int32_t C, const float* f_out, const float* n_target, const float* lin,
                           float* d_map, float* partials, void* stream) {
    if (int rc = check_lpips_head(B, npix, C)) return rc;
    if ((int64_t)B * npix > 0 && (!f_out || !n_target || !lin || !partials))
        return fail(EXA_RASTER_E_NULLPTR, "lpips head: NULL argument");
    if (B == 0 || npix == 0) return 0;
    lpips_head_fwd<<<dim3((unsigned)head_blocks(npix), B), BLOCK, 0, static_cast<hipStream_t>(stream)>>>(
        (int)npix, C, f_out, n_target, lin, d_map, partials);
    return launched("lpips_head_fwd");
}

int exa_lpips_head_reduce(int32_t B, int32_t n_taps, const float* const* partials, const int64_t* npix, float* out,
                          void* stream) {
    if (B < 0 || B > 65535) return fail(EXA_RASTER_E_INVALID, "lpips head: B must be 0 .. 65535");
    if (n_taps < 1 || n_taps > EXA_LPIPS_MAX_TAPS) return fail(EXA_RASTER_E_INVALID, "lpips head: n_taps must be 1 .. 8");
    if (!partials || !npix || (B > 0 && !out)) return fail(EXA_RASTER_E_NULLPTR, "lpips head: NULL argument");
    for (int l = 0; l < n_taps; ++l) {
        if (npix[l] <= 0 || npix[l] > 0x7fffffffLL - 256) return fail(EXA_RASTER_E_INVALID, "lpips head: a tap without pixels");
        if (B > 0 && !partials[l]) return fail(EXA_RASTER_E_NULLPTR, "lpips head: NULL argument");
    }
    if (B == 0) return 0;
    ReduceArgs a = {};
    a.n_taps = n_taps; a.out = out;
    for (int l = 0; l < n_taps; ++l) {
        a.partials[l] = partials[l]; a.nblk[l] = (int)head_blocks(npix[l]); a.npix[l] = (float)npix[l];
    }
    lpips_head_reduce<<<B, BLOCK, 0, static_cast<hipStream_t>(stream)>>>(a);
    return launched("lpips_head_reduce");
}

int exa_lpips_head_backward(int32_t B, int64_t npix, int32_t C, const float* f_out, const float* n_target, const float* lin,
                            const float* dL_dout, float* dL_df, void* stream) {
    if (int rc = check_lpips_head(B, npix, C)) return rc;
    if ((int64_t)B * npix > 0 && (!f_out || !n_target || !lin || !dL_dout || !dL_df))
        return fail(EXA_RASTER_E_NULLPTR, "lpips head: NULL argument");
    if (B == 0 || npix == 0) return 0;
    lpips_head_bwd<<<dim3((unsigned)head_blocks(npix), B), BLOCK, 0, static_cast<hipStream_t>(stream)>>>(
        (int)npix, C, f_out, n_target, lin, dL_dout, dL_df);
    return launched("lpips_head_bwd");
}

}  // extern "C"
