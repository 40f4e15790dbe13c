// Triplane feature lookup (include/exa_triplane.h): the bilinear F.grid_sample of ExAvatar's extract_tri_feature
// (reference module.py:424-457) over a body and a face plane set, and its atomic-free backward.  The semantics -- the
// op-by-op fp32 forward and the backward's two-level summation order -- are written out in the header; this file
// implements them.
//
//   triplane_plan_keys  one thread per (row, plane): the texel keys of the plane's four taps (the plan's step 1).
//   triplane_fwd        one thread per (row, plane, group of CPT channels), consecutive threads over the channels of a
//                       row, so a wave's output is contiguous 4 * 3C-byte rows.  Both sets in one launch: the row's
//                       selector picks the set.
//   triplane_bwd        one workgroup per run of consecutive texels (the plan's step 4), both sets and all three
//                       planes in one launch.  Pass 1: each thread takes a (segment, group of CPT channels) pair, walks
//                       the segment's entries in order, reads the g row coalesced across channels, recomputes the tap
//                       weight from the coordinates and leaves the partial in LDS.  Pass 2: each thread takes a
//                       (texel, channel) pair, consecutive threads over consecutive texels of one channel, sums the
//                       texel's partials in segment order and stores the gradient element.  Every element is written
//                       by exactly one thread: no atomics, no memsets.
//
// All three use the same device functions (unnormalize / tap_weight / tap_texel) for a row's taps.
// Compiled with -ffp-contract=off (build.py): the products must not be contracted into fused multiply-adds.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/exa_triplane.h"
#include "abi_status.h"

namespace exa_triplane_impl {

using exa::ceil_div;

constexpr int FWD_BLOCK = 256;
constexpr int BWD_BLOCK = 1024;
constexpr int KEY_BLOCK = 256;

// A row's sampling position on one plane: the unnormalised source coordinate and its floor.
struct Pos {
    float ix, iy, x0, y0;
};

__device__ __forceinline__ void plane_uv(float gx, float gy, float gz, int k, float& u, float& v) {
    u = k == 2 ? gy : gx;
    v = k == 0 ? gy : gz;
}

// align_corners=False: ix = ((u + 1) * W - 1) / 2, every operation rounded in fp32
__device__ __forceinline__ Pos unnormalize(float u, float v, int H, int W) {
    Pos p;
    p.ix = ((u + 1.0f) * (float)W - 1.0f) / 2.0f;
    p.iy = ((v + 1.0f) * (float)H - 1.0f) / 2.0f;
    p.x0 = floorf(p.ix);
    p.y0 = floorf(p.iy);
    return p;
}

// weight of tap t (0 = (x0, y0), 1 = (x1, y0), 2 = (x0, y1), 3 = (x1, y1)): nw, ne, sw, se of the header
__device__ __forceinline__ float tap_weight(const Pos& p, int t) {
    const float wx = (t & 1) ? p.ix - p.x0 : (p.x0 + 1.0f) - p.ix;
    const float wy = (t & 2) ? p.iy - p.y0 : (p.y0 + 1.0f) - p.iy;
    return wx * wy;
}

// texel offset y * W + x of tap t, or -1 when it lies outside [0, W) x [0, H) (compared in float: no conversion of an
// out-of-range value to int)
__device__ __forceinline__ int tap_texel(const Pos& p, int t, int H, int W) {
    const float x = (t & 1) ? p.x0 + 1.0f : p.x0;
    const float y = (t & 2) ? p.y0 + 1.0f : p.y0;
    if (!(x >= 0.0f && x < (float)W && y >= 0.0f && y < (float)H)) return -1;
    return (int)y * W + (int)x;
}

struct KeyParams {
    int32_t N, H, W;
    const float* coords;
    const uint8_t* is_face;
    int32_t* keys;
};

__global__ __launch_bounds__(KEY_BLOCK) void triplane_plan_keys(KeyParams P) {
    const int64_t q = (int64_t)blockIdx.x * KEY_BLOCK + threadIdx.x;      // (row, plane)
    if (q >= (int64_t)P.N * 3) return;
    const int i = (int)(q / 3), k = (int)(q - (int64_t)i * 3);
    const float* g = P.coords + (int64_t)i * 3;
    float u, v;
    plane_uv(g[0], g[1], g[2], k, u, v);
    const Pos p = unnormalize(u, v, P.H, P.W);
    const int HW = P.H * P.W;
    const int T = 6 * HW;
    const int base = (P.is_face[i] ? 3 * HW : 0) + k * HW;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int yx = tap_texel(p, t, P.H, P.W);
        P.keys[q * 4 + t] = yx < 0 ? T : base + yx;
    }
}

struct FwdParams {
    int32_t N, C, H, W;
    const float* body;
    const float* face;
    const float* coords;
    const uint8_t* is_face;
    float* out;
};

template <int CPT>
__global__ __launch_bounds__(FWD_BLOCK) void triplane_fwd(FwdParams P) {
    const int G = P.C / CPT;
    const int64_t q = (int64_t)blockIdx.x * FWD_BLOCK + threadIdx.x;      // (row, plane, channel group)
    if (q >= (int64_t)P.N * 3 * G) return;
    const int i = (int)(q / (3 * G));
    const int r = (int)(q - (int64_t)i * 3 * G);
    const int k = r / G, cg = r - k * G;
    const float* g = P.coords + (int64_t)i * 3;
    float u, v;
    plane_uv(g[0], g[1], g[2], k, u, v);
    const Pos p = unnormalize(u, v, P.H, P.W);
    const int64_t HW = (int64_t)P.H * P.W;
    const float* pl = (P.is_face[i] ? P.face : P.body) + ((int64_t)k * P.C + cg * CPT) * HW;
    int yx[4];
    float w[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        yx[t] = tap_texel(p, t, P.H, P.W);
        w[t] = tap_weight(p, t);
    }
    float acc[CPT];
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
        float a = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (yx[t] >= 0) a = a + pl[c * HW + yx[t]] * w[t];
        acc[c] = a;
    }
    float* o = P.out + (int64_t)i * 3 * P.C + k * P.C + cg * CPT;
    if constexpr (CPT == 4) {
        *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
#pragma unroll
        for (int c = 0; c < CPT; ++c) o[c] = acc[c];
    }
}

struct BwdParams {
    int32_t N, C, H, W, max_segs;
    const float* coords;
    const float* gout;
    const int32_t* entries;
    const int32_t* seg_entry;
    const int32_t* tex_seg;
    const int32_t* wg_tex;
    float* gbody;
    float* gface;
};

template <int CPT>
__device__ __forceinline__ void load_g(const float* src, float (&gv)[CPT]) {
    if constexpr (CPT == 4) {
        const float4 x = *reinterpret_cast<const float4*>(src);
        gv[0] = x.x; gv[1] = x.y; gv[2] = x.z; gv[3] = x.w;
    } else {
#pragma unroll
        for (int c = 0; c < CPT; ++c) gv[c] = src[c];
    }
}

template <int CPT>
__global__ __launch_bounds__(BWD_BLOCK) void triplane_bwd(BwdParams P) {
    extern __shared__ float part[];      // [segments of this workgroup][C]
    const int t0 = P.wg_tex[blockIdx.x], t1 = P.wg_tex[blockIdx.x + 1];
    const int s0 = P.tex_seg[t0];
    int ns = P.tex_seg[t1] - s0;
    if (ns > P.max_segs) ns = P.max_segs;      // a plan that breaks its own bound must not write past the LDS
    const int C = P.C, G = C / CPT, row = 3 * C;

    // pass 1: segment partials, sequential from +0 in entry order
    for (int q = threadIdx.x; q < ns * G; q += BWD_BLOCK) {
        const int sl = q / G, cg = q - sl * G;
        const int a = P.seg_entry[s0 + sl], b = P.seg_entry[s0 + sl + 1];
        float acc[CPT];
#pragma unroll
        for (int c = 0; c < CPT; ++c) acc[c] = 0.0f;
#pragma unroll 4
        for (int j = a; j < b; ++j) {
            const int e = P.entries[j];
            const int i = e / 12, rem = e - i * 12;
            const int k = rem >> 2, t = rem & 3;
            const float* g = P.coords + (int64_t)i * 3;
            float u, v;
            plane_uv(g[0], g[1], g[2], k, u, v);
            const float w = tap_weight(unnormalize(u, v, P.H, P.W), t);
            float gv[CPT];
            load_g<CPT>(P.gout + (int64_t)i * row + k * C + cg * CPT, gv);
#pragma unroll
            for (int c = 0; c < CPT; ++c) acc[c] = acc[c] + gv[c] * w;
        }
#pragma unroll
        for (int c = 0; c < CPT; ++c) part[sl * C + cg * CPT + c] = acc[c];
    }
    __syncthreads();

    // pass 2: per (texel, channel), the partials in segment order from +0; consecutive threads on consecutive texels
    const int nt = t1 - t0;
    const int HW = P.H * P.W;
    for (int q = threadIdx.x; q < nt * C; q += BWD_BLOCK) {
        const int c = q / nt, tl = q - c * nt;
        const int tx = t0 + tl;
        int a = P.tex_seg[tx] - s0, b = P.tex_seg[tx + 1] - s0;
        if (b > ns) b = ns;
        float acc = 0.0f;
        for (int s = a; s < b; ++s) acc = acc + part[s * C + c];
        const int face = tx >= 3 * HW;
        const int tt = tx - (face ? 3 * HW : 0);
        const int k = tt / HW, yx = tt - k * HW;
        (face ? P.gface : P.gbody)[((int64_t)k * C + c) * HW + yx] = acc;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

EXA_ABI_STATUS("exa_triplane")

int check_shape(int32_t N, int32_t C, int32_t H, int32_t W) {
    if (N < 0) return fail(EXA_TRIPLANE_E_INVALID, "negative row count");
    if (N > EXA_TRIPLANE_MAX_ROWS) return fail(EXA_TRIPLANE_E_INVALID, "more than 2^27 rows");
    if (C < 1 || C > EXA_TRIPLANE_MAX_C) return fail(EXA_TRIPLANE_E_INVALID, "C must be 1 .. 1024");
    if (H < 1 || W < 1) return fail(EXA_TRIPLANE_E_INVALID, "H and W must be >= 1");
    if ((int64_t)6 * H * W > EXA_TRIPLANE_MAX_TEXELS) return fail(EXA_TRIPLANE_E_INVALID, "6 H W exceeds 2^28 texels");
    return 0;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace exa_triplane_impl

using namespace exa_triplane_impl;

extern "C" {

int exa_triplane_version(void) { return EXA_TRIPLANE_VERSION; }

const char* exa_triplane_last_error(void) { return g_err; }

int exa_triplane_plan_keys(int32_t N, int32_t H, int32_t W, const float* coords, const uint8_t* is_face, int32_t* keys,
                           void* stream) {
    if (int rc = check_shape(N, 1, H, W)) return rc;
    if (N == 0) return 0;
    if (!coords || !is_face || !keys) return fail(EXA_TRIPLANE_E_NULLPTR, "coords / is_face / keys is NULL");
    KeyParams P = {N, H, W, coords, is_face, keys};
    hipLaunchKernelGGL(triplane_plan_keys, dim3(ceil_div((int64_t)N * 3, KEY_BLOCK)), dim3(KEY_BLOCK), 0,
                       (hipStream_t)stream, P);
    return launched("triplane_plan_keys");
}

int exa_triplane_forward(int32_t N, int32_t C, int32_t H, int32_t W, const float* body, const float* face,
                         const float* coords, const uint8_t* is_face, float* out, void* stream) {
    if (int rc = check_shape(N, C, H, W)) return rc;
    if (N == 0) return 0;
    if (!body || !face) return fail(EXA_TRIPLANE_E_NULLPTR, "body / face is NULL");
    if (!coords || !is_face || !out) return fail(EXA_TRIPLANE_E_NULLPTR, "coords / is_face / out is NULL");
    FwdParams P = {N, C, H, W, body, face, coords, is_face, out};
    hipStream_t st = (hipStream_t)stream;
    if (C % 4 == 0 && aligned16(out)) {
        hipLaunchKernelGGL(triplane_fwd<4>, dim3(ceil_div((int64_t)N * 3 * (C / 4), FWD_BLOCK)), dim3(FWD_BLOCK), 0,
                           st, P);
    } else {
        hipLaunchKernelGGL(triplane_fwd<1>, dim3(ceil_div((int64_t)N * 3 * C, FWD_BLOCK)), dim3(FWD_BLOCK), 0, st, P);
    }
    return launched("triplane_fwd");
}

int exa_triplane_backward(int32_t N, int32_t C, int32_t H, int32_t W, const float* coords, const float* grad_out,
                          const int32_t* entries, const int32_t* seg_entry, const int32_t* tex_seg,
                          const int32_t* wg_tex, int32_t num_wg, int32_t max_wg_segments, float* grad_body,
                          float* grad_face, void* stream) {
    if (int rc = check_shape(N, C, H, W)) return rc;
    if (num_wg < 1) return fail(EXA_TRIPLANE_E_INVALID, "num_wg must be >= 1");
    if (max_wg_segments < 1 || (int64_t)max_wg_segments * C * 4 > EXA_TRIPLANE_MAX_LDS)
        return fail(EXA_TRIPLANE_E_INVALID, "max_wg_segments * C * 4 must be 4 .. 65536 bytes");
    if (!grad_body || !grad_face) return fail(EXA_TRIPLANE_E_NULLPTR, "grad_body / grad_face is NULL");
    if (!seg_entry || !tex_seg || !wg_tex) return fail(EXA_TRIPLANE_E_NULLPTR, "seg_entry / tex_seg / wg_tex is NULL");
    if (N > 0 && (!coords || !grad_out || !entries))
        return fail(EXA_TRIPLANE_E_NULLPTR, "coords / grad_out / entries is NULL");
    BwdParams P = {N, C, H, W, max_wg_segments, coords, grad_out, entries, seg_entry, tex_seg, wg_tex, grad_body,
                   grad_face};
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)max_wg_segments * C * sizeof(float);
    if (C % 4 == 0 && (N == 0 || aligned16(grad_out)))
        hipLaunchKernelGGL(triplane_bwd<4>, dim3(num_wg), dim3(BWD_BLOCK), lds, st, P);
    else
        hipLaunchKernelGGL(triplane_bwd<1>, dim3(num_wg), dim3(BWD_BLOCK), lds, st, P);
    return launched("triplane_bwd");
}

}  // extern "C"
