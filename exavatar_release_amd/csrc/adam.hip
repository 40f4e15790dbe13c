// The Adam step for gfx950 (include/exa_raster.h, exa_raster_adam_step): the update of torch.optim.Adam without weight
// decay or amsgrad for up to 64 separately allocated tensors in one launch.  The header writes out every operation;
// tests/adam_oracle.py restates them in numpy.  Compiled with -ffp-contract=off and no fast-math flag: `/` and sqrtf are
// the correctly rounded expansions (v_div_scale / v_div_fmas / v_div_fixup; v_sqrt_f32 and its corrections).
//
//   adam_step   memory-bound and elementwise: 16 B read and 12 B written per element.  A workgroup of ADAM_BLOCK = 256
//               threads owns one chunk of ADAM_CHUNK = 4096 consecutive elements of one segment (16 KiB of each of its four
//               arrays).  The chunk counts of the segments lie end to end on the grid; the segments and the prefix counts
//               travel BY VALUE in the argument block (3.3 KiB), so there is no device table, no copy and no state between
//               calls.  blockIdx.x is wave-uniform: the binary search over the prefix counts and the loads of the
//               segment's record are scalar loads of the argument block.  A thread moves ADAM_VEC = 4 consecutive floats,
//               ADAM_ITERS = 4 times at a stride of 1024 floats, so that every wave instruction covers 1 KiB contiguously.
//               A full chunk of a 16-byte aligned segment issues its sixteen 16-byte loads before the first use; a partial
//               chunk goes group by group, the last n % 4 elements one by one; a segment with a misaligned array goes
//               element by element (lane i at element i: still coalesced).  A chunk starts 16 KiB into its arrays, so it
//               is aligned as its segment is.  No LDS, no barrier, no atomics: the same inputs give the same bits.
#include <cmath>

#include "../../include/exa_raster.h"
#include "abi_status.h"

namespace exa {

// the kernel's argument block, as exa_raster_adam_step fills it: up to ADAM_MAX_SEGMENTS non-empty tensors
constexpr int ADAM_MAX_SEGMENTS = 64;
struct AdamArgs {
    int32_t n_seg;                             // 1 .. ADAM_MAX_SEGMENTS, every one with n > 0
    float w1, b2, w2, eps;                     // (float)(1 - beta1), (float)beta2, (float)(1 - beta2), (float)eps
    uint32_t start[ADAM_MAX_SEGMENTS + 1];     // first chunk of every segment; start[n_seg] = the grid
    ExaRasterAdamSegment seg[ADAM_MAX_SEGMENTS];
};

namespace {

constexpr int ADAM_BLOCK = 256;
constexpr int ADAM_VEC = 4;
constexpr int ADAM_ITERS = 4;
constexpr int ADAM_CHUNK = EXA_RASTER_ADAM_CHUNK;
constexpr int ADAM_STRIDE = ADAM_BLOCK * ADAM_VEC;       // floats a workgroup moves per iteration
static_assert(ADAM_CHUNK == ADAM_STRIDE * ADAM_ITERS, "chunk = block x vector x iterations");
static_assert(ADAM_MAX_SEGMENTS == EXA_RASTER_ADAM_MAX_SEGMENTS, "segments per launch");
static_assert(sizeof(AdamArgs) <= 4096, "the argument block of a HIP kernel holds 4 KiB");

struct AdamScalars {
    float w1, one_minus_w1, b2, w2, eps, neg_step, bc2_sqrt;
    bool lerp_hi;
};

// the five lines of include/exa_raster.h for one element
__device__ __forceinline__ void adam_element(const AdamScalars& S, float g, float& p, float& m, float& v) {
    const float d0 = g - m;
    m = S.lerp_hi ? g - d0 * S.one_minus_w1 : m + S.w1 * d0;
    v = v * S.b2 + (S.w2 * g) * g;
    const float d = sqrtf(v) / S.bc2_sqrt + S.eps;
    p = p + S.neg_step * (m / d);
}

__device__ __forceinline__ void adam_four(const AdamScalars& S, const float4& g, float4& p, float4& m, float4& v) {
    adam_element(S, g.x, p.x, m.x, v.x);
    adam_element(S, g.y, p.y, m.y, v.y);
    adam_element(S, g.z, p.z, m.z, v.z);
    adam_element(S, g.w, p.w, m.w, v.w);
}

__global__ __launch_bounds__(ADAM_BLOCK) void adam_step(AdamArgs A) {
    const uint32_t b = blockIdx.x;
    int lo = 0, hi = A.n_seg;                 // the last segment whose first chunk is <= b: start[] is strictly increasing
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (b >= A.start[mid]) lo = mid; else hi = mid;
    }
    const int64_t base = (int64_t)(b - A.start[lo]) * ADAM_CHUNK;
    const int64_t n = A.seg[lo].n - base;     // elements from this chunk's first to the segment's end: > 0
    float* const p = A.seg[lo].param + base;
    const float* const g = A.seg[lo].grad + base;
    float* const m = A.seg[lo].exp_avg + base;
    float* const v = A.seg[lo].exp_avg_sq + base;
    AdamScalars S;
    S.w1 = A.w1; S.one_minus_w1 = 1.0f - A.w1; S.b2 = A.b2; S.w2 = A.w2; S.eps = A.eps;
    S.neg_step = -A.seg[lo].step_size; S.bc2_sqrt = A.seg[lo].bc2_sqrt;
    S.lerp_hi = !(A.w1 < 0.5f);
    const bool aligned = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
    const int t = threadIdx.x;
    if (aligned && n >= ADAM_CHUNK) {
        float4 P[ADAM_ITERS], G[ADAM_ITERS], M[ADAM_ITERS], V[ADAM_ITERS];
#pragma unroll
        for (int it = 0; it < ADAM_ITERS; ++it) {
            const int i = it * ADAM_STRIDE + t * ADAM_VEC;
            G[it] = *reinterpret_cast<const float4*>(g + i);
            M[it] = *reinterpret_cast<const float4*>(m + i);
            V[it] = *reinterpret_cast<const float4*>(v + i);
            P[it] = *reinterpret_cast<const float4*>(p + i);
        }
#pragma unroll
        for (int it = 0; it < ADAM_ITERS; ++it) {
            const int i = it * ADAM_STRIDE + t * ADAM_VEC;
            adam_four(S, G[it], P[it], M[it], V[it]);
            *reinterpret_cast<float4*>(m + i) = M[it];
            *reinterpret_cast<float4*>(v + i) = V[it];
            *reinterpret_cast<float4*>(p + i) = P[it];
        }
    } else if (aligned) {
        const int left = (int)n;              // < ADAM_CHUNK
        for (int i = t * ADAM_VEC; i < left; i += ADAM_STRIDE) {
            if (i + ADAM_VEC <= left) {
                const float4 G = *reinterpret_cast<const float4*>(g + i);
                float4 M = *reinterpret_cast<const float4*>(m + i);
                float4 V = *reinterpret_cast<const float4*>(v + i);
                float4 P = *reinterpret_cast<const float4*>(p + i);
                adam_four(S, G, P, M, V);
                *reinterpret_cast<float4*>(m + i) = M;
                *reinterpret_cast<float4*>(v + i) = V;
                *reinterpret_cast<float4*>(p + i) = P;
            } else {
                for (int k = i; k < left; ++k) {
                    float pk = p[k], mk = m[k], vk = v[k];
                    adam_element(S, g[k], pk, mk, vk);
                    m[k] = mk; v[k] = vk; p[k] = pk;
                }
            }
        }
    } else {
        const int left = n < ADAM_CHUNK ? (int)n : ADAM_CHUNK;
        for (int k = t; k < left; k += ADAM_BLOCK) {
            float pk = p[k], mk = m[k], vk = v[k];
            adam_element(S, g[k], pk, mk, vk);
            m[k] = mk; v[k] = vk; p[k] = pk;
        }
    }
}

}  // namespace

}  // namespace exa

namespace exa_raster_impl {
using namespace exa;
EXA_ABI_STATUS_SHARED("exa_raster")       // exa_raster_last_error() and its buffer are api.hip's
}  // namespace exa_raster_impl

using namespace exa_raster_impl;

extern "C" int exa_raster_adam_step(const ExaRasterAdamSegment* segs, int32_t n_seg, double beta1, double beta2, double eps,
                                    void* stream) {
    if (n_seg < 0) return fail(EXA_RASTER_E_INVALID, "adam: negative n_seg");
    if (n_seg > 0 && !segs) return fail(EXA_RASTER_E_NULLPTR, "adam: segs is NULL");
    if (!std::isfinite(beta1) || !std::isfinite(beta2) || !std::isfinite(eps))
        return fail(EXA_RASTER_E_INVALID, "adam: beta1, beta2 and eps must be finite");
    if (beta1 < 0.0 || beta1 >= 1.0 || beta2 < 0.0 || beta2 >= 1.0)
        return fail(EXA_RASTER_E_INVALID, "adam: beta1 and beta2 must be in [0, 1)");
    if (eps < 0.0) return fail(EXA_RASTER_E_INVALID, "adam: eps must be >= 0");
    for (int32_t s = 0; s < n_seg; ++s) {      // every segment before the first launch
        const ExaRasterAdamSegment& g = segs[s];
        if (g.n < 0) return fail(EXA_RASTER_E_INVALID, "adam: negative n in a segment");
        if (g.n > EXA_RASTER_ADAM_MAX_N) return fail(EXA_RASTER_E_INVALID, "adam: more than 2^36 elements in a segment (EXA_RASTER_ADAM_MAX_N)");
        if (g.n == 0) continue;
        if (!g.param || !g.grad || !g.exp_avg || !g.exp_avg_sq)
            return fail(EXA_RASTER_E_NULLPTR, "adam: a segment with n > 0 holds a NULL pointer");
        if (!std::isfinite(g.step_size) || !std::isfinite(g.bc2_sqrt))
            return fail(EXA_RASTER_E_INVALID, "adam: step_size and bc2_sqrt must be finite");
        if (!(g.bc2_sqrt > 0.0f)) return fail(EXA_RASTER_E_INVALID, "adam: bc2_sqrt must be > 0 (a step count >= 1)");
    }
    AdamArgs A;
    A.w1 = (float)(1.0 - beta1); A.b2 = (float)beta2; A.w2 = (float)(1.0 - beta2); A.eps = (float)eps;
    A.n_seg = 0;
    A.start[0] = 0;
    for (int32_t s = 0; s <= n_seg; ++s) {     // the non-empty segments, ADAM_MAX_SEGMENTS to a launch
        if (s < n_seg && segs[s].n > 0) {
            A.seg[A.n_seg] = segs[s];
            A.start[A.n_seg + 1] = A.start[A.n_seg] + (uint32_t)((segs[s].n + EXA_RASTER_ADAM_CHUNK - 1) / EXA_RASTER_ADAM_CHUNK);
            ++A.n_seg;
        }
        if (A.n_seg == ADAM_MAX_SEGMENTS || (s == n_seg && A.n_seg > 0)) {
            for (int k = A.n_seg + 1; k <= ADAM_MAX_SEGMENTS; ++k) A.start[k] = A.start[A.n_seg];
            for (int k = A.n_seg; k < ADAM_MAX_SEGMENTS; ++k) A.seg[k] = ExaRasterAdamSegment{};
            hipLaunchKernelGGL(adam_step, dim3(A.start[A.n_seg]), dim3(ADAM_BLOCK), 0, static_cast<hipStream_t>(stream), A);
            if (int rc = launched("adam_step")) return rc;
            A.n_seg = 0;
        }
    }
    return 0;
}
