// The house sums: every fp32 sum over lanes, waves or partials whose order a public header promises, stated once.  The
// contracts: include/exa_mesh.h ("WG(s)", "added as a tree") and include/exa_raster.h (the face L1 mean, the LPIPS head).
// Device code only.  The wave sums work in place.  ssim.hip's (w0 + w1) + (w2 + w3) pairing is its own and stays there.
#pragma once
#include <hip/hip_runtime.h>

namespace exa {

// The wave butterfly: for d = 32 .. 1, s = s + s[lane ^ d].  Both partners form the same sum, so every lane ends with the
// wave's.  All 64 lanes must be active.
__device__ __forceinline__ void wave_sum_all(float& s) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s = s + __shfl_xor(s, d, 64);
}

// The wave tree: for d = 32 .. 1, q = q + q[lane + d].  Only lane 0 ends with the wave's sum, in the same bits as lane 0 of
// the butterfly: after the step of distance d the lanes below d hold the same additions of the same operands in both.
__device__ __forceinline__ void wave_sum_lane0(float& q) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) q = q + __shfl_down(q, d, 64);
}

// The workgroup sum of four waves, N values at once: the butterfly, then ((wave 0 + wave 1) + wave 2) + wave 3.  Every thread
// calls it and ends with the sums.  No barrier follows the LDS reads: a second call in a kernel needs a __syncthreads() first.
template <int WAVES, int N>
__device__ __forceinline__ void block_sums(float (&s)[N]) {
    static_assert(WAVES == 4, "the order is written out for four waves");
    __shared__ float wave_sum[N][WAVES];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        wave_sum_all(s[k]);
        if ((threadIdx.x & 63) == 0) wave_sum[k][threadIdx.x >> 6] = s[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = ((wave_sum[k][0] + wave_sum[k][1]) + wave_sum[k][2]) + wave_sum[k][3];
}

template <int WAVES>
__device__ __forceinline__ float block_sum(float s) {
    float v[1] = {s};
    block_sums<WAVES>(v);
    return v[0];
}

// The strided partial sum of a workgroup of BLOCK threads: thread t returns ((+0.0 + p[t]) + p[t + BLOCK]) + ..
template <int BLOCK, typename Index>
__device__ __forceinline__ float strided_sum(const float* p, Index n) {
    float s = 0.0f;
    for (Index j = threadIdx.x; j < n; j += BLOCK) s = s + p[j];
    return s;
}

// The same in one walk over N rows of n partials that lie `stride` apart: s[k] = s[k] + p[k * stride + t], + BLOCK, ..
template <int BLOCK, int N, typename Index>
__device__ __forceinline__ void strided_sums(float* s, const float* p, Index n, Index stride) {
    for (Index j = threadIdx.x; j < n; j += BLOCK)
#pragma unroll
        for (int k = 0; k < N; ++k) s[k] = s[k] + p[k * stride + j];
}

}  // namespace exa
