// Mesh Laplacian regulariser (include/exa_mesh.h, the reference's LaplacianReg, loss.py:97-131) with an atomic-free
// backward.  The semantics -- the op-by-op fp32 forward and the backward's summation order -- are written out in the
// header; this file implements them.
//
//   lap_fwd         one thread per (b, v), one workgroup per 256 vertices.  The workgroup stages its 256 rows of the
//                   neighbour table (indices and weights, contiguous in memory) in LDS with coalesced loads, then every
//                   thread walks its row once for `out` and once for `target`, C channels at a time, and writes d and
//                   loss.  The gathered rows of x come through the caches (x is a few MB).
//   lap_bwd_stage   one thread per (b, u): g = (grad_loss * weight) * (2 d) into the workspace.
//   lap_bwd_gather  one thread per (b, v): g[b,v] plus its incoming slots in CSR order (ascending u, then k), each
//                   nbr_w[u,k] * g[b,u]; the CSR entry u * K + k is also the weight's flat index.
// No atomics, no memsets, no allocation, no synchronisation: every output element is one thread's sum in the header's
// order.  Compiled with -ffp-contract=off (build.py): the products must not be contracted into fused multiply-adds.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/exa_mesh.h"
#include "abi_status.h"
#include "index_transpose.h"

namespace exa_mesh_impl {

using exa::align256;
using exa::ceil_div;

EXA_ABI_STATUS_SHARED("exa_mesh")         // exa_mesh_last_error() and its buffer are mesh_raster.hip's

constexpr int LAP_BLOCK = 256;
constexpr int LAP_MAXC = EXA_MESH_LAP_MAX_CHANNELS;
constexpr int LAP_MAXK = EXA_MESH_LAP_MAX_NEIGHBORS;
constexpr int LAP_LD = LAP_MAXK + 1;          // LDS row stride of the staged table (odd: lane-per-row reads do not share a bank)
constexpr int64_t LAP_MAX_SLOTS = 1 << 28;    // V * K: the CSR entries are int32
constexpr int LAP_MAX_BATCH = 65535;          // B is a grid dimension of the forward
constexpr int64_t LAP_MAX_ELEMS = 1 << 30;    // B * V * C
static_assert((LAP_MAXK & (LAP_MAXK - 1)) == 0 && LAP_BLOCK % LAP_MAXK == 0, "the staging loop's (row, slot) split");

__device__ __forceinline__ float lap_qnan() { return __int_as_float(0x7fc00000); }

template <int C>
__device__ __forceinline__ void load_row(const float* p, float (&r)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) r[c] = p[c];
}

struct LapFwdParams {
    int32_t B, Bt, V, K;
    const float* out;
    const float* target;                      // NULL: no target
    const int32_t* nbr_idx;
    const float* nbr_w;
    const float* weight;                      // NULL: no weight
    float* loss;
    float* d;
};

// lap(x)[v]: x[v], then the K slots of the staged row in order
template <int C>
__device__ __forceinline__ void lap_row(const float* x, int64_t v, const int* il, const float* wl, int K, int V,
                                        float (&acc)[C]) {
    load_row<C>(x + v * C, acc);
    for (int k = 0; k < K; ++k) {
        const int j = il[k];
        const float w = wl[k];
        float r[C];
        if ((unsigned)j < (unsigned)V) {                       // the guard: a row outside [0, V) is never read
            load_row<C>(x + (int64_t)j * C, r);
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) r[c] = lap_qnan();
        }
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = acc[c] + r[c] * w;
    }
}

template <int C>
__global__ __launch_bounds__(LAP_BLOCK) void lap_fwd(LapFwdParams P) {
    __shared__ int idxl[LAP_BLOCK * LAP_LD];
    __shared__ float wl[LAP_BLOCK * LAP_LD];
    const int tid = threadIdx.x, K = P.K, V = P.V;
    const int64_t v0 = (int64_t)blockIdx.x * LAP_BLOCK;
    // the tile's rows are contiguous in the table: thread (r, k) of a pass loads slot k of row r, 16 rows per pass
    {
        const int k = tid & (LAP_MAXK - 1);
        for (int r = tid / LAP_MAXK; r < LAP_BLOCK; r += LAP_BLOCK / LAP_MAXK) {
            if (k < K && v0 + r < V) {
                const int64_t s = (v0 + r) * K + k;
                idxl[r * LAP_LD + k] = P.nbr_idx[s];
                wl[r * LAP_LD + k] = P.nbr_w[s];
            }
        }
    }
    __syncthreads();
    const int64_t v = v0 + tid;
    if (v >= V) return;
    const int b = blockIdx.y;
    const int* il = idxl + tid * LAP_LD;
    const float* wr = wl + tid * LAP_LD;
    float dd[C];
    lap_row<C>(P.out + (int64_t)b * V * C, v, il, wr, K, V, dd);
    if (P.target) {
        float t[C];
        lap_row<C>(P.target + (int64_t)(P.Bt == 1 ? 0 : b) * V * C, v, il, wr, K, V, t);
#pragma unroll
        for (int c = 0; c < C; ++c) dd[c] = dd[c] - t[c];
    }
    const int64_t o = ((int64_t)b * V + v) * C;
    const bool weighted = P.weight != nullptr;
    const float wv = weighted ? P.weight[v] : 1.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float l = dd[c] * dd[c];
        if (weighted) l = l * wv;
        P.d[o + c] = dd[c];
        P.loss[o + c] = l;
    }
}

struct LapBwdParams {
    int32_t B, V, K;
    const float* d;
    const float* grad_loss;
    const float* nbr_w;
    const float* weight;                      // NULL: no weight
    const int32_t* offsets;
    const int32_t* entries;
    float* g;                                 // workspace [B, V, C]
    float* dout;
};

template <int C>
__global__ __launch_bounds__(LAP_BLOCK) void lap_bwd_stage(LapBwdParams P) {
    const int64_t i = (int64_t)blockIdx.x * LAP_BLOCK + threadIdx.x;
    if (i >= (int64_t)P.B * P.V) return;
    const int u = (int)(i % P.V);
    float gl[C], dd[C];
    load_row<C>(P.grad_loss + i * C, gl);
    load_row<C>(P.d + i * C, dd);
    if (P.weight) {
        const float wu = P.weight[u];
#pragma unroll
        for (int c = 0; c < C; ++c) gl[c] = gl[c] * wu;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) P.g[i * C + c] = gl[c] * (2.0f * dd[c]);
}

template <int C>
__global__ __launch_bounds__(LAP_BLOCK) void lap_bwd_gather(LapBwdParams P) {
    const int64_t i = (int64_t)blockIdx.x * LAP_BLOCK + threadIdx.x;
    if (i >= (int64_t)P.B * P.V) return;
    const int V = P.V, K = P.K;
    const int v = (int)(i % V);
    const float* g = P.g + (i - v) * C;                        // this batch element's [V, C]
    const unsigned slots = (unsigned)V * (unsigned)K;
    float acc[C];
    load_row<C>(g + (int64_t)v * C, acc);
    for (int q = P.offsets[v], end = P.offsets[v + 1]; q < end; ++q) {
        const unsigned e = (unsigned)P.entries[q];
        float w, r[C];
        if (e < slots) {                                       // the guard: nothing outside the tables is read
            w = P.nbr_w[e];
            load_row<C>(g + (int64_t)(e / (unsigned)K) * C, r);
        } else {
            w = lap_qnan();
#pragma unroll
            for (int c = 0; c < C; ++c) r[c] = lap_qnan();
        }
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = acc[c] + w * r[c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) P.dout[i * C + c] = acc[c];
}

// ---- host side ------------------------------------------------------------------------------------------------------

int lap_check_shape(int32_t B, int32_t V, int32_t C, int32_t K) {
    if (B < 0 || V < 0) return fail(EXA_MESH_E_INVALID, "negative size");
    if (C < 1 || C > LAP_MAXC) return fail(EXA_MESH_E_INVALID, "C (channels) must be 1 .. 8");
    if (K < 1 || K > LAP_MAXK) return fail(EXA_MESH_E_INVALID, "K (neighbours per vertex) must be 1 .. 16");
    if ((int64_t)V * K > LAP_MAX_SLOTS) return fail(EXA_MESH_E_INVALID, "V * K exceeds 2^28");
    if (B > LAP_MAX_BATCH) return fail(EXA_MESH_E_INVALID, "B exceeds 65535");
    if ((int64_t)B * V * C > LAP_MAX_ELEMS) return fail(EXA_MESH_E_INVALID, "B * V * C exceeds 2^30");
    return 0;
}

uint64_t lap_workspace_bytes(int32_t B, int32_t V, int32_t C) { return align256((uint64_t)B * V * C * sizeof(float)); }

// KERNEL<C> for the run-time C
#define LAP_LAUNCH(KERNEL, C, grid, st, P)                                                                             \
    switch (C) {                                                                                                       \
        case 1: hipLaunchKernelGGL(KERNEL<1>, grid, dim3(LAP_BLOCK), 0, st, P); break;                                 \
        case 2: hipLaunchKernelGGL(KERNEL<2>, grid, dim3(LAP_BLOCK), 0, st, P); break;                                 \
        case 3: hipLaunchKernelGGL(KERNEL<3>, grid, dim3(LAP_BLOCK), 0, st, P); break;                                 \
        case 4: hipLaunchKernelGGL(KERNEL<4>, grid, dim3(LAP_BLOCK), 0, st, P); break;                                 \
        case 5: hipLaunchKernelGGL(KERNEL<5>, grid, dim3(LAP_BLOCK), 0, st, P); break;                                 \
        case 6: hipLaunchKernelGGL(KERNEL<6>, grid, dim3(LAP_BLOCK), 0, st, P); break;                                 \
        case 7: hipLaunchKernelGGL(KERNEL<7>, grid, dim3(LAP_BLOCK), 0, st, P); break;                                 \
        default: hipLaunchKernelGGL(KERNEL<8>, grid, dim3(LAP_BLOCK), 0, st, P); break;                                \
    }

}  // namespace exa_mesh_impl

using namespace exa_mesh_impl;

extern "C" {

int exa_mesh_neighbor_transpose(int32_t V, int32_t K, const int32_t* nbr_idx, int32_t* offsets, int32_t* entries) {
    if (V < 0) return fail(EXA_MESH_E_INVALID, "negative size");
    if (K < 1 || K > LAP_MAXK) return fail(EXA_MESH_E_INVALID, "K (neighbours per vertex) must be 1 .. 16");
    if ((int64_t)V * K > LAP_MAX_SLOTS) return fail(EXA_MESH_E_INVALID, "V * K exceeds 2^28");
    if (!offsets || (V > 0 && (!nbr_idx || !entries))) return fail(EXA_MESH_E_NULLPTR, "NULL argument");
    // ascending (u, k) per vertex: the shared index transpose (index_transpose.h)
    const int64_t e = exa::index_transpose(V, (int64_t)V * K, nbr_idx, false, offsets, entries);
    if (e >= 0) {
        char what[128];
        snprintf(what, sizeof(what), "neighbour index %d of vertex %d, slot %d is outside [0, %d)", (int)nbr_idx[e],
                 (int)(e / K), (int)(e % K), (int)V);
        return fail(EXA_MESH_E_INVALID, what);
    }
    return 0;
}

int exa_mesh_laplacian_forward(int32_t B, int32_t Bt, int32_t V, int32_t C, int32_t K, const float* out,
                               const float* target, const int32_t* nbr_idx, const float* nbr_w, const float* weight,
                               float* loss, float* d, void* stream) {
    if (int rc = lap_check_shape(B, V, C, K)) return rc;
    if (target && Bt != 1 && Bt != B) return fail(EXA_MESH_E_INVALID, "Bt (target batch) must be 1 or B");
    if (B == 0 || V == 0) return 0;
    if (!out || !nbr_idx || !nbr_w) return fail(EXA_MESH_E_NULLPTR, "out / nbr_idx / nbr_w is NULL");
    if (!loss || !d) return fail(EXA_MESH_E_NULLPTR, "loss / d is NULL");
    const LapFwdParams P = {B, Bt, V, K, out, target, nbr_idx, nbr_w, weight, loss, d};
    const dim3 grid(ceil_div(V, LAP_BLOCK), B);
    LAP_LAUNCH(lap_fwd, C, grid, (hipStream_t)stream, P)
    return launched("lap_fwd");
}

int exa_mesh_laplacian_workspace_size(int32_t B, int32_t V, int32_t C, uint64_t* out_bytes) {
    if (!out_bytes) return fail(EXA_MESH_E_NULLPTR, "out_bytes is NULL");
    if (int rc = lap_check_shape(B, V, C, 1)) return rc;
    *out_bytes = lap_workspace_bytes(B, V, C);
    return 0;
}

int exa_mesh_laplacian_backward(int32_t B, int32_t V, int32_t C, int32_t K, const float* d, const float* grad_loss,
                                const float* nbr_w, const float* weight, const int32_t* in_offsets,
                                const int32_t* in_entries, void* ws, uint64_t ws_bytes, float* dL_dout, void* stream) {
    if (int rc = lap_check_shape(B, V, C, K)) return rc;
    if (B == 0 || V == 0) return 0;
    if (!d || !grad_loss || !nbr_w) return fail(EXA_MESH_E_NULLPTR, "d / grad_loss / nbr_w is NULL");
    if (!in_offsets || !in_entries) return fail(EXA_MESH_E_NULLPTR, "in_offsets / in_entries is NULL");
    if (!dL_dout) return fail(EXA_MESH_E_NULLPTR, "dL_dout is NULL");
    if (!ws) return fail(EXA_MESH_E_NULLPTR, "ws (workspace) is NULL");
    if (ws_bytes < lap_workspace_bytes(B, V, C))
        return fail(EXA_MESH_E_INVALID, "workspace is smaller than exa_mesh_laplacian_workspace_size");
    const LapBwdParams P = {B, V, K, d, grad_loss, nbr_w, weight, in_offsets, in_entries, (float*)ws, dL_dout};
    const dim3 grid(ceil_div((int64_t)B * V, LAP_BLOCK));
    hipStream_t st = (hipStream_t)stream;
    LAP_LAUNCH(lap_bwd_stage, C, grid, st, P)
    if (int rc = launched("lap_bwd_stage")) return rc;
    LAP_LAUNCH(lap_bwd_gather, C, grid, st, P)
    return launched("lap_bwd_gather");
}

}  // extern "C"
