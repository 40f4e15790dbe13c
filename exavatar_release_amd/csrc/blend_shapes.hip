// Blend-shape offsets (include/exa_mesh.h, exa_mesh_blend_*): the reference's pose correctives
// (get_mean_offset_offset, module.py:473-493) and expression offsets (module.py:537) as one operation -- a short
// coefficient vector times a compacted, feature-major table, scattered to a flat [M] output.  The semantics -- the
// op-by-op fp32 forward, its K-segments and the backward's two-level sum -- are written out in the header; this file
// implements them.
//
//   blend_fwd          one launch.  Workgroups [0, tiles) each own 256 compact columns: wave w of the eight sums
//                      K-segment w of its four columns per lane (16-byte loads along the column axis, eight rows in
//                      flight per lane, coef staged in LDS), the eight partials meet in LDS and 256 threads add them in
//                      ascending segment order and scatter through `cols`.  Workgroups [tiles, tiles + fill) write the
//                      outputs no column covers (base or +0.0), so nothing needs a memset.
//   blend_bwd_partial  workgroup (chunk, row group): 1024 compact columns x 16 table rows.  Every thread gathers the
//                      gradients of its four columns once, then per row forms its four products, the wave adds the 64
//                      lanes in a fixed tree and the four wave sums are added in ascending order: one partial per
//                      (chunk, row) into the caller's workspace.
//   blend_bwd_finish   dL/dcoef[k] = the chunks' partials in ascending chunk order (one thread per k), and dL/dbase
//                      elementwise, in the same launch.
// No atomics, no memsets, no allocation, no synchronisation: every output element is one thread's sum in the header's
// order.  Compiled with -ffp-contract=off (build.py): the products must not be contracted into fused multiply-adds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/exa_mesh.h"
#include "abi_status.h"
#include "fixed_sum.h"

namespace exa_mesh_impl {

using exa::align256;
using exa::ceil_div;

EXA_ABI_STATUS_SHARED("exa_mesh")         // exa_mesh_last_error() and its buffer are mesh_raster.hip's

constexpr int BL_SEGS = EXA_MESH_BLEND_SEGMENTS;
constexpr int BL_MAXK = EXA_MESH_BLEND_MAX_K;
constexpr int BL_BLOCK = 64 * BL_SEGS;        // one wave per K-segment
constexpr int BL_TILE = 256;                  // compact columns per workgroup: 64 lanes x 4
constexpr int BL_ROWS = 8;                    // table rows in flight per lane
constexpr int BL_FILL = 4 * BL_BLOCK;         // outputs per fill workgroup
constexpr int BLB_BLOCK = 256;
constexpr int BLB_WAVES = BLB_BLOCK / 64;
constexpr int BLB_CHUNK = EXA_MESH_BLEND_CHUNK;
constexpr int BLB_ROWS = 16;                  // table rows per workgroup of the backward
constexpr int BLB_FLIGHT = 4;                 // of which in flight per lane
constexpr int64_t BL_MAX_OUT = 1 << 30;       // M
static_assert(BLB_CHUNK == 4 * BLB_BLOCK && BL_TILE == 4 * 64 && BLB_WAVES == 4, "four columns per lane");
static_assert(BL_MAXK <= BL_BLOCK && BLB_ROWS % BLB_FLIGHT == 0, "coef staging, row groups");

struct BlendFwdParams {
    int32_t K, N, ld, M, tiles;
    const float* coef;
    const float* table;
    const int32_t* cols;
    const int32_t* inv;
    const float* base;                        // NULL: the uncovered outputs are +0.0
    float* out;
    float* masked;                            // NULL: not wanted
};

__device__ __forceinline__ void blend_row(float4& acc, float c, const float4& t) {
    acc.x = acc.x + c * t.x;
    acc.y = acc.y + c * t.y;
    acc.z = acc.z + c * t.z;
    acc.w = acc.w + c * t.w;
}

__global__ __launch_bounds__(BL_BLOCK) void blend_fwd(BlendFwdParams P) {
    __shared__ float coef_l[BL_MAXK];
    __shared__ float4 part[BL_SEGS][64];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= P.tiles) {
        // the outputs no compact column covers
        const int64_t j0 = (int64_t)((int)blockIdx.x - P.tiles) * BL_FILL + tid;
#pragma unroll
        for (int i = 0; i < BL_FILL / BL_BLOCK; ++i) {
            const int64_t j = j0 + i * BL_BLOCK;
            if (j < P.M && P.inv[j] < 0) {
                const float v = P.base ? P.base[j] : 0.0f;
                P.out[j] = v;
                if (P.masked) P.masked[j] = v;
            }
        }
        return;
    }
    const int K = P.K;
    if (tid < K) coef_l[tid] = P.coef[tid];
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    const int L = (K + BL_SEGS - 1) / BL_SEGS;                 // rows per segment: a function of K alone
    const int k0 = wave * L;
    const int k1 = min(K, k0 + L);
    const int64_t c = (int64_t)blockIdx.x * BL_TILE + lane * 4;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (c < P.ld) {                                            // ld is a multiple of 4: all four columns exist
        const int64_t ld = P.ld;
        const float* p = P.table + (int64_t)k0 * ld + c;
        int k = k0;
        for (; k + BL_ROWS <= k1; k += BL_ROWS) {
            float4 t[BL_ROWS];
#pragma unroll
            for (int i = 0; i < BL_ROWS; ++i) t[i] = *reinterpret_cast<const float4*>(p + i * ld);
#pragma unroll
            for (int i = 0; i < BL_ROWS; ++i) blend_row(acc, coef_l[k + i], t[i]);
            p += BL_ROWS * ld;
        }
        for (; k < k1; ++k) {
            blend_row(acc, coef_l[k], *reinterpret_cast<const float4*>(p));
            p += ld;
        }
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (tid < BL_TILE) {
        const float* pl = reinterpret_cast<const float*>(&part[0][0]);
        float sum = pl[tid];
#pragma unroll
        for (int s = 1; s < BL_SEGS; ++s) sum = sum + pl[s * BL_TILE + tid];
        const int64_t col = (int64_t)blockIdx.x * BL_TILE + tid;
        if (col < P.N) {
            const int j = P.cols[col];
            if ((unsigned)j < (unsigned)P.M) {                 // the guard: nothing outside the outputs is written
                P.out[j] = sum;
                if (P.masked) P.masked[j] = 0.0f;
            }
        }
    }
}

struct BlendBwdParams {
    int32_t K, N, ld, M, chunks;
    const float* table;
    const int32_t* cols;
    const int32_t* inv;
    const float* g_out;
    const float* g_masked;                    // NULL: none
    float* ws;                                // [chunks, K]
    float* dcoef;                             // NULL: not wanted
    float* dbase;                             // NULL: not wanted
};

__global__ __launch_bounds__(BLB_BLOCK) void blend_bwd_partial(BlendBwdParams P) {
    __shared__ float wl[BLB_ROWS][BLB_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int chunk = blockIdx.x, r0 = blockIdx.y * BLB_ROWS;
    const int64_t c = (int64_t)chunk * BLB_CHUNK + tid * 4;
    float g[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        g[i] = 0.0f;
        if (c + i < P.N) {
            const int j = P.cols[c + i];
            if ((unsigned)j < (unsigned)P.M) g[i] = P.g_out[j];
        }
    }
    const bool inside = c < P.ld;
    const int64_t ld = P.ld;
    for (int r = 0; r < BLB_ROWS; r += BLB_FLIGHT) {
        float4 t[BLB_FLIGHT];
#pragma unroll
        for (int i = 0; i < BLB_FLIGHT; ++i) {
            const int k = r0 + r + i;
            t[i] = (inside && k < P.K) ? *reinterpret_cast<const float4*>(P.table + k * ld + c)
                                       : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (int i = 0; i < BLB_FLIGHT; ++i) {
            float q = ((t[i].x * g[0] + t[i].y * g[1]) + t[i].z * g[2]) + t[i].w * g[3];
            exa::wave_sum_lane0(q);
            if (lane == 0) wl[r + i][wave] = q;                                // lane 0: the header's tree
        }
    }
    __syncthreads();
    if (tid < BLB_ROWS && r0 + tid < P.K)
        P.ws[(int64_t)chunk * P.K + r0 + tid] = ((wl[tid][0] + wl[tid][1]) + wl[tid][2]) + wl[tid][3];
}

__global__ __launch_bounds__(BLB_BLOCK) void blend_bwd_finish(BlendBwdParams P) {
    const int tid = threadIdx.x;
    const int coef_blocks = P.dcoef ? (P.K + BLB_BLOCK - 1) / BLB_BLOCK : 0;
    if ((int)blockIdx.x < coef_blocks) {
        const int k = blockIdx.x * BLB_BLOCK + tid;
        if (k < P.K) {
            float acc = 0.0f;
            for (int ch = 0; ch < P.chunks; ++ch) acc = acc + P.ws[(int64_t)ch * P.K + k];
            P.dcoef[k] = acc;
        }
        return;
    }
    if (!P.dbase) return;
    const int64_t j0 = (int64_t)((int)blockIdx.x - coef_blocks) * (4 * BLB_BLOCK) + tid;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t j = j0 + i * BLB_BLOCK;
        if (j < P.M) {
            float v = 0.0f;
            if (P.inv[j] < 0) {
                if (P.g_out && P.g_masked) v = P.g_out[j] + P.g_masked[j];
                else if (P.g_out) v = P.g_out[j];
                else if (P.g_masked) v = P.g_masked[j];
            }
            P.dbase[j] = v;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

int blend_check_shape(int32_t K, int32_t N, int32_t ld, int32_t M) {
    if (N < 0 || M < 0) return fail(EXA_MESH_E_INVALID, "negative size");
    if (K < 1 || K > BL_MAXK) return fail(EXA_MESH_E_INVALID, "K (blend coefficients) must be 1 .. 512");
    if ((int64_t)M > BL_MAX_OUT) return fail(EXA_MESH_E_INVALID, "M (outputs) exceeds 2^30");
    if (N > M) return fail(EXA_MESH_E_INVALID, "N (compact columns) exceeds M (outputs)");
    if (ld < N || (ld & 3)) return fail(EXA_MESH_E_INVALID, "ld must be a multiple of 4 that is >= N");
    return 0;
}

uint64_t blend_workspace_bytes(int32_t K, int32_t N) {
    return align256((uint64_t)ceil_div(N, BLB_CHUNK) * K * sizeof(float));
}

}  // namespace exa_mesh_impl

using namespace exa_mesh_impl;

extern "C" {

int exa_mesh_blend_forward(int32_t K, int32_t N, int32_t ld, int32_t M, const float* coef, const float* table,
                           const int32_t* cols, const int32_t* inv, const float* base, float* out, float* out_masked,
                           void* stream) {
    if (int rc = blend_check_shape(K, N, ld, M)) return rc;
    if (M == 0) return 0;
    if (!coef || !inv || !out) return fail(EXA_MESH_E_NULLPTR, "coef / inv / out is NULL");
    if (N > 0 && (!table || !cols)) return fail(EXA_MESH_E_NULLPTR, "table / cols is NULL");
    if ((uintptr_t)table & 15) return fail(EXA_MESH_E_INVALID, "table must be 16-byte aligned");
    const int tiles = (int)ceil_div(N, BL_TILE);
    const BlendFwdParams P = {K, N, ld, M, tiles, coef, table, cols, inv, base, out, out_masked};
    hipLaunchKernelGGL(blend_fwd, dim3(tiles + ceil_div(M, BL_FILL)), dim3(BL_BLOCK), 0, (hipStream_t)stream, P);
    return launched("blend_fwd");
}

int exa_mesh_blend_workspace_size(int32_t K, int32_t N, uint64_t* out_bytes) {
    if (!out_bytes) return fail(EXA_MESH_E_NULLPTR, "out_bytes is NULL");
    if (N < 0) return fail(EXA_MESH_E_INVALID, "negative size");
    if (K < 1 || K > BL_MAXK) return fail(EXA_MESH_E_INVALID, "K (blend coefficients) must be 1 .. 512");
    if ((int64_t)N > BL_MAX_OUT) return fail(EXA_MESH_E_INVALID, "N (compact columns) exceeds 2^30");
    *out_bytes = blend_workspace_bytes(K, N);
    return 0;
}

int exa_mesh_blend_backward(int32_t K, int32_t N, int32_t ld, int32_t M, const float* table, const int32_t* cols,
                            const int32_t* inv, const float* g_out, const float* g_masked, void* ws, uint64_t ws_bytes,
                            float* dL_dcoef, float* dL_dbase, void* stream) {
    if (int rc = blend_check_shape(K, N, ld, M)) return rc;
    if (!dL_dcoef && !dL_dbase) return 0;
    if (dL_dbase && M > 0 && !inv) return fail(EXA_MESH_E_NULLPTR, "inv is NULL");
    const int chunks = dL_dcoef ? (int)ceil_div(N, BLB_CHUNK) : 0;
    if (chunks > 0) {
        if (!table || !cols || !g_out) return fail(EXA_MESH_E_NULLPTR, "table / cols / g_out is NULL");
        if ((uintptr_t)table & 15) return fail(EXA_MESH_E_INVALID, "table must be 16-byte aligned");
        if (!ws) return fail(EXA_MESH_E_NULLPTR, "ws (workspace) is NULL");
        if (ws_bytes < blend_workspace_bytes(K, N))
            return fail(EXA_MESH_E_INVALID, "workspace is smaller than exa_mesh_blend_workspace_size");
    }
    const BlendBwdParams P = {K, N, ld, M, chunks, table, cols, inv, g_out, g_masked, (float*)ws, dL_dcoef, dL_dbase};
    hipStream_t st = (hipStream_t)stream;
    if (chunks > 0) {
        hipLaunchKernelGGL(blend_bwd_partial, dim3(chunks, ceil_div(K, BLB_ROWS)), dim3(BLB_BLOCK), 0, st, P);
        if (int rc = launched("blend_bwd_partial")) return rc;
    }
    const unsigned blocks = (dL_dcoef ? ceil_div(K, BLB_BLOCK) : 0) + (dL_dbase ? ceil_div(M, 4 * BLB_BLOCK) : 0);
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(blend_bwd_finish, dim3(blocks), dim3(BLB_BLOCK), 0, st, P);
    return launched("blend_bwd_finish");
}

}  // extern "C"
