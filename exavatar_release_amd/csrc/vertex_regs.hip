// Arm and hand regularisers of the upsampled mesh (include/exa_mesh.h; the reference's ArmRGBReg, HandRGBReg and
// HandMeanReg, loss.py:148-197).  The semantics -- every operation in fp32 in a stated order -- are written out in the
// header; this file implements them.
//
//   arm_compact     ONE workgroup.  Turns the two bool masks into the upper and the lower record list {x, y, z, index}
//                   (16 bytes each, ascending vertex index), the rank of every vertex in the lower list (-1: not in it)
//                   and the two counts in the header, with a block-wide prefix sum per 16 384 vertices: no atomics, so
//                   the lists are the same on every call.
//   arm_select      one wave per lower vertex, ARM_WAVES waves per workgroup; the workgroup stages tiles of ARM_TILE upper
//                   records in LDS with 16-byte loads.  The wave keeps its 64 best keys (bits of d2, index) sorted, one
//                   per lane.  Per batch of 64 candidates it ballots those that are valid and beat the key of lane
//                   K_max - 1, and inserts them one by one in a wave-uniform loop (a lane shift and a compare).  The
//                   number of valid candidates is summed by popcount.  No per-row capacity, no fallback, whatever U is.
//                   Writes the first K_max keys' indices, the count, and the minimum count of the workgroup's rows.
//   arm_finish      ONE workgroup: the minimum of those minima, k = min(K_max, n_min) into the header.
//   arm_loss_fwd    one thread per (b, v): +0 outside the lower list, else the target (k rows summed in key order), d, loss.
//   arm_loss_bwd    one thread per (b, v): +0 outside the lower list, else (2 d) g.
//   hand_partial    one workgroup per (hand, b, chunk of 256 list rows): the rows are gathered into LDS in parallel, then
//                   three threads (one per channel) add them up sequentially from +0.
//   hand_rgb_fwd    every workgroup adds the chunk partials up sequentially, divides, and writes 256 rows of the loss.
//   hand_rgb_bwd    one thread per (b, v), through the inverse ranks: right term, then left term.
//   hand_mean_fwd / hand_mean_bwd   one thread per (b, hand row) / per (b, v).
// No atomics, no memsets, no allocation, no synchronisation: every output element is one thread's value in the
// header's order.  Compiled with -ffp-contract=off (build.py): no product is contracted into a fused multiply-add.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/exa_mesh.h"
#include "abi_status.h"

namespace exa_mesh_impl {

using exa::align256;
using exa::ceil_div;

EXA_ABI_STATUS_SHARED("exa_mesh")         // exa_mesh_last_error() and its buffer are mesh_raster.hip's

constexpr int ARM_MAXK = EXA_MESH_ARM_MAX_K;
constexpr int ARM_WAVES = EXA_MESH_ARM_WAVES;
constexpr int ARM_TILE = EXA_MESH_ARM_TILE;
constexpr int ARM_SEL_THREADS = ARM_WAVES * 64;
constexpr int CMP_THREADS = 1024;
constexpr int CMP_WAVES = CMP_THREADS / 64;
constexpr int CMP_PER = 16;                   // consecutive vertices per thread and pass
constexpr int REG_BLOCK = 256;
constexpr int REG_CHUNK = EXA_MESH_REG_CHUNK;
constexpr int REG_MAX_BATCH = 65535;          // B is a grid dimension
constexpr int64_t REG_MAX_ELEMS = 1 << 30;    // B * V * 3
constexpr int32_t REG_MAX_VERTS = 1 << 26;
static_assert(ARM_MAXK == 64, "one key per lane of a wave");
static_assert(REG_CHUNK == REG_BLOCK, "hand_partial: one thread per row of a chunk");
static_assert(ARM_TILE % 64 == 0 && ARM_TILE % ARM_SEL_THREADS == 0, "whole batches, whole staging passes");

__device__ __forceinline__ float reg_qnan() { return __int_as_float(0x7fc00000); }

// ---- arm: compaction ----------------------------------------------------------------------------------------------------
struct ArmCompactParams {
    int32_t V;
    const float* mesh;
    const uint8_t* is_upper;
    const uint8_t* is_lower;
    float4* upper_rec;
    float4* lower_rec;
    int32_t* lower_rank;
    int32_t* header;
};

__global__ __launch_bounds__(CMP_THREADS) void arm_compact(ArmCompactParams P) {
    __shared__ int wtot_u[CMP_WAVES], wtot_l[CMP_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t V = P.V;
    int base_u = 0, base_l = 0;
    for (int64_t v0 = 0; v0 < V; v0 += CMP_THREADS * CMP_PER) {
        const int64_t s = v0 + (int64_t)tid * CMP_PER;
        uint32_t mu = 0, ml = 0;
        for (int i = 0; i < CMP_PER; ++i) {
            if (s + i < V) {
                mu |= (uint32_t)(P.is_upper[s + i] != 0) << i;
                ml |= (uint32_t)(P.is_lower[s + i] != 0) << i;
            }
        }
        const int cu = __popc(mu), cl = __popc(ml);
        int su = cu, sl = cl;                                  // inclusive scan over the wave
        for (int off = 1; off < 64; off <<= 1) {
            const int tu = __shfl_up(su, off, 64), tl = __shfl_up(sl, off, 64);
            if (lane >= off) {
                su += tu;
                sl += tl;
            }
        }
        if (lane == 63) {
            wtot_u[wave] = su;
            wtot_l[wave] = sl;
        }
        __syncthreads();
        int before_u = 0, before_l = 0, tot_u = 0, tot_l = 0;
        for (int w = 0; w < CMP_WAVES; ++w) {
            if (w < wave) {
                before_u += wtot_u[w];
                before_l += wtot_l[w];
            }
            tot_u += wtot_u[w];
            tot_l += wtot_l[w];
        }
        int pu = base_u + before_u + su - cu, pl = base_l + before_l + sl - cl;
        for (int i = 0; i < CMP_PER; ++i) {
            const int64_t v = s + i;
            if (v >= V) break;
            const bool up = (mu >> i) & 1, lo = (ml >> i) & 1;
            if (up || lo) {
                const float4 r = make_float4(P.mesh[v * 3], P.mesh[v * 3 + 1], P.mesh[v * 3 + 2], __int_as_float((int)v));
                if (up) P.upper_rec[pu++] = r;                 // pu, pl <= v < V: inside the [V] lists
                if (lo) P.lower_rec[pl] = r;
            }
            P.lower_rank[v] = lo ? pl++ : -1;
        }
        base_u += tot_u;
        base_l += tot_l;
        __syncthreads();                                       // the totals are read before the next pass overwrites them
    }
    if (tid == 0) {
        P.header[0] = base_u;
        P.header[1] = base_l;
    }
}

// ---- arm: selection -----------------------------------------------------------------------------------------------------
struct ArmSelectParams {
    int32_t rows, K;
    float thr;
    const float4* upper_rec;
    const float4* lower_rec;
    const int32_t* header;
    int32_t* nbr;
    int32_t* n_valid;
    int32_t* wg_min;
};

constexpr unsigned long long ARM_EMPTY = ~0ull;

__global__ __launch_bounds__(ARM_SEL_THREADS) void arm_select(ArmSelectParams P) {
    __shared__ float4 tile[ARM_TILE];
    __shared__ int wn[ARM_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int U = P.header[0];
    const int L = min(P.header[1], P.rows);
    const int row0 = blockIdx.x * ARM_WAVES;
    if (row0 >= L) return;                                     // the whole workgroup: rows beyond the device-side L
    const int row = row0 + wave;
    const bool active = row < L;                               // wave-uniform
    const float4 me = active ? P.lower_rec[row] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int worst_lane = P.K - 1;
    unsigned long long key = ARM_EMPTY;                        // lane i: the i-th smallest key so far
    int n = 0;
    for (int u0 = 0; u0 < U; u0 += ARM_TILE) {
        __syncthreads();
        for (int i = tid; i < ARM_TILE; i += ARM_SEL_THREADS)
            if (u0 + i < U) tile[i] = P.upper_rec[u0 + i];
        __syncthreads();
        if (!active) continue;
        const int cnt = min(ARM_TILE, U - u0);
        for (int c0 = 0; c0 < cnt; c0 += 64) {
            const int j = c0 + lane;
            const bool in = j < cnt;
            const float4 r = tile[in ? j : c0];                // c0 < cnt: a staged record
            const float dx = me.x - r.x, dy = me.y - r.y, dz = me.z - r.z;
            const bool valid = in && fabsf(dx) < P.thr;
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            const uint32_t bits = d2 != d2 ? 0x7fc00000u : (uint32_t)__float_as_int(d2);
            const unsigned long long cand = ((unsigned long long)bits << 32) | (uint32_t)__float_as_int(r.w);
            n += __popcll(__ballot(valid));
            unsigned long long worst = __shfl(key, worst_lane, 64);
            unsigned long long m = __ballot(valid && cand < worst);
            while (m) {                                        // wave-uniform
                const int src = __ffsll((long long)m) - 1;
                m &= m - 1;
                const unsigned long long c = __shfl(cand, src, 64);
                if (c >= worst) continue;
                const unsigned long long prev = __shfl_up(key, 1, 64);
                if (key > c) key = (lane > 0 && prev > c) ? prev : c;
                worst = __shfl(key, worst_lane, 64);
            }
        }
    }
    if (active) {
        if (lane < P.K) P.nbr[(int64_t)row * P.K + lane] = key == ARM_EMPTY ? -1 : (int32_t)(uint32_t)key;
        if (lane == 0) P.n_valid[row] = n;
    }
    if (lane == 0) wn[wave] = active ? n : INT_MAX;
    __syncthreads();
    if (tid == 0) {
        int mn = wn[0];
        for (int w = 1; w < ARM_WAVES; ++w) mn = min(mn, wn[w]);
        P.wg_min[blockIdx.x] = mn;
    }
}

__global__ __launch_bounds__(REG_BLOCK) void arm_finish(int32_t rows, int32_t K, const int32_t* wg_min, int32_t* header) {
    __shared__ int part[REG_BLOCK];
    const int tid = threadIdx.x;
    const int L = min(header[1], rows);
    const int groups = (L + ARM_WAVES - 1) / ARM_WAVES;
    int mn = INT_MAX;
    for (int i = tid; i < groups; i += REG_BLOCK) mn = min(mn, wg_min[i]);
    part[tid] = mn;
    __syncthreads();
    for (int s = REG_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) part[tid] = min(part[tid], part[tid + s]);
        __syncthreads();
    }
    if (tid == 0) {
        const int n_min = L > 0 ? part[0] : 0;
        header[2] = min(K, n_min);
        header[3] = n_min;
    }
}

// ---- arm: loss ----------------------------------------------------------------------------------------------------------
struct ArmLossParams {
    int32_t B, V, rows, K;
    const float* rgb;
    const int32_t* lower_rank;
    const int32_t* nbr;
    const int32_t* header;
    float* loss;
    float* d;
};

__global__ __launch_bounds__(REG_BLOCK) void arm_loss_fwd(ArmLossParams P) {
    const int64_t i = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x;
    if (i >= (int64_t)P.B * P.V) return;
    const int V = P.V;
    const int v = (int)(i % V);
    const int r = P.lower_rank[v];
    float* loss = P.loss + i * 3;
    float* d = P.d + i * 3;
    if (r < 0) {
        for (int c = 0; c < 3; ++c) loss[c] = d[c] = 0.0f;
        return;
    }
    const float* x = P.rgb + (i - v) * 3;                      // this batch element's [V, 3]
    float t[3] = {0.0f, 0.0f, 0.0f};
    const int k = min(P.header[2], P.K);
    if (r < P.rows) {
        const int32_t* list = P.nbr + (int64_t)r * P.K;
        for (int j = 0; j < k; ++j) {
            const int u = list[j];
            if ((unsigned)u < (unsigned)V) {                   // the guard: a row outside [0, V) is never read
                for (int c = 0; c < 3; ++c) t[c] = t[c] + x[(int64_t)u * 3 + c];
            } else {
                for (int c = 0; c < 3; ++c) t[c] = reg_qnan();
            }
        }
    } else {
        for (int c = 0; c < 3; ++c) t[c] = reg_qnan();         // a lower vertex beyond the caller's row capacity
    }
    const float fk = (float)k;
    for (int c = 0; c < 3; ++c) {
        const float target = t[c] / fk;                        // k == 0: 0 / 0 = NaN, the reference's empty mean
        const float dd = x[(int64_t)v * 3 + c] - target;
        d[c] = dd;
        loss[c] = dd * dd;
    }
}

__global__ __launch_bounds__(REG_BLOCK) void arm_loss_bwd(int32_t B, int32_t V, const float* d, const float* grad_loss,
                                                          const int32_t* lower_rank, float* grad_rgb) {
    const int64_t i = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x;
    if (i >= (int64_t)B * V) return;
    const bool lower = lower_rank[(int)(i % V)] >= 0;
    for (int c = 0; c < 3; ++c) grad_rgb[i * 3 + c] = lower ? (2.0f * d[i * 3 + c]) * grad_loss[i * 3 + c] : 0.0f;
}

// ---- hand rgb -----------------------------------------------------------------------------------------------------------
struct HandRgbParams {
    int32_t B, V, N, chunks;
    const float* rgb;
    const int32_t* r_idx;
    const int32_t* l_idx;
    const int32_t* r_rank;
    const int32_t* l_rank;
    const float* grad_loss;
    float* partials;                          // [2, B, chunks, 3]
    float* means;                             // [B, 2, 3]
    float* loss;                              // [B, N, 3]
    float* grad_rgb;                          // [B, V, 3]
};

__device__ __forceinline__ float hand_row(const float* x, int v, int V, int c) {
    return (unsigned)v < (unsigned)V ? x[(int64_t)v * 3 + c] : reg_qnan();       // the guard, as above
}

__global__ __launch_bounds__(REG_BLOCK) void hand_partial(HandRgbParams P) {
    __shared__ float rows[REG_CHUNK * 3];
    const int tid = threadIdx.x, chunk = blockIdx.x, b = blockIdx.y, hand = blockIdx.z;
    const int32_t* idx = hand ? P.l_idx : P.r_idx;
    const float* x = P.rgb + (int64_t)b * P.V * 3;
    const int j = chunk * REG_CHUNK + tid;
    if (j < P.N) {
        const int v = idx[j];
        for (int c = 0; c < 3; ++c) rows[tid * 3 + c] = hand_row(x, v, P.V, c);
    }
    __syncthreads();
    if (tid < 3) {
        const int cnt = min(REG_CHUNK, P.N - chunk * REG_CHUNK);
        float acc = 0.0f;
        for (int t = 0; t < cnt; ++t) acc = acc + rows[t * 3 + tid];
        P.partials[(((int64_t)hand * P.B + b) * P.chunks + chunk) * 3 + tid] = acc;
    }
}

__global__ __launch_bounds__(REG_BLOCK) void hand_rgb_fwd(HandRgbParams P) {
    __shared__ float mean[6];
    const int tid = threadIdx.x, b = blockIdx.y;
    if (tid < 6) {
        const int hand = tid / 3, c = tid % 3;
        const float* p = P.partials + ((int64_t)hand * P.B + b) * P.chunks * 3;
        float acc = 0.0f;
        for (int ch = 0; ch < P.chunks; ++ch) acc = acc + p[ch * 3 + c];
        const float m = acc / (float)P.N;
        mean[tid] = m;
        if (blockIdx.x == 0) P.means[b * 6 + tid] = m;
    }
    __syncthreads();
    const int j = blockIdx.x * REG_BLOCK + tid;
    if (j >= P.N) return;
    const float* x = P.rgb + (int64_t)b * P.V * 3;
    const int vr = P.r_idx[j], vl = P.l_idx[j];
    for (int c = 0; c < 3; ++c) {
        const float dr = hand_row(x, vr, P.V, c) - mean[c];
        const float dl = hand_row(x, vl, P.V, c) - mean[3 + c];
        P.loss[((int64_t)b * P.N + j) * 3 + c] = dr * dr + dl * dl;
    }
}

__global__ __launch_bounds__(REG_BLOCK) void hand_rgb_bwd(HandRgbParams P) {
    const int64_t i = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x;
    if (i >= (int64_t)P.B * P.V) return;
    const int v = (int)(i % P.V), b = (int)(i / P.V);
    const int ir = P.r_rank[v], il = P.l_rank[v];
    const bool in_r = (unsigned)ir < (unsigned)P.N, in_l = (unsigned)il < (unsigned)P.N;
    for (int c = 0; c < 3; ++c) {
        const float x = P.rgb[i * 3 + c];
        float tr = 0.0f, tl = 0.0f;
        if (in_r) tr = P.grad_loss[((int64_t)b * P.N + ir) * 3 + c] * (2.0f * (x - P.means[b * 6 + c]));
        if (in_l) tl = P.grad_loss[((int64_t)b * P.N + il) * 3 + c] * (2.0f * (x - P.means[b * 6 + 3 + c]));
        P.grad_rgb[i * 3 + c] = in_r && in_l ? tr + tl : in_r ? tr : in_l ? tl : 0.0f;
    }
}

// ---- hand mean ----------------------------------------------------------------------------------------------------------
struct HandMeanParams {
    int32_t B, V, H;
    const float* offset;                      // [B, V, 3]
    const float* normal;                      // [V, 3]
    const int32_t* h_idx;                     // [H]
    const int32_t* h_rank;                    // [V]
    const float* grad_loss;                   // [B, H]
    float* loss;                              // [B, H]
    float* grad_offset;                       // [B, V, 3]
};

constexpr float HAND_EPS = 1e-12f;            // F.normalize's eps

// norm, s = max(norm, eps), q = o / s and dot = (n0 q0 + n1 q1) + n2 q2 of one row
__device__ __forceinline__ float hand_dot(const float* o, const float* nv, float& norm, float& s, float (&q)[3]) {
    norm = sqrtf((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]);
    s = norm < HAND_EPS ? HAND_EPS : norm;                     // a NaN norm stays NaN, as clamp_min keeps it
    for (int c = 0; c < 3; ++c) q[c] = o[c] / s;
    return (nv[0] * q[0] + nv[1] * q[1]) + nv[2] * q[2];
}

__global__ __launch_bounds__(REG_BLOCK) void hand_mean_fwd(HandMeanParams P) {
    const int64_t i = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x;
    if (i >= (int64_t)P.B * P.H) return;
    const int j = (int)(i % P.H), b = (int)(i / P.H);
    const int v = P.h_idx[j];
    if ((unsigned)v >= (unsigned)P.V) {                        // the guard, as above
        P.loss[i] = reg_qnan();
        return;
    }
    float norm, s, q[3];
    const float dot = hand_dot(P.offset + ((int64_t)b * P.V + v) * 3, P.normal + (int64_t)v * 3, norm, s, q);
    P.loss[i] = dot < 0.0f ? 0.0f : dot;                       // a NaN dot stays NaN, as clamp keeps it
}

__global__ __launch_bounds__(REG_BLOCK) void hand_mean_bwd(HandMeanParams P) {
    const int64_t i = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x;
    if (i >= (int64_t)P.B * P.V) return;
    const int v = (int)(i % P.V), b = (int)(i / P.V);
    const int j = P.h_rank[v];
    float* out = P.grad_offset + i * 3;
    if ((unsigned)j >= (unsigned)P.H) {
        for (int c = 0; c < 3; ++c) out[c] = 0.0f;
        return;
    }
    const float* o = P.offset + i * 3;
    const float* nv = P.normal + (int64_t)v * 3;
    float norm, s, q[3];
    const float dot = hand_dot(o, nv, norm, s, q);
    const float g = dot >= 0.0f ? P.grad_loss[(int64_t)b * P.H + j] : 0.0f;     // clamp(min=0) passes at equality
    float dq[3], a[3];
    for (int c = 0; c < 3; ++c) {
        dq[c] = g * nv[c];
        a[c] = dq[c] / s;
    }
    if (norm >= HAND_EPS) {                                    // clamp_min passes the gradient to the norm
        const float t = (dq[0] * (q[0] / s) + dq[1] * (q[1] / s)) + dq[2] * (q[2] / s);
        const float w = (-t) / norm;
        for (int c = 0; c < 3; ++c) out[c] = a[c] + o[c] * w;
    } else {
        for (int c = 0; c < 3; ++c) out[c] = a[c];
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
int reg_check_shape(int32_t B, int32_t V) {
    if (B < 0 || V < 0) return fail(EXA_MESH_E_INVALID, "negative size");
    if (V > REG_MAX_VERTS) return fail(EXA_MESH_E_INVALID, "V exceeds 2^26");
    if (B > REG_MAX_BATCH) return fail(EXA_MESH_E_INVALID, "B exceeds 65535");
    if ((int64_t)B * V * 3 > REG_MAX_ELEMS) return fail(EXA_MESH_E_INVALID, "B * V * 3 exceeds 2^30");
    return 0;
}

int arm_check_rows(int32_t V, int32_t rows, int32_t K) {
    if (rows < 0 || rows > V) return fail(EXA_MESH_E_INVALID, "rows (lower-arm row capacity) must be 0 .. V");
    if (K < 1 || K > ARM_MAXK) return fail(EXA_MESH_E_INVALID, "K_max must be 1 .. 64");
    return 0;
}

uint64_t hand_rgb_ws_bytes(int32_t B, int32_t N) {
    return align256((uint64_t)2 * B * ceil_div(N, REG_CHUNK) * 3 * sizeof(float));
}

}  // namespace exa_mesh_impl

using namespace exa_mesh_impl;

extern "C" {

int exa_mesh_arm_plan(int32_t V, int32_t rows, int32_t K_max, float dist_x_thr, const float* mesh,
                      const uint8_t* is_upper, const uint8_t* is_lower, float* upper_rec, float* lower_rec,
                      int32_t* lower_rank, int32_t* nbr, int32_t* n_valid, int32_t* wg_min, int32_t* header,
                      void* stream) {
    if (int rc = reg_check_shape(1, V)) return rc;
    if (int rc = arm_check_rows(V, rows, K_max)) return rc;
    if (!(dist_x_thr > 0.0f) || isinf(dist_x_thr)) return fail(EXA_MESH_E_INVALID, "dist_x_thr must be finite and > 0");
    if (!header) return fail(EXA_MESH_E_NULLPTR, "header is NULL");
    if (V > 0 && (!mesh || !is_upper || !is_lower || !upper_rec || !lower_rec || !lower_rank))
        return fail(EXA_MESH_E_NULLPTR, "mesh / is_upper / is_lower / upper_rec / lower_rec / lower_rank is NULL");
    if (rows > 0 && (!nbr || !n_valid || !wg_min)) return fail(EXA_MESH_E_NULLPTR, "nbr / n_valid / wg_min is NULL");
    hipStream_t st = (hipStream_t)stream;
    const ArmCompactParams C = {V, mesh, is_upper, is_lower, (float4*)upper_rec, (float4*)lower_rec, lower_rank, header};
    hipLaunchKernelGGL(arm_compact, dim3(1), dim3(CMP_THREADS), 0, st, C);
    if (int rc = launched("arm_compact")) return rc;
    if (rows > 0) {
        const ArmSelectParams S = {rows,    K_max,   dist_x_thr, (const float4*)upper_rec, (const float4*)lower_rec,
                                   header,  nbr,     n_valid,    wg_min};
        hipLaunchKernelGGL(arm_select, dim3(ceil_div(rows, ARM_WAVES)), dim3(ARM_SEL_THREADS), 0, st, S);
        if (int rc = launched("arm_select")) return rc;
    }
    hipLaunchKernelGGL(arm_finish, dim3(1), dim3(REG_BLOCK), 0, st, rows, K_max, (const int32_t*)wg_min, header);
    return launched("arm_finish");
}

int exa_mesh_arm_loss_forward(int32_t B, int32_t V, int32_t rows, int32_t K_max, const float* rgb,
                              const int32_t* lower_rank, const int32_t* nbr, const int32_t* header, float* loss, float* d,
                              void* stream) {
    if (int rc = reg_check_shape(B, V)) return rc;
    if (int rc = arm_check_rows(V, rows, K_max)) return rc;
    if (B == 0 || V == 0) return 0;
    if (!rgb || !lower_rank || !header) return fail(EXA_MESH_E_NULLPTR, "rgb / lower_rank / header is NULL");
    if (rows > 0 && !nbr) return fail(EXA_MESH_E_NULLPTR, "nbr is NULL");
    if (!loss || !d) return fail(EXA_MESH_E_NULLPTR, "loss / d is NULL");
    const ArmLossParams P = {B, V, rows, K_max, rgb, lower_rank, nbr, header, loss, d};
    hipLaunchKernelGGL(arm_loss_fwd, dim3(ceil_div((int64_t)B * V, REG_BLOCK)), dim3(REG_BLOCK), 0, (hipStream_t)stream, P);
    return launched("arm_loss_fwd");
}

int exa_mesh_arm_loss_backward(int32_t B, int32_t V, const float* d, const float* grad_loss, const int32_t* lower_rank,
                               float* dL_drgb, void* stream) {
    if (int rc = reg_check_shape(B, V)) return rc;
    if (B == 0 || V == 0) return 0;
    if (!d || !grad_loss || !lower_rank || !dL_drgb) return fail(EXA_MESH_E_NULLPTR, "d / grad_loss / lower_rank / dL_drgb is NULL");
    hipLaunchKernelGGL(arm_loss_bwd, dim3(ceil_div((int64_t)B * V, REG_BLOCK)), dim3(REG_BLOCK), 0, (hipStream_t)stream, B, V,
                       d, grad_loss, lower_rank, dL_drgb);
    return launched("arm_loss_bwd");
}

int exa_mesh_hand_rgb_workspace_size(int32_t B, int32_t N, uint64_t* out_bytes) {
    if (!out_bytes) return fail(EXA_MESH_E_NULLPTR, "out_bytes is NULL");
    if (B < 0 || N < 0) return fail(EXA_MESH_E_INVALID, "negative size");
    if (B > REG_MAX_BATCH || N > REG_MAX_VERTS) return fail(EXA_MESH_E_INVALID, "B exceeds 65535 or N exceeds 2^26");
    *out_bytes = hand_rgb_ws_bytes(B, N);
    return 0;
}

int exa_mesh_hand_rgb_forward(int32_t B, int32_t V, int32_t N, const float* rgb, const int32_t* r_idx,
                              const int32_t* l_idx, void* ws, uint64_t ws_bytes, float* means, float* loss, void* stream) {
    if (int rc = reg_check_shape(B, V)) return rc;
    if (N < 0 || N > V) return fail(EXA_MESH_E_INVALID, "N (vertices per hand) must be 0 .. V");
    if (B == 0 || N == 0) return 0;
    if (!rgb || !r_idx || !l_idx) return fail(EXA_MESH_E_NULLPTR, "rgb / r_idx / l_idx is NULL");
    if (!means || !loss) return fail(EXA_MESH_E_NULLPTR, "means / loss is NULL");
    if (!ws) return fail(EXA_MESH_E_NULLPTR, "ws (workspace) is NULL");
    if (ws_bytes < hand_rgb_ws_bytes(B, N))
        return fail(EXA_MESH_E_INVALID, "workspace is smaller than exa_mesh_hand_rgb_workspace_size");
    const int chunks = (int)ceil_div(N, REG_CHUNK);
    const HandRgbParams P = {B, V, N, chunks, rgb, r_idx, l_idx, nullptr, nullptr, nullptr, (float*)ws, means, loss, nullptr};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(hand_partial, dim3(chunks, B, 2), dim3(REG_BLOCK), 0, st, P);
    if (int rc = launched("hand_partial")) return rc;
    hipLaunchKernelGGL(hand_rgb_fwd, dim3(chunks, B), dim3(REG_BLOCK), 0, st, P);
    return launched("hand_rgb_fwd");
}

int exa_mesh_hand_rgb_backward(int32_t B, int32_t V, int32_t N, const float* rgb, const float* means,
                               const float* grad_loss, const int32_t* r_rank, const int32_t* l_rank, float* dL_drgb,
                               void* stream) {
    if (int rc = reg_check_shape(B, V)) return rc;
    if (N < 0 || N > V) return fail(EXA_MESH_E_INVALID, "N (vertices per hand) must be 0 .. V");
    if (B == 0 || V == 0) return 0;
    if (!rgb || !r_rank || !l_rank || !dL_drgb) return fail(EXA_MESH_E_NULLPTR, "rgb / r_rank / l_rank / dL_drgb is NULL");
    if (N > 0 && (!means || !grad_loss)) return fail(EXA_MESH_E_NULLPTR, "means / grad_loss is NULL");
    const HandRgbParams P = {B, V, N, 0, rgb, nullptr, nullptr, r_rank, l_rank, grad_loss, nullptr, (float*)means, nullptr, dL_drgb};
    hipLaunchKernelGGL(hand_rgb_bwd, dim3(ceil_div((int64_t)B * V, REG_BLOCK)), dim3(REG_BLOCK), 0, (hipStream_t)stream, P);
    return launched("hand_rgb_bwd");
}

int exa_mesh_hand_mean_forward(int32_t B, int32_t V, int32_t H, const float* offset, const float* normal,
                               const int32_t* h_idx, float* loss, void* stream) {
    if (int rc = reg_check_shape(B, V)) return rc;
    if (H < 0 || H > V) return fail(EXA_MESH_E_INVALID, "H (hand vertices) must be 0 .. V");
    if (B == 0 || H == 0) return 0;
    if (!offset || !normal || !h_idx || !loss) return fail(EXA_MESH_E_NULLPTR, "offset / normal / h_idx / loss is NULL");
    const HandMeanParams P = {B, V, H, offset, normal, h_idx, nullptr, nullptr, loss, nullptr};
    hipLaunchKernelGGL(hand_mean_fwd, dim3(ceil_div((int64_t)B * H, REG_BLOCK)), dim3(REG_BLOCK), 0, (hipStream_t)stream, P);
    return launched("hand_mean_fwd");
}

int exa_mesh_hand_mean_backward(int32_t B, int32_t V, int32_t H, const float* offset, const float* normal,
                                const float* grad_loss, const int32_t* h_rank, float* dL_doffset, void* stream) {
    if (int rc = reg_check_shape(B, V)) return rc;
    if (H < 0 || H > V) return fail(EXA_MESH_E_INVALID, "H (hand vertices) must be 0 .. V");
    if (B == 0 || V == 0) return 0;
    if (!offset || !normal || !h_rank || !dL_doffset) return fail(EXA_MESH_E_NULLPTR, "offset / normal / h_rank / dL_doffset is NULL");
    if (H > 0 && !grad_loss) return fail(EXA_MESH_E_NULLPTR, "grad_loss is NULL");
    const HandMeanParams P = {B, V, H, offset, normal, nullptr, h_rank, grad_loss, nullptr, dL_doffset};
    hipLaunchKernelGGL(hand_mean_bwd, dim3(ceil_div((int64_t)B * V, REG_BLOCK)), dim3(REG_BLOCK), 0, (hipStream_t)stream, P);
    return launched("hand_mean_bwd");
}

}  // extern "C"
