// Linear blend skinning (include/exa_skin.h): the per-vertex transforms of ExAvatar's get_transform_mat_vertex, the
// two lbs calls and the camera -> world step (reference module.py:413-422, 548-556), and an atomic-free backward.  The
// semantics -- the op-by-op fp32 forward and the backward's two-level summation order -- are written out in the header;
// this file implements them.
//
//   skin_fwd        one wave per 64 vertices.  T's rows 0-2 sit in LDS; the wave stages its 64 gathered weight rows in
//                   LDS with one coalesced row load per instruction (lane l loads weight l), then every lane blends its
//                   vertex's A (12 accumulators, j ascending) and applies it to each set.
//   skin_bwd_chunk  one workgroup of 256 threads per chunk of EXA_SKIN_CHUNK vertices, walked in four sub-chunks of 64:
//                   stage the sub-chunk's weight rows, three waves blend one row of A each, wave 0 forms g', the point
//                   gradients and G_v of its vertex, then every thread adds the sub-chunk's vertices, in ascending order,
//                   into its outputs (12 J + 3 chunk partials in all, at most four per thread, kept in registers across
//                   the sub-chunks).  The partials go to the workspace, each written by exactly one thread.
//   skin_bwd_sum    one workgroup per 64 outputs of [grad_T | grad_trans]: tiles of 128 chunk partials are loaded into
//                   LDS by all four waves, then one thread per output adds them in chunk order.  Row 3 of grad_T is
//                   written as +0.
// No atomics, no memsets: every output element is one thread's sum in the header's order.
// Compiled with -ffp-contract=off (build.py): the products must not be contracted into fused multiply-adds.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/exa_skin.h"
#include "abi_status.h"

namespace exa_skin_impl {

using exa::ceil_div;

constexpr int MAXJ = EXA_SKIN_MAX_JOINTS;
constexpr int MAXS = EXA_SKIN_MAX_SETS;
constexpr int CHUNK = EXA_SKIN_CHUNK;
constexpr int SUB = 64;                       // vertices per staged sub-chunk (one wave's worth)
constexpr int LDW = MAXJ + 1;                 // LDS row stride of the staged weights (odd: lane-per-vertex reads do not
                                              // share a bank)
constexpr int BWD_BLOCK = 256;
constexpr int OUT_PER_THREAD = (12 * MAXJ + 3 + BWD_BLOCK - 1) / BWD_BLOCK;
constexpr int SUM_BLOCK = 256;
constexpr int SUM_COLS = 64;                  // outputs per workgroup of skin_bwd_sum
constexpr int SUM_TILE = 128;                 // chunk partials per LDS tile
static_assert(CHUNK % SUB == 0, "a chunk is a whole number of sub-chunks");
static_assert(SUM_TILE % (SUM_BLOCK / SUM_COLS) == 0, "the tile loads cover the tile");

struct Common {
    int32_t V, S, J, Vw;
    const float* pts[MAXS];
    const float* W;
    const int64_t* idx;
    const float* T;
    const float* Rinv;                        // NULL: no camera step
};

__device__ __forceinline__ float qnan() { return __int_as_float(0x7fc00000); }

// T's rows 0-2 into Tl[j * 12 + r * 4 + c]
__device__ __forceinline__ void stage_T(const Common& P, float* Tl, int tid, int nthreads) {
    for (int q = tid; q < P.J * 12; q += nthreads) {
        const int j = q / 12, rc = q - j * 12;
        Tl[q] = P.T[j * 16 + rc];
    }
}

// The weight rows of vertices v0 .. v0 + 63 into Wl[SUB][LDW].  rowl[k] is vertex v0 + k's row, or -1 when its index
// lies outside [0, Vw) (then its weights are NaN) or the vertex is past V (weights 0, never used).  The caller
// synchronises between the two halves: first `stage_row_index` by the threads k < SUB, then `stage_rows` by all waves.
__device__ __forceinline__ void stage_row_index(const Common& P, int64_t v0, int* rowl, int k) {
    const int64_t v = v0 + k;
    int row = -2;                                              // past V
    if (v < P.V) {
        const int64_t r = P.idx ? P.idx[v] : v;
        row = (r >= 0 && r < P.Vw) ? (int)r : -1;              // the guard: a row outside [0, Vw) is never read
    }
    rowl[k] = row;
}

__device__ __forceinline__ void stage_rows(const Common& P, const int* rowl, float* Wl, int wave, int nwaves, int lane) {
    for (int k = wave; k < SUB; k += nwaves) {
        const int row = rowl[k];
        if (lane < P.J) {
            float w = 0.0f;
            if (row >= 0)
                w = P.W[(int64_t)row * P.J + lane];
            else if (row == -1)
                w = qnan();
            Wl[k * LDW + lane] = w;
        }
    }
}

// g' = Rinv^T g (left to right), or g
__device__ __forceinline__ void camera_grad(const float* Rinv, float g0, float g1, float g2, float (&gp)[3]) {
    if (Rinv) {
#pragma unroll
        for (int c = 0; c < 3; ++c) gp[c] = (Rinv[0 * 3 + c] * g0 + Rinv[1 * 3 + c] * g1) + Rinv[2 * 3 + c] * g2;
    } else {
        gp[0] = g0;
        gp[1] = g1;
        gp[2] = g2;
    }
}

struct FwdParams {
    Common c;
    const float* trans;
    const float* t;
    float* out[MAXS];
};

__global__ __launch_bounds__(SUB) void skin_fwd(FwdParams P) {
    __shared__ float Tl[MAXJ * 12];
    __shared__ float Wl[SUB * LDW];
    __shared__ int rowl[SUB];
    const Common& C = P.c;
    const int lane = threadIdx.x;
    const int64_t v0 = (int64_t)blockIdx.x * SUB;
    stage_T(C, Tl, lane, SUB);
    stage_row_index(C, v0, rowl, lane);
    __syncthreads();
    stage_rows(C, rowl, Wl, 0, 1, lane);
    __syncthreads();
    const int64_t v = v0 + lane;
    if (v >= C.V) return;

    float A[12];
#pragma unroll
    for (int rc = 0; rc < 12; ++rc) A[rc] = 0.0f;
    for (int j = 0; j < C.J; ++j) {
        const float w = Wl[lane * LDW + j];
        const float4* tj = reinterpret_cast<const float4*>(Tl + j * 12);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float4 tr = tj[r];
            A[r * 4 + 0] = A[r * 4 + 0] + w * tr.x;
            A[r * 4 + 1] = A[r * 4 + 1] + w * tr.y;
            A[r * 4 + 2] = A[r * 4 + 2] + w * tr.z;
            A[r * 4 + 3] = A[r * 4 + 3] + w * tr.w;
        }
    }
    const float tr0 = P.trans[0], tr1 = P.trans[1], tr2 = P.trans[2];
    for (int s = 0; s < C.S; ++s) {
        const float* x = C.pts[s] + v * 3;
        const float x0 = x[0], x1 = x[1], x2 = x[2];
        float p[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float q = ((A[r * 4 + 0] * x0 + A[r * 4 + 1] * x1) + A[r * 4 + 2] * x2) + A[r * 4 + 3];
            p[r] = q + (r == 0 ? tr0 : r == 1 ? tr1 : tr2);
        }
        float* o = P.out[s] + v * 3;
        if (C.Rinv) {
            const float* R = C.Rinv;
            const float d0 = p[0] - P.t[0], d1 = p[1] - P.t[1], d2 = p[2] - P.t[2];
#pragma unroll
            for (int r = 0; r < 3; ++r) o[r] = (R[r * 3 + 0] * d0 + R[r * 3 + 1] * d1) + R[r * 3 + 2] * d2;
        } else {
            o[0] = p[0];
            o[1] = p[1];
            o[2] = p[2];
        }
    }
}

struct BwdParams {
    Common c;
    const float* gout[MAXS];
    float* gpts[MAXS];                        // NULL entries: that set's point gradient is not written
    float* partials;                          // [ceil(V / CHUNK)][12 J + 3]
};

__global__ __launch_bounds__(BWD_BLOCK) void skin_bwd_chunk(BwdParams P) {
    __shared__ float Tl[MAXJ * 12];
    __shared__ float Wl[SUB * LDW];
    __shared__ float Al[SUB * 12];
    __shared__ float Gl[SUB * 12];
    __shared__ int rowl[SUB];
    const Common& C = P.c;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int J = C.J, NO = 12 * J + 3;
    stage_T(C, Tl, tid, BWD_BLOCK);

    // this thread's outputs: o = tid + k * BWD_BLOCK; grad_T column (j, rc) or grad_trans row (w = 1, exact)
    int wj[OUT_PER_THREAD], gi[OUT_PER_THREAD];
    float acc[OUT_PER_THREAD];
#pragma unroll
    for (int k = 0; k < OUT_PER_THREAD; ++k) {
        const int o = tid + k * BWD_BLOCK;
        if (o < 12 * J) {
            wj[k] = o / 12;
            gi[k] = o - wj[k] * 12;
        } else {
            wj[k] = -1;                                        // grad_trans (or no output)
            gi[k] = o < NO ? (o - 12 * J) * 4 + 3 : 0;
        }
        acc[k] = 0.0f;
    }

    const int64_t c0 = (int64_t)blockIdx.x * CHUNK;
    for (int sc = 0; sc < CHUNK / SUB; ++sc) {
        const int64_t v0 = c0 + sc * SUB;
        if (v0 >= C.V) break;                                  // uniform across the workgroup
        const int nv = (int)(C.V - v0 < SUB ? C.V - v0 : SUB);
        if (tid < SUB) stage_row_index(C, v0, rowl, tid);
        __syncthreads();                                       // also orders the previous sub-chunk's reads of Wl / Gl
        stage_rows(C, rowl, Wl, wave, BWD_BLOCK / 64, lane);
        __syncthreads();

        // A, one row per wave (waves 0-2), j ascending
        if (wave < 3 && lane < nv) {
            const int r = wave;
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
            for (int j = 0; j < J; ++j) {
                const float w = Wl[lane * LDW + j];
                const float4 tr = *reinterpret_cast<const float4*>(Tl + j * 12 + r * 4);
                a0 = a0 + w * tr.x;
                a1 = a1 + w * tr.y;
                a2 = a2 + w * tr.z;
                a3 = a3 + w * tr.w;
            }
            Al[lane * 12 + r * 4 + 0] = a0;
            Al[lane * 12 + r * 4 + 1] = a1;
            Al[lane * 12 + r * 4 + 2] = a2;
            Al[lane * 12 + r * 4 + 3] = a3;
        }
        __syncthreads();

        // g', the point gradients and G_v, one lane per vertex
        if (wave == 0 && lane < nv) {
            const int64_t v = v0 + lane;
            const float* A = Al + lane * 12;
            float G[12];
#pragma unroll
            for (int q = 0; q < 12; ++q) G[q] = 0.0f;
            for (int s = 0; s < C.S; ++s) {
                const float* g = P.gout[s] + v * 3;
                float gp[3];
                camera_grad(C.Rinv, g[0], g[1], g[2], gp);
                if (float* gx = P.gpts[s]) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        gx[v * 3 + c] = (A[0 * 4 + c] * gp[0] + A[1 * 4 + c] * gp[1]) + A[2 * 4 + c] * gp[2];
                }
                const float* x = C.pts[s] + v * 3;
                const float xt[4] = {x[0], x[1], x[2], 1.0f};
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) G[r * 4 + c] = G[r * 4 + c] + gp[r] * xt[c];
            }
#pragma unroll
            for (int q = 0; q < 12; ++q) Gl[lane * 12 + q] = G[q];
        }
        __syncthreads();

        // the chunk partials: this sub-chunk's vertices in ascending order
#pragma unroll
        for (int k = 0; k < OUT_PER_THREAD; ++k) {
            if (tid + k * BWD_BLOCK >= NO) continue;
            const int j = wj[k], q = gi[k];
            float a = acc[k];
            if (j >= 0) {
                for (int u = 0; u < nv; ++u) a = a + Wl[u * LDW + j] * Gl[u * 12 + q];
            } else {
                for (int u = 0; u < nv; ++u) a = a + Gl[u * 12 + q];
            }
            acc[k] = a;
        }
    }
#pragma unroll
    for (int k = 0; k < OUT_PER_THREAD; ++k) {
        const int o = tid + k * BWD_BLOCK;
        if (o < NO) P.partials[(int64_t)blockIdx.x * NO + o] = acc[k];
    }
}

struct SumParams {
    int32_t J, nchunks;
    const float* partials;
    float* gT;                                // [J, 4, 4] or NULL
    float* gtrans;                            // [3] or NULL
};

__global__ __launch_bounds__(SUM_BLOCK) void skin_bwd_sum(SumParams P) {
    __shared__ float tile[SUM_TILE * SUM_COLS];
    const int tid = threadIdx.x, col = tid & (SUM_COLS - 1), part = tid / SUM_COLS;
    const int J = P.J, NO = 12 * J + 3, NQ = 16 * J + 3;
    const int q = blockIdx.x * SUM_COLS + col;                // output: grad_T element q < 16 J, else grad_trans
    int src = -1;                                             // partial column, -1 = row 3 of grad_T or past the end
    if (q < 16 * J) {
        const int j = q >> 4, r = (q >> 2) & 3, c = q & 3;
        if (r < 3) src = j * 12 + r * 4 + c;
    } else if (q < NQ) {
        src = 12 * J + (q - 16 * J);
    }
    float acc = 0.0f;
    for (int k0 = 0; k0 < P.nchunks; k0 += SUM_TILE) {
#pragma unroll
        for (int i = 0; i < SUM_TILE / (SUM_BLOCK / SUM_COLS); ++i) {
            const int kl = i * (SUM_BLOCK / SUM_COLS) + part;
            const int k = k0 + kl;
            tile[kl * SUM_COLS + col] = (src >= 0 && k < P.nchunks) ? P.partials[(int64_t)k * NO + src] : 0.0f;
        }
        __syncthreads();
        if (part == 0) {
            const int n = P.nchunks - k0 < SUM_TILE ? P.nchunks - k0 : SUM_TILE;
            for (int kl = 0; kl < n; ++kl) acc = acc + tile[kl * SUM_COLS + col];
        }
        __syncthreads();
    }
    if (part != 0 || q >= NQ) return;
    if (q < 16 * J) {
        if (P.gT) P.gT[q] = src >= 0 ? acc : 0.0f;
    } else if (P.gtrans) {
        P.gtrans[q - 16 * J] = acc;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

EXA_ABI_STATUS("exa_skin")

int check_shape(int32_t V, int32_t S, int32_t J, int32_t Vw, const int64_t* idx) {
    if (V < 0) return fail(EXA_SKIN_E_INVALID, "negative vertex count V");
    if (V > EXA_SKIN_MAX_POINTS) return fail(EXA_SKIN_E_INVALID, "V exceeds 2^28");
    if (S < 1 || S > EXA_SKIN_MAX_SETS) return fail(EXA_SKIN_E_INVALID, "S (point sets) must be 1 .. 4");
    if (J < 1 || J > EXA_SKIN_MAX_JOINTS) return fail(EXA_SKIN_E_INVALID, "J (joints) must be 1 .. 64");
    if (Vw < 0 || Vw > EXA_SKIN_MAX_POINTS) return fail(EXA_SKIN_E_INVALID, "Vw (weight rows) must be 0 .. 2^28");
    if (!idx && Vw != V) return fail(EXA_SKIN_E_INVALID, "without idx the weight table must have V rows");
    return 0;
}

uint64_t num_chunks(int32_t V) { return ((uint64_t)V + CHUNK - 1) / CHUNK; }

uint64_t workspace_bytes_for(int32_t V, int32_t J) { return num_chunks(V) * (uint64_t)(12 * J + 3) * sizeof(float); }

// the S device pointers of a host array, every one present; the entries past S are NULL
template <typename Ptr>
int copy_sets(const Ptr* src, int S, Ptr (&dst)[MAXS], const char* what) {
    if (!src) return fail(EXA_SKIN_E_NULLPTR, what);
    for (int s = 0; s < MAXS; ++s) {
        dst[s] = s < S ? src[s] : nullptr;
        if (s < S && !dst[s]) return fail(EXA_SKIN_E_NULLPTR, what);
    }
    return 0;
}

int check_common(int32_t V, int32_t S, int32_t J, int32_t Vw, const float* const* points, const float* weights,
                 const int64_t* idx, const float* T, const float* Rinv, Common& c) {
    c = Common{V, S, J, Vw, {}, weights, idx, T, Rinv};
    if (int rc = copy_sets(points, S, c.pts, "points (or one of its S entries) is NULL")) return rc;
    if (!weights || !T) return fail(EXA_SKIN_E_NULLPTR, "weights / T is NULL");
    return 0;
}

}  // namespace exa_skin_impl

using namespace exa_skin_impl;

extern "C" {

int exa_skin_version(void) { return EXA_SKIN_VERSION; }

const char* exa_skin_last_error(void) { return g_err; }

int exa_skin_workspace_size(int32_t V, int32_t J, uint64_t* out_bytes) {
    if (!out_bytes) return fail(EXA_SKIN_E_NULLPTR, "out_bytes is NULL");
    if (V < 0 || V > EXA_SKIN_MAX_POINTS) return fail(EXA_SKIN_E_INVALID, "V must be 0 .. 2^28");
    if (J < 1 || J > EXA_SKIN_MAX_JOINTS) return fail(EXA_SKIN_E_INVALID, "J (joints) must be 1 .. 64");
    *out_bytes = workspace_bytes_for(V, J);
    return 0;
}

int exa_skin_forward(int32_t V, int32_t S, int32_t J, int32_t Vw, const float* const* points, const float* weights,
                     const int64_t* idx, const float* T, const float* trans, const float* Rinv, const float* t,
                     float* const* out, void* stream) {
    if (int rc = check_shape(V, S, J, Vw, idx)) return rc;
    if (!Rinv != !t) return fail(EXA_SKIN_E_INVALID, "Rinv and t must be given together");
    if (V == 0) return 0;
    FwdParams P;
    if (int rc = check_common(V, S, J, Vw, points, weights, idx, T, Rinv, P.c)) return rc;
    if (!trans) return fail(EXA_SKIN_E_NULLPTR, "trans is NULL");
    if (int rc = copy_sets(out, S, P.out, "out (or one of its S entries) is NULL")) return rc;
    P.trans = trans;
    P.t = t;
    hipLaunchKernelGGL(skin_fwd, dim3(ceil_div(V, SUB)), dim3(SUB), 0, (hipStream_t)stream, P);
    return launched("skin_fwd");
}

int exa_skin_backward(int32_t V, int32_t S, int32_t J, int32_t Vw, const float* const* points, const float* weights,
                      const int64_t* idx, const float* T, const float* Rinv, const float* const* grad_out,
                      float* const* grad_points, float* grad_T, float* grad_trans, void* workspace,
                      uint64_t workspace_bytes, void* stream) {
    if (int rc = check_shape(V, S, J, Vw, idx)) return rc;
    hipStream_t st = (hipStream_t)stream;
    SumParams Q = {J, (int32_t)num_chunks(V), nullptr, grad_T, grad_trans};
    if (V > 0) {
        BwdParams P;
        if (int rc = check_common(V, S, J, Vw, points, weights, idx, T, Rinv, P.c)) return rc;
        if (int rc = copy_sets(grad_out, S, P.gout, "grad_out (or one of its S entries) is NULL")) return rc;
        for (int s = 0; s < MAXS; ++s) P.gpts[s] = (grad_points && s < S) ? grad_points[s] : nullptr;
        if (!workspace) return fail(EXA_SKIN_E_NULLPTR, "workspace is NULL");
        if (workspace_bytes < workspace_bytes_for(V, J))
            return fail(EXA_SKIN_E_INVALID, "workspace is smaller than exa_skin_workspace_size");
        P.partials = (float*)workspace;
        Q.partials = P.partials;
        hipLaunchKernelGGL(skin_bwd_chunk, dim3((unsigned)num_chunks(V)), dim3(BWD_BLOCK), 0, st, P);
        if (int rc = launched("skin_bwd_chunk")) return rc;
    }
    if (!grad_T && !grad_trans) return 0;
    hipLaunchKernelGGL(skin_bwd_sum, dim3(ceil_div(16 * J + 3, SUM_COLS)), dim3(SUM_BLOCK), 0, st, Q);
    return launched("skin_bwd_sum");
}

}  // extern "C"
