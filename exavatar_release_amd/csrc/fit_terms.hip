// The mesh terms of the fitting loss (include/exa_mesh.h; the reference's EdgeLengthLoss, FaceOffsetSymmetricReg and
// PoseLoss, fitting/common/nets/loss.py:73-87, 125-167, and the centred vertex-to-vertex term, fitting/main/model.py:235-237).
// The semantics -- every operation in fp32 in a stated order -- are written out in the header; this file implements them.
//
//   edge_fwd          one thread per (b, face): the three edge lengths of both meshes, three loss elements.
//   edge_bwd          one thread per (b, vertex): walks the vertex's (face, corner) slots of the transposed CSR in order
//                     and recomputes the two edges of each slot, so nothing is scattered and nothing staged.
//   sym_fwd           one thread per (b, face row): three taps, the flipped offset, the row's loss.
//   sym_bwd           one thread per (b, face row): its own three sign terms, then the rows that tap it, in CSR order,
//                     each with its flipped offset recomputed.
//   pose_fwd / _bwd   one thread per rotation; the quaternion route and its Jacobian are axis_angle.h (the kinematics').
//   v2v_sums          workgroup (g, b): the six per-workgroup sums of out and target (block_sums, the house sum).
//   v2v_map           workgroup (g, b): re-adds the partials of its b into the six means (every workgroup forms the same
//                     bits; workgroup 0 stores them for the backward), then one vertex per thread.
//   v2v_bwd_sums      the cotangent s per element, left in dL_dout, and its per-workgroup sums.
//   v2v_bwd_center    re-adds the partials, dL_dout = s - S / V in place.
// The rows are read with 4-byte loads: the arrays may start at any 4-byte boundary.  No atomics, no memsets, no
// allocation, no synchronisation: every output element is one thread's value in the header's order.  Compiled with
// -ffp-contract=off (build.py): no product is contracted into a fused multiply-add.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/exa_mesh.h"
#include "abi_status.h"
#include "axis_angle.h"
#include "fixed_sum.h"
#include "index_transpose.h"

namespace exa_mesh_impl {

using exa::ceil_div;

EXA_ABI_STATUS_SHARED("exa_mesh")         // exa_mesh_last_error() and its buffer are mesh_raster.hip's

namespace {

constexpr int FIT_BLOCK = EXA_MESH_FIT_ROWS;
constexpr int64_t FIT_MAX_ELEMS = 1 << 30;    // elements of any one array
constexpr int FIT_MAX_BATCH = 65535;          // B is a grid dimension of the centred term
static_assert(FIT_BLOCK == 256, "block_sums is written out for four waves");

__device__ __forceinline__ float fit_qnan() { return __int_as_float(0x7fc00000); }

__device__ __forceinline__ float fit_sign(float x) { return (x > 0.0f ? 1.0f : 0.0f) - (x < 0.0f ? 1.0f : 0.0f); }

// ---- edge length ------------------------------------------------------------------------------------------------------
struct EdgeArgs {
    int32_t B, V, F;
    int64_t gt_stride, valid_stride;          // per batch element: V * 3 and V, or 0 for a broadcast
    const float* out; const float* gt; const float* valid;
    const int32_t* faces; const int32_t* offsets; const int32_t* entries;
    const float* grad;
    float* loss; float* dout;
};

// the corners (a, b) of edge k
__device__ __forceinline__ int edge_a(int k) { return k == 2 ? 1 : 0; }
__device__ __forceinline__ int edge_b(int k) { return k == 0 ? 1 : 2; }

__device__ __forceinline__ float edge_length(const float* x, int a, int b, float* diff) {
    diff[0] = x[(int64_t)a * 3 + 0] - x[(int64_t)b * 3 + 0];
    diff[1] = x[(int64_t)a * 3 + 1] - x[(int64_t)b * 3 + 1];
    diff[2] = x[(int64_t)a * 3 + 2] - x[(int64_t)b * 3 + 2];
    return sqrtf((diff[0] * diff[0] + diff[1] * diff[1]) + diff[2] * diff[2]);
}

__device__ __forceinline__ bool edge_face(const EdgeArgs& a, int f, int* v) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = a.faces[(int64_t)f * 3 + k];
    return (unsigned)v[0] < (unsigned)a.V && (unsigned)v[1] < (unsigned)a.V && (unsigned)v[2] < (unsigned)a.V;
}

__global__ __launch_bounds__(FIT_BLOCK) void edge_fwd(EdgeArgs a) {
    const int64_t i = (int64_t)blockIdx.x * FIT_BLOCK + threadIdx.x;
    if (i >= (int64_t)a.B * a.F) return;
    const int b = (int)(i / a.F), f = (int)(i % a.F);
    float* loss = a.loss + (int64_t)b * 3 * a.F + f;
    int v[3];
    if (!edge_face(a, f, v)) {                                 // the guard: a row outside [0, V) is never read
#pragma unroll
        for (int k = 0; k < 3; ++k) loss[(int64_t)k * a.F] = fit_qnan();
        return;
    }
    const float* xo = a.out + (int64_t)b * a.V * 3;
    const float* xg = a.gt + b * a.gt_stride;
    const float* va = a.valid + b * a.valid_stride;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int p = v[edge_a(k)], q = v[edge_b(k)];
        float diff[3];
        const float d_out = edge_length(xo, p, q, diff);
        const float d_gt = edge_length(xg, p, q, diff);
        loss[(int64_t)k * a.F] = fabsf(d_out - d_gt) * (va[p] * va[q]);
    }
}

__global__ __launch_bounds__(FIT_BLOCK) void edge_bwd(EdgeArgs a) {
    const int64_t i = (int64_t)blockIdx.x * FIT_BLOCK + threadIdx.x;
    if (i >= (int64_t)a.B * a.V) return;
    const int b = (int)(i / a.V), vtx = (int)(i % a.V);
    const float* xo = a.out + (int64_t)b * a.V * 3;
    const float* xg = a.gt + b * a.gt_stride;
    const float* va = a.valid + b * a.valid_stride;
    const float* g = a.grad + (int64_t)b * 3 * a.F;
    const unsigned slots = 3u * (unsigned)a.F;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int q = a.offsets[vtx], end = a.offsets[vtx + 1]; q < end; ++q) {
        const unsigned e = (unsigned)a.entries[q];
        int v[3];
        if (e >= slots || !edge_face(a, (int)(e / 3u), v)) {   // the guard: nothing outside the tables is read
            acc[0] = acc[1] = acc[2] = fit_qnan();
            continue;
        }
        const int f = (int)(e / 3u), corner = (int)(e % 3u);
        // the two edges of this corner in ascending k: corner 0: k = 0, 1; corner 1: k = 0, 2; corner 2: k = 1, 2
        const int k0 = corner == 2 ? 1 : 0, k1 = corner == 0 ? 1 : 2;
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int k = n == 0 ? k0 : k1;
            const int p = v[edge_a(k)], r = v[edge_b(k)];
            float diff[3], dg[3];
            const float d_out = edge_length(xo, p, r, diff);
            const float d_gt = edge_length(xg, p, r, dg);
            const float m = va[p] * va[r];
            const float t = ((g[(int64_t)k * a.F + f] * m) * fit_sign(d_out - d_gt)) / d_out;
            const bool is_a = edge_a(k) == corner;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float qv = d_out == 0.0f ? 0.0f : t * diff[c];      // a zero-length edge contributes +0.0
                acc[c] = acc[c] + (is_a ? qv : -qv);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) a.dout[i * 3 + c] = acc[c];
}

// ---- flip symmetry ----------------------------------------------------------------------------------------------------
struct SymArgs {
    int32_t B, Vf;
    const float* p; const int32_t* taps; const float* w;
    const int32_t* offsets; const int32_t* entries;
    const float* grad;
    float* loss; float* dp;
};

// d_0 = p[i,0] + f_0, d_c = p[i,c] - f_c: what the row's three absolute values are taken of (pb: this batch element's rows)
__device__ __forceinline__ void sym_terms(const SymArgs& a, const float* pb, int i, float* d) {
    float r[3][3], w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int t = a.taps[(int64_t)i * 3 + k];
        w[k] = a.w[(int64_t)i * 3 + k];
#pragma unroll
        for (int c = 0; c < 3; ++c)
            r[k][c] = t == -1 ? 0.0f : (unsigned)t < (unsigned)a.Vf ? pb[(int64_t)t * 3 + c] : fit_qnan();
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float f = (r[0][c] * w[0] + r[1][c] * w[1]) + r[2][c] * w[2];
        const float x = pb[(int64_t)i * 3 + c];
        d[c] = c == 0 ? x + f : x - f;
    }
}

__global__ __launch_bounds__(FIT_BLOCK) void sym_fwd(SymArgs a) {
    const int64_t n = (int64_t)blockIdx.x * FIT_BLOCK + threadIdx.x;
    if (n >= (int64_t)a.B * a.Vf) return;
    const int i = (int)(n % a.Vf);
    float d[3];
    sym_terms(a, a.p + (n - i) * 3, i, d);
    a.loss[n] = (fabsf(d[0]) + fabsf(d[1])) + fabsf(d[2]);
}

__global__ __launch_bounds__(FIT_BLOCK) void sym_bwd(SymArgs a) {
    const int64_t n = (int64_t)blockIdx.x * FIT_BLOCK + threadIdx.x;
    if (n >= (int64_t)a.B * a.Vf) return;
    const int i = (int)(n % a.Vf);
    const float* pb = a.p + (n - i) * 3;
    const float* gb = a.grad + (n - i);
    const unsigned slots = 3u * (unsigned)a.Vf;
    float d[3], acc[3];
    sym_terms(a, pb, i, d);
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = fit_sign(d[c]) * gb[i];
    for (int q = a.offsets[i], end = a.offsets[i + 1]; q < end; ++q) {
        const unsigned e = (unsigned)a.entries[q];
        if (e >= slots) {                                      // the guard: nothing outside the tables is read
            acc[0] = acc[1] = acc[2] = fit_qnan();
            continue;
        }
        const int j = (int)(e / 3u);
        const float w = a.w[e], gj = gb[j];
        sym_terms(a, pb, j, d);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float s = fit_sign(d[c]) * gj;
            acc[c] = acc[c] + (c == 0 ? s : -s) * w;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) a.dp[n * 3 + c] = acc[c];
}

// ---- pose ---------------------------------------------------------------------------------------------------------------
struct PoseArgs {
    int64_t N;
    const float* out; const float* gt; const float* grad;
    float* loss; float* dout;
};

__device__ __forceinline__ void pose_matrices(const PoseArgs& a, int64_t n, float* Ro, float* Rg) {
    exa::quaternion_matrix(exa::aa_quaternion(a.out[n * 3 + 0], a.out[n * 3 + 1], a.out[n * 3 + 2]), Ro);
    exa::quaternion_matrix(exa::aa_quaternion(a.gt[n * 3 + 0], a.gt[n * 3 + 1], a.gt[n * 3 + 2]), Rg);
}

__global__ __launch_bounds__(FIT_BLOCK) void pose_fwd(PoseArgs a) {
    const int64_t n = (int64_t)blockIdx.x * FIT_BLOCK + threadIdx.x;
    if (n >= a.N) return;
    float Ro[9], Rg[9];
    pose_matrices(a, n, Ro, Rg);
#pragma unroll
    for (int q = 0; q < 9; ++q) a.loss[n * 9 + q] = fabsf(Ro[q] - Rg[q]);
}

__global__ __launch_bounds__(FIT_BLOCK) void pose_bwd(PoseArgs a) {
    const int64_t n = (int64_t)blockIdx.x * FIT_BLOCK + threadIdx.x;
    if (n >= a.N) return;
    float Ro[9], Rg[9], G[9], gp[3];
    pose_matrices(a, n, Ro, Rg);
#pragma unroll
    for (int q = 0; q < 9; ++q) G[q] = a.grad[n * 9 + q] * fit_sign(Ro[q] - Rg[q]);
    exa::aa_backward(a.out[n * 3 + 0], a.out[n * 3 + 1], a.out[n * 3 + 2], G, gp);
#pragma unroll
    for (int c = 0; c < 3; ++c) a.dout[n * 3 + c] = gp[c];
}

// ---- centred vertex-to-vertex -----------------------------------------------------------------------------------------
struct V2vArgs {
    int32_t V, blocks;
    float scale, nv;                          // nv = (float)V
    const float* out; const float* target; const float* weight; const float* grad;
    float* partials;                          // [B, K, blocks]: K = 6 forward, 3 backward
    float* means;                             // [B, 6]: written by the forward, read by the backward
    float* loss; float* dout;
};

// SUM2's second level for the K rows of batch element b: every thread ends with the K sums
template <int K>
__device__ __forceinline__ void v2v_totals(const V2vArgs& a, int b, float (&s)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0.0f;
    exa::strided_sums<FIT_BLOCK, K>(s, a.partials + (int64_t)b * K * a.blocks, a.blocks, a.blocks);
    exa::block_sums<FIT_BLOCK / 64>(s);      // the header's WG(s)
}

template <int K>
__device__ __forceinline__ void v2v_store_partials(const V2vArgs& a, int b, float (&s)[K]) {
    exa::block_sums<FIT_BLOCK / 64>(s);      // the header's WG(values)
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) a.partials[((int64_t)b * K + k) * a.blocks + blockIdx.x] = s[k];
    }
}

__global__ __launch_bounds__(FIT_BLOCK) void v2v_sums(V2vArgs a) {
    const int b = blockIdx.y, v = blockIdx.x * FIT_BLOCK + threadIdx.x;
    float s[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (v < a.V) {
        const int64_t o = ((int64_t)b * a.V + v) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s[c] = a.out[o + c];
            s[3 + c] = a.target[o + c];
        }
    }
    v2v_store_partials<6>(a, b, s);
}

// e = (a - ma) - (t - mt) of the thread's vertex
__device__ __forceinline__ void v2v_residual(const V2vArgs& a, int64_t o, const float* m, float* e) {
#pragma unroll
    for (int c = 0; c < 3; ++c) e[c] = (a.out[o + c] - m[c]) - (a.target[o + c] - m[3 + c]);
}

__global__ __launch_bounds__(FIT_BLOCK) void v2v_map(V2vArgs a) {
    const int b = blockIdx.y, v = blockIdx.x * FIT_BLOCK + threadIdx.x;
    float m[6];
    v2v_totals<6>(a, b, m);
#pragma unroll
    for (int k = 0; k < 6; ++k) m[k] = m[k] / a.nv;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) a.means[b * 6 + k] = m[k];
    }
    if (v >= a.V) return;
    const int64_t o = ((int64_t)b * a.V + v) * 3;
    const float w = a.weight[v];
    float e[3];
    v2v_residual(a, o, m, e);
#pragma unroll
    for (int c = 0; c < 3; ++c) a.loss[o + c] = (fabsf(e[c]) * w) * a.scale;
}

__global__ __launch_bounds__(FIT_BLOCK) void v2v_bwd_sums(V2vArgs a) {
    const int b = blockIdx.y, v = blockIdx.x * FIT_BLOCK + threadIdx.x;
    float s[3] = {0.0f, 0.0f, 0.0f};
    if (v < a.V) {
        const int64_t o = ((int64_t)b * a.V + v) * 3;
        const float w = a.weight[v];
        float m[6], e[3];
#pragma unroll
        for (int k = 0; k < 6; ++k) m[k] = a.means[b * 6 + k];
        v2v_residual(a, o, m, e);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s[c] = ((a.grad[o + c] * w) * a.scale) * fit_sign(e[c]);
            a.dout[o + c] = s[c];
        }
    }
    v2v_store_partials<3>(a, b, s);
}

__global__ __launch_bounds__(FIT_BLOCK) void v2v_bwd_center(V2vArgs a) {
    const int b = blockIdx.y, v = blockIdx.x * FIT_BLOCK + threadIdx.x;
    float S[3];
    v2v_totals<3>(a, b, S);
    if (v >= a.V) return;
    const int64_t o = ((int64_t)b * a.V + v) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) a.dout[o + c] = a.dout[o + c] - (S[c] / a.nv);
}

int check_rows(int64_t B, int64_t rows, int64_t width, const char* what) {
    if (B < 0 || rows < 0) return fail(EXA_MESH_E_INVALID, "negative size");
    if (B * rows * width > FIT_MAX_ELEMS) return fail(EXA_MESH_E_INVALID, what);
    return 0;
}

int check_edge(int32_t B, int32_t Bt, int32_t Bv, int32_t V, int32_t F) {
    if (F < 0) return fail(EXA_MESH_E_INVALID, "negative size");
    if (int rc = check_rows(B, V, 3, "B * V * 3 exceeds 2^30")) return rc;
    if (int rc = check_rows(B, F, 3, "B * F * 3 exceeds 2^30")) return rc;
    if (Bt != 1 && Bt != B) return fail(EXA_MESH_E_INVALID, "Bt (coord_gt batch) must be 1 or B");
    if (Bv != 1 && Bv != B) return fail(EXA_MESH_E_INVALID, "Bv (valid batch) must be 1 or B");
    return 0;
}

EdgeArgs edge_args(int32_t B, int32_t Bt, int32_t Bv, int32_t V, int32_t F, const float* coord_out, const float* coord_gt,
                   const float* valid, const int32_t* faces) {
    EdgeArgs a = {};
    a.B = B; a.V = V; a.F = F;
    a.gt_stride = Bt == 1 ? 0 : (int64_t)V * 3;
    a.valid_stride = Bv == 1 ? 0 : (int64_t)V;
    a.out = coord_out; a.gt = coord_gt; a.valid = valid; a.faces = faces;
    return a;
}

int check_v2v(int32_t B, int32_t V) {
    if (int rc = check_rows(B, V, 3, "B * V * 3 exceeds 2^30")) return rc;
    if (B > FIT_MAX_BATCH) return fail(EXA_MESH_E_INVALID, "B exceeds 65535");
    return 0;
}

}  // namespace

}  // namespace exa_mesh_impl

using namespace exa_mesh_impl;

extern "C" {

int exa_mesh_edge_length_forward(int32_t B, int32_t Bt, int32_t Bv, int32_t V, int32_t F, const float* coord_out,
                                 const float* coord_gt, const float* valid, const int32_t* faces, float* loss,
                                 void* stream) {
    if (int rc = check_edge(B, Bt, Bv, V, F)) return rc;
    if (B == 0 || F == 0) return 0;
    if (!coord_out || !coord_gt || !valid || !faces) return fail(EXA_MESH_E_NULLPTR, "coord_out / coord_gt / valid / faces is NULL");
    if (!loss) return fail(EXA_MESH_E_NULLPTR, "loss is NULL");
    EdgeArgs a = edge_args(B, Bt, Bv, V, F, coord_out, coord_gt, valid, faces);
    a.loss = loss;
    hipLaunchKernelGGL(edge_fwd, dim3(ceil_div((int64_t)B * F, FIT_BLOCK)), dim3(FIT_BLOCK), 0, (hipStream_t)stream, a);
    return launched("edge_fwd");
}

int exa_mesh_edge_length_backward(int32_t B, int32_t Bt, int32_t Bv, int32_t V, int32_t F, const float* coord_out,
                                  const float* coord_gt, const float* valid, const int32_t* faces,
                                  const int32_t* vert_offsets, const int32_t* vert_entries, const float* grad_loss,
                                  float* dL_dcoord_out, void* stream) {
    if (int rc = check_edge(B, Bt, Bv, V, F)) return rc;
    if (B == 0 || V == 0) return 0;
    if (!vert_offsets) return fail(EXA_MESH_E_NULLPTR, "vert_offsets is NULL");
    if (F > 0 && (!coord_out || !coord_gt || !valid || !faces || !vert_entries || !grad_loss))
        return fail(EXA_MESH_E_NULLPTR, "coord_out / coord_gt / valid / faces / vert_entries / grad_loss is NULL");
    if (!dL_dcoord_out) return fail(EXA_MESH_E_NULLPTR, "dL_dcoord_out is NULL");
    EdgeArgs a = edge_args(B, Bt, Bv, V, F, coord_out, coord_gt, valid, faces);
    a.offsets = vert_offsets; a.entries = vert_entries; a.grad = grad_loss; a.dout = dL_dcoord_out;
    hipLaunchKernelGGL(edge_bwd, dim3(ceil_div((int64_t)B * V, FIT_BLOCK)), dim3(FIT_BLOCK), 0, (hipStream_t)stream, a);
    return launched("edge_bwd");
}

int exa_mesh_flip_symmetry_plan(int32_t V_full, int32_t Vf, const int32_t* face_vertex_idx, const int32_t* closest_faces,
                                const float* bc, int32_t* vertex_row, int32_t* taps, float* weights, int32_t* offsets,
                                int32_t* entries) {
    if (V_full < 0 || Vf < 0) return fail(EXA_MESH_E_INVALID, "negative size");
    if ((int64_t)V_full * 3 > FIT_MAX_ELEMS) return fail(EXA_MESH_E_INVALID, "V_full * 3 exceeds 2^30");
    if (!offsets || (V_full > 0 && (!closest_faces || !bc || !vertex_row)) ||
        (Vf > 0 && (!face_vertex_idx || !taps || !weights || !entries)))
        return fail(EXA_MESH_E_NULLPTR, "NULL argument");
    char what[160];
    for (int64_t e = 0; e < (int64_t)V_full * 3; ++e) {
        if (closest_faces[e] < 0 || closest_faces[e] >= V_full) {
            snprintf(what, sizeof(what), "closest_faces index %d of vertex %d, slot %d is outside [0, %d)",
                     (int)closest_faces[e], (int)(e / 3), (int)(e % 3), (int)V_full);
            return fail(EXA_MESH_E_INVALID, what);
        }
    }
    for (int32_t v = 0; v < V_full; ++v) vertex_row[v] = -1;
    for (int32_t i = 0; i < Vf; ++i) {
        const int32_t v = face_vertex_idx[i];
        if (v < 0 || v >= V_full) {
            snprintf(what, sizeof(what), "face_vertex_idx[%d] = %d is outside [0, %d)", (int)i, (int)v, (int)V_full);
            return fail(EXA_MESH_E_INVALID, what);
        }
        if (vertex_row[v] != -1) {
            snprintf(what, sizeof(what), "face_vertex_idx names vertex %d twice (rows %d and %d)", (int)v,
                     (int)vertex_row[v], (int)i);
            return fail(EXA_MESH_E_INVALID, what);
        }
        vertex_row[v] = i;
    }
    for (int32_t i = 0; i < Vf; ++i) {
        const int64_t v = face_vertex_idx[i];
        for (int k = 0; k < 3; ++k) {
            taps[(int64_t)i * 3 + k] = vertex_row[closest_faces[v * 3 + k]];
            weights[(int64_t)i * 3 + k] = bc[v * 3 + k];
        }
    }
    // ascending (row, slot) per tapped row: the shared index transpose (index_transpose.h); -1 taps name no row
    if (exa::index_transpose(Vf, (int64_t)Vf * 3, taps, true, offsets, entries) >= 0)
        return fail(EXA_MESH_E_INVALID, "flip_symmetry_plan: a tap left [-1, Vf)");
    return 0;
}

int exa_mesh_flip_symmetry_forward(int32_t B, int32_t Vf, const float* face_offset, const int32_t* taps,
                                   const float* weights, float* loss, void* stream) {
    if (int rc = check_rows(B, Vf, 3, "B * Vf * 3 exceeds 2^30")) return rc;
    if (B == 0 || Vf == 0) return 0;
    if (!face_offset || !taps || !weights) return fail(EXA_MESH_E_NULLPTR, "face_offset / taps / weights is NULL");
    if (!loss) return fail(EXA_MESH_E_NULLPTR, "loss is NULL");
    SymArgs a = {};
    a.B = B; a.Vf = Vf; a.p = face_offset; a.taps = taps; a.w = weights; a.loss = loss;
    hipLaunchKernelGGL(sym_fwd, dim3(ceil_div((int64_t)B * Vf, FIT_BLOCK)), dim3(FIT_BLOCK), 0, (hipStream_t)stream, a);
    return launched("sym_fwd");
}

int exa_mesh_flip_symmetry_backward(int32_t B, int32_t Vf, const float* face_offset, const int32_t* taps,
                                    const float* weights, const int32_t* offsets, const int32_t* entries,
                                    const float* grad_loss, float* dL_dface_offset, void* stream) {
    if (int rc = check_rows(B, Vf, 3, "B * Vf * 3 exceeds 2^30")) return rc;
    if (B == 0 || Vf == 0) return 0;
    if (!face_offset || !taps || !weights) return fail(EXA_MESH_E_NULLPTR, "face_offset / taps / weights is NULL");
    if (!offsets || !entries || !grad_loss) return fail(EXA_MESH_E_NULLPTR, "offsets / entries / grad_loss is NULL");
    if (!dL_dface_offset) return fail(EXA_MESH_E_NULLPTR, "dL_dface_offset is NULL");
    SymArgs a = {};
    a.B = B; a.Vf = Vf; a.p = face_offset; a.taps = taps; a.w = weights;
    a.offsets = offsets; a.entries = entries; a.grad = grad_loss; a.dp = dL_dface_offset;
    hipLaunchKernelGGL(sym_bwd, dim3(ceil_div((int64_t)B * Vf, FIT_BLOCK)), dim3(FIT_BLOCK), 0, (hipStream_t)stream, a);
    return launched("sym_bwd");
}

int exa_mesh_pose_loss_forward(int64_t N, const float* pose_out, const float* pose_gt, float* loss, void* stream) {
    if (int rc = check_rows(1, N, 9, "N * 9 exceeds 2^30")) return rc;
    if (N == 0) return 0;
    if (!pose_out || !pose_gt || !loss) return fail(EXA_MESH_E_NULLPTR, "pose_out / pose_gt / loss is NULL");
    PoseArgs a = {};
    a.N = N; a.out = pose_out; a.gt = pose_gt; a.loss = loss;
    hipLaunchKernelGGL(pose_fwd, dim3(ceil_div(N, FIT_BLOCK)), dim3(FIT_BLOCK), 0, (hipStream_t)stream, a);
    return launched("pose_fwd");
}

int exa_mesh_pose_loss_backward(int64_t N, const float* pose_out, const float* pose_gt, const float* grad_loss,
                                float* dL_dpose_out, void* stream) {
    if (int rc = check_rows(1, N, 9, "N * 9 exceeds 2^30")) return rc;
    if (N == 0) return 0;
    if (!pose_out || !pose_gt || !grad_loss || !dL_dpose_out)
        return fail(EXA_MESH_E_NULLPTR, "pose_out / pose_gt / grad_loss / dL_dpose_out is NULL");
    PoseArgs a = {};
    a.N = N; a.out = pose_out; a.gt = pose_gt; a.grad = grad_loss; a.dout = dL_dpose_out;
    hipLaunchKernelGGL(pose_bwd, dim3(ceil_div(N, FIT_BLOCK)), dim3(FIT_BLOCK), 0, (hipStream_t)stream, a);
    return launched("pose_bwd");
}

int64_t exa_mesh_centered_v2v_blocks(int32_t V) { return V <= 0 ? 0 : ((int64_t)V + FIT_BLOCK - 1) / FIT_BLOCK; }

int exa_mesh_centered_v2v_forward(int32_t B, int32_t V, const float* out, const float* target, const float* weight,
                                  float scale, float* partials, float* means, float* loss, void* stream) {
    if (int rc = check_v2v(B, V)) return rc;
    if (B == 0 || V == 0) return 0;
    if (!out || !target || !weight) return fail(EXA_MESH_E_NULLPTR, "out / target / weight is NULL");
    if (!partials || !means || !loss) return fail(EXA_MESH_E_NULLPTR, "partials / means / loss is NULL");
    V2vArgs a = {};
    a.V = V; a.blocks = (int32_t)exa_mesh_centered_v2v_blocks(V); a.scale = scale; a.nv = (float)V;
    a.out = out; a.target = target; a.weight = weight; a.partials = partials; a.means = means; a.loss = loss;
    const dim3 grid((unsigned)a.blocks, (unsigned)B);
    hipLaunchKernelGGL(v2v_sums, grid, dim3(FIT_BLOCK), 0, (hipStream_t)stream, a);
    if (int rc = launched("v2v_sums")) return rc;
    hipLaunchKernelGGL(v2v_map, grid, dim3(FIT_BLOCK), 0, (hipStream_t)stream, a);
    return launched("v2v_map");
}

int exa_mesh_centered_v2v_backward(int32_t B, int32_t V, const float* out, const float* target, const float* weight,
                                   float scale, const float* means, const float* grad_loss, float* partials,
                                   float* dL_dout, void* stream) {
    if (int rc = check_v2v(B, V)) return rc;
    if (B == 0 || V == 0) return 0;
    if (!out || !target || !weight) return fail(EXA_MESH_E_NULLPTR, "out / target / weight is NULL");
    if (!means || !grad_loss || !partials || !dL_dout)
        return fail(EXA_MESH_E_NULLPTR, "means / grad_loss / partials / dL_dout is NULL");
    V2vArgs a = {};
    a.V = V; a.blocks = (int32_t)exa_mesh_centered_v2v_blocks(V); a.scale = scale; a.nv = (float)V;
    a.out = out; a.target = target; a.weight = weight; a.grad = grad_loss; a.partials = partials;
    a.means = (float*)means; a.dout = dL_dout;
    const dim3 grid((unsigned)a.blocks, (unsigned)B);
    hipLaunchKernelGGL(v2v_bwd_sums, grid, dim3(FIT_BLOCK), 0, (hipStream_t)stream, a);
    if (int rc = launched("v2v_bwd_sums")) return rc;
    hipLaunchKernelGGL(v2v_bwd_center, grid, dim3(FIT_BLOCK), 0, (hipStream_t)stream, a);
    return launched("v2v_bwd_center");
}

}  // extern "C"
