// SMPL-X template stage and mesh upsampling (include/exa_mesh.h, exa_mesh_upsample_* and exa_mesh_body_*): the
// reference's get_neutral_pose_human(True, True) + get_zero_pose_human (module.py:337-387) and upsample_mesh
// (smpl_x.py:84-91).  The semantics -- the op-by-op fp32 forward and the order of every sum of the backward -- are
// written out in the header; this file implements them.
//
//   up_fwd            one thread per element of the fine mesh: a copy, a midpoint, or a midpoint of midpoints recomputed
//                     in the thread from the flat parent table.
//   up_bwd            one thread per element of a coarser level: its own gradient, then its dependants' halves in the
//                     CSR's order.  Launched once per round, the finer round first.
//   body_shape        one thread per element of v_shaped: the L-term sum over the feature-major directions (coef in
//                     LDS, eight rows in flight), + v_base, and v_posed next to it.
//   body_jreg         one wave per joint: the lanes stride over the row's non-zeros, then the header's tree.
//   body_add          the two cotangents of the neutral-pose joints, added.
//   body_jreg_bwd     one thread per element of dL/dv_shaped: the skinning's point gradient, then the column's
//                     non-zeros in ascending joint; the first workgroup also writes dL/djoint_offset.
//   body_coef_partial / body_coef_finish    dL/dcoef's two-level sum.
// The kinematic chains and the skinning are the library's own entry points (exa_mesh_kinematics_*, exa_skin_*), called
// on the caller's stream.  No atomics, no memsets, no allocation, no synchronisation.  Compiled with -ffp-contract=off
// (build.py): no product is contracted into a fused multiply-add.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/exa_mesh.h"
#include "../../include/exa_skin.h"
#include "abi_status.h"
#include "body.h"
#include "fixed_sum.h"

namespace exa_mesh_impl {

using exa::align256;
using exa::ceil_div;

EXA_ABI_STATUS_SHARED("exa_mesh")         // exa_mesh_last_error() and its buffer are mesh_raster.hip's

constexpr int UP_BLOCK = 256;
constexpr int UP_MAXC = EXA_MESH_UP_MAX_CHANNELS;
constexpr int64_t UP_MAXV = EXA_MESH_UP_MAX_VERTS;
constexpr int BD_BLOCK = 256;
constexpr int BD_MAXL = EXA_MESH_BODY_MAX_COEF;
constexpr int BD_ROWS = 8;                    // direction rows in flight per thread
constexpr int BD_CHUNK = EXA_MESH_BODY_CHUNK;
constexpr int BD_CROWS = 16;                  // direction rows per workgroup of body_coef_partial
constexpr int BD_MAXJ = EXA_MESH_KIN_MAX_JOINTS;
constexpr int64_t BD_MAXV = EXA_MESH_BODY_MAX_VERTS;
static_assert(BD_CHUNK == BD_BLOCK && BD_BLOCK == 4 * 64, "one element per lane, four waves per chunk");
static_assert(BD_MAXL <= BD_STAGE && 9 * (BD_MAXJ - 1) <= BD_STAGE, "coef staging");

// ---- upsampling -----------------------------------------------------------------------------------------------------

struct UpFwdParams {
    int32_t V0, V1, Vn, C;
    const int32_t* par;
    const float* x;
    float* out;
};

// the value of vertex p of the level below the finest: a coarse vertex, or a round-1 midpoint recomputed
__device__ __forceinline__ float up_val(const UpFwdParams& P, int p, int c) {
    if (p < P.V0) return P.x[(int64_t)p * P.C + c];
    const int a = P.par[2 * (int64_t)(p - P.V0)], b = P.par[2 * (int64_t)(p - P.V0) + 1];
    if ((unsigned)a >= (unsigned)P.V0 || (unsigned)b >= (unsigned)P.V0) return __int_as_float(0x7fc00000);
    return (P.x[(int64_t)a * P.C + c] + P.x[(int64_t)b * P.C + c]) * 0.5f;
}

__global__ __launch_bounds__(UP_BLOCK) void up_fwd(UpFwdParams P) {
    const int64_t e = (int64_t)blockIdx.x * UP_BLOCK + threadIdx.x;
    if (e >= (int64_t)P.Vn * P.C) return;
    const int i = (int)(e / P.C), c = (int)(e - (int64_t)i * P.C);
    if (i < P.V0) {
        P.out[e] = P.x[e];
        return;
    }
    const int a = P.par[2 * (int64_t)(i - P.V0)], b = P.par[2 * (int64_t)(i - P.V0) + 1];
    const int lim = i < P.V1 ? P.V0 : P.V1;   // the guard: a parent outside its level reads nothing
    if ((unsigned)a >= (unsigned)lim || (unsigned)b >= (unsigned)lim) {
        P.out[e] = __int_as_float(0x7fc00000);
        return;
    }
    P.out[e] = (up_val(P, a, c) + up_val(P, b, c)) * 0.5f;
}

struct UpBwdParams {
    int32_t Vc, Vf, C;                        // vertices of this level, of the level above it
    const int32_t* off;
    const int32_t* dep;
    const float* g;                           // [Vf, C]
    const float* extra;                       // [Vc, C] or NULL
    float* out;                               // [Vc, C]
};

__global__ __launch_bounds__(UP_BLOCK) void up_bwd(UpBwdParams P) {
    const int64_t e = (int64_t)blockIdx.x * UP_BLOCK + threadIdx.x;
    if (e >= (int64_t)P.Vc * P.C) return;
    const int p = (int)(e / P.C), c = (int)(e - (int64_t)p * P.C);
    float acc = P.g[e];
    if (P.extra) acc = P.extra[e] + acc;
    const int e0 = max(P.off[p], 0), e1 = min(P.off[p + 1], 2 * (P.Vf - P.Vc));      // the guard: inside dep
    for (int k = e0; k < e1; ++k) {
        const int d = P.dep[k];
        if ((unsigned)d < (unsigned)P.Vf) acc = acc + P.g[(int64_t)d * P.C + c] * 0.5f;
    }
    P.out[e] = acc;
}

int up_check(const ExaMeshUpsample* up, int32_t C) {
    if (!up) return fail(EXA_MESH_E_NULLPTR, "up (the upsampling plan) is NULL");
    if (up->levels != 1 && up->levels != 2) return fail(EXA_MESH_E_INVALID, "levels (subdivide_num) must be 1 or 2");
    if (C < 1 || C > UP_MAXC) return fail(EXA_MESH_E_INVALID, "C (channels) must be 1 .. 8");
    if (up->V0 < 0 || up->V1 < up->V0 || up->Vn < up->V1) return fail(EXA_MESH_E_INVALID, "need 0 <= V0 <= V1 <= Vn");
    if (up->levels == 1 && up->Vn != up->V1) return fail(EXA_MESH_E_INVALID, "Vn must equal V1 with one round");
    if ((int64_t)up->Vn > UP_MAXV) return fail(EXA_MESH_E_INVALID, "Vn (fine vertices) exceeds 2^26");
    if (up->Vn > up->V0 && !up->par) return fail(EXA_MESH_E_NULLPTR, "par is NULL");
    return 0;
}

int up_forward(const ExaMeshUpsample* up, int32_t C, const float* x, float* out, hipStream_t st) {
    if (int rc = up_check(up, C)) return rc;
    if (up->Vn == 0) return 0;
    if (!x || !out) return fail(EXA_MESH_E_NULLPTR, "x / out is NULL");
    const UpFwdParams P = {up->V0, up->V1, up->Vn, C, up->par, x, out};
    hipLaunchKernelGGL(up_fwd, dim3(ceil_div((int64_t)up->Vn * C, UP_BLOCK)), dim3(UP_BLOCK), 0, st, P);
    return launched("up_fwd");
}

uint64_t up_workspace_bytes(const ExaMeshUpsample* up, int32_t C) {
    return up->levels == 2 ? align256((uint64_t)up->V1 * C * sizeof(float)) : 0;
}

int up_backward(const ExaMeshUpsample* up, int32_t C, const float* g, const float* g_extra, void* ws, uint64_t ws_bytes,
                float* dx, hipStream_t st) {
    if (int rc = up_check(up, C)) return rc;
    if (up->V0 == 0) return 0;
    if (!g || !dx) return fail(EXA_MESH_E_NULLPTR, "g / dx is NULL");
    if (!up->off1 || (up->V1 > up->V0 && !up->dep1)) return fail(EXA_MESH_E_NULLPTR, "off1 / dep1 is NULL");
    const float* h = g;
    if (up->levels == 2) {
        if (!up->off2 || (up->Vn > up->V1 && !up->dep2)) return fail(EXA_MESH_E_NULLPTR, "off2 / dep2 is NULL");
        if (!ws) return fail(EXA_MESH_E_NULLPTR, "ws (workspace) is NULL");
        if (ws_bytes < (uint64_t)up->V1 * C * sizeof(float))
            return fail(EXA_MESH_E_INVALID, "workspace is smaller than 4 V1 C bytes");
        const UpBwdParams P2 = {up->V1, up->Vn, C, up->off2, up->dep2, g, nullptr, (float*)ws};
        hipLaunchKernelGGL(up_bwd, dim3(ceil_div((int64_t)up->V1 * C, UP_BLOCK)), dim3(UP_BLOCK), 0, st, P2);
        if (int rc = launched("up_bwd (round 2)")) return rc;
        h = (const float*)ws;
    }
    const UpBwdParams P1 = {up->V0, up->V1, C, up->off1, up->dep1, h, g_extra, dx};
    hipLaunchKernelGGL(up_bwd, dim3(ceil_div((int64_t)up->V0 * C, UP_BLOCK)), dim3(UP_BLOCK), 0, st, P1);
    return launched("up_bwd (round 1)");
}

// One round on the host: the unique edges of `faces` over V vertices in ascending (low, high), the subdivided faces
// and, per face, nothing else.  Every index is known to lie in [0, V).
void up_round(int64_t V, const std::vector<int32_t>& faces, std::vector<int32_t>& edges, std::vector<int32_t>& next) {
    const size_t F = faces.size() / 3;
    std::vector<uint64_t> keys(3 * F);
    for (size_t f = 0; f < F; ++f) {
        const int32_t v[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
        for (int k = 0; k < 3; ++k) {         // edge k is the one opposite corner k
            const int32_t a = v[(k + 1) % 3], b = v[(k + 2) % 3];
            keys[3 * f + k] = (uint64_t)std::min(a, b) * (uint64_t)V + (uint64_t)std::max(a, b);
        }
    }
    std::vector<uint64_t> uniq(keys);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    edges.resize(2 * uniq.size());
    for (size_t e = 0; e < uniq.size(); ++e) {
        edges[2 * e] = (int32_t)(uniq[e] / (uint64_t)V);
        edges[2 * e + 1] = (int32_t)(uniq[e] % (uint64_t)V);
    }
    next.resize(12 * F);
    for (size_t f = 0; f < F; ++f) {
        int32_t m[3];
        for (int k = 0; k < 3; ++k)
            m[k] = (int32_t)(V + (std::lower_bound(uniq.begin(), uniq.end(), keys[3 * f + k]) - uniq.begin()));
        const int32_t v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
        const int32_t rows[4][3] = {{v0, m[2], m[1]}, {v1, m[0], m[2]}, {v2, m[1], m[0]}, {m[0], m[1], m[2]}};
        for (int g = 0; g < 4; ++g)
            for (int k = 0; k < 3; ++k) next[3 * (g * F + f) + k] = rows[g][k];
    }
}

// The dependants' CSR of one round: Vc coarse vertices, E new vertices Vc .. Vc + E - 1 with parents `edges`.
void up_transpose(int32_t Vc, const std::vector<int32_t>& edges, int32_t* off, int32_t* dep) {
    const size_t E = edges.size() / 2;
    for (int32_t p = 0; p <= Vc; ++p) off[p] = 0;
    for (size_t i = 0; i < 2 * E; ++i) ++off[edges[i] + 1];
    for (int32_t p = 0; p < Vc; ++p) off[p + 1] += off[p];
    std::vector<int32_t> fill(off, off + Vc);
    for (size_t e = 0; e < E; ++e)            // ascending dependant, low parent before high
        for (int s = 0; s < 2; ++s) dep[fill[edges[2 * e + s]]++] = (int32_t)(Vc + e);
}

// ---- the template stage ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(BD_BLOCK) void body_shape(ShapeParams P) {
    __shared__ float coef_l[BD_STAGE];
    const int tid = threadIdx.x;
    for (int l = tid; l < P.L; l += BD_BLOCK) coef_l[l] = l < P.La ? P.coef[l] : P.coef_b[l - P.La];
    if (blockIdx.x == 0 && tid < 3 && P.zero3) P.zero3[tid] = 0.0f;
    __syncthreads();
    const int m = blockIdx.x * BD_BLOCK + tid;
    if (m >= P.M) return;
    const int64_t ld = P.M;
    const float* p = P.dirs + m;
    float s = 0.0f;
    int l = 0;
    for (; l + BD_ROWS <= P.L; l += BD_ROWS) {
        float t[BD_ROWS];
#pragma unroll
        for (int i = 0; i < BD_ROWS; ++i) t[i] = p[i * ld];
#pragma unroll
        for (int i = 0; i < BD_ROWS; ++i) s = s + coef_l[l + i] * t[i];
        p += BD_ROWS * ld;
    }
    for (; l < P.L; ++l) {
        s = s + coef_l[l] * *p;
        p += ld;
    }
    const float vs = P.base[m] + s;
    P.v_shaped[m] = vs;
    if (P.pose_offsets) P.v_posed[m] = vs + P.pose_offsets[m];
}

__global__ __launch_bounds__(64) void body_jreg(JregParams P) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const int i0 = max(P.off[j], 0), i1 = min(P.off[j + 1], P.nnz);      // the guard: inside col / val
    float p[3] = {0.0f, 0.0f, 0.0f};
    for (int i = i0 + lane; i < i1; i += 64) {
        const int v = P.col[i];
        const float w = P.val[i];
        if ((unsigned)v < (unsigned)P.V) {    // the guard: an index outside the mesh reads nothing
#pragma unroll
            for (int c = 0; c < 3; ++c) p[c] = p[c] + w * P.v_shaped[3 * (int64_t)v + c];
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) p[c] = __int_as_float(0x7fc00000);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) exa::wave_sum_lane0(p[c]);      // lane 0: the header's tree
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) P.Jr[3 * j + c] = (j == P.root || !P.joint_offset) ? p[c] : p[c] + P.joint_offset[3 * j + c];
    }
}

__global__ __launch_bounds__(BD_BLOCK) void body_add(int n, const float* a, const float* b, float* out) {
    const int i = blockIdx.x * BD_BLOCK + threadIdx.x;
    if (i < n) out[i] = a[i] + b[i];
}

__global__ __launch_bounds__(BD_BLOCK) void body_jreg_bwd(JregBwdParams P) {
    __shared__ float dJ[3 * BD_MAXJ];
    const int tid = threadIdx.x;
    if (tid < 3 * P.J) {
        float v = 0.0f;
        if (P.gJA && P.gJC) v = P.gJA[tid] + P.gJC[tid];
        else if (P.gJA) v = P.gJA[tid];
        else if (P.gJC) v = P.gJC[tid];
        dJ[tid] = v;
        if (blockIdx.x == 0 && P.d_joint_offset) P.d_joint_offset[tid] = tid / 3 == P.root ? 0.0f : v;
    }
    __syncthreads();
    if (!P.dvs) return;
    const int m = blockIdx.x * BD_BLOCK + tid;
    if (m >= 3 * P.V) return;
    const int v = m / 3, c = m - 3 * v;
    float acc = P.g_vp ? P.g_vp[m] : 0.0f;
    const int i0 = max(P.off[v], 0), i1 = min(P.off[v + 1], P.nnz);      // the guard: inside row / val
    for (int i = i0; i < i1; ++i) {
        const int j = P.row[i];
        if ((unsigned)j < (unsigned)P.J) acc = acc + P.val[i] * dJ[3 * j + c];
    }
    P.dvs[m] = acc;
}

__global__ __launch_bounds__(BD_BLOCK) void body_coef_partial(CoefParams P) {
    __shared__ float wl[BD_CROWS][4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int chunk = blockIdx.x, r0 = blockIdx.y * BD_CROWS;
    const int m = chunk * BD_CHUNK + tid;
    const bool inside = m < P.M;
    const float g = inside ? P.dvs[m] : 0.0f;
    const int64_t ld = P.M;
#pragma unroll 4
    for (int r = 0; r < BD_CROWS; ++r) {
        const int l = r0 + r;
        const float t = (inside && l < P.L) ? P.dirs[l * ld + m] : 0.0f;
        float q = inside ? t * g : 0.0f;
        exa::wave_sum_lane0(q);
        if (lane == 0) wl[r][wave] = q;
    }
    __syncthreads();
    if (tid < BD_CROWS && r0 + tid < P.L)
        P.partial[(int64_t)chunk * P.L + r0 + tid] = ((wl[tid][0] + wl[tid][1]) + wl[tid][2]) + wl[tid][3];
}

__global__ __launch_bounds__(BD_BLOCK) void body_coef_finish(CoefParams P) {
    const int l = blockIdx.x * BD_BLOCK + threadIdx.x;
    if (l >= P.L) return;
    float acc = 0.0f;
    for (int ch = 0; ch < P.chunks; ++ch) acc = acc + P.partial[(int64_t)ch * P.L + l];
    if (l < P.split) P.dcoef[l] = acc;
    else P.dcoef_b[l - P.split] = acc;
}

int launch_body_shape(const ShapeParams& P, hipStream_t st) {
    hipLaunchKernelGGL(body_shape, dim3(ceil_div(P.M, BD_BLOCK)), dim3(BD_BLOCK), 0, st, P);
    return launched("body_shape");
}

int launch_body_jreg(const JregParams& P, int32_t J, hipStream_t st) {
    hipLaunchKernelGGL(body_jreg, dim3(J), dim3(64), 0, st, P);
    return launched("body_jreg");
}

int launch_body_jreg_bwd(const JregBwdParams& P, bool all_vertices, hipStream_t st) {
    hipLaunchKernelGGL(body_jreg_bwd, dim3(all_vertices ? ceil_div(3 * (int64_t)P.V, BD_BLOCK) : 1), dim3(BD_BLOCK), 0, st, P);
    return launched("body_jreg_bwd");
}

int launch_body_coef(const CoefParams& P, hipStream_t st) {
    hipLaunchKernelGGL(body_coef_partial, dim3(P.chunks, ceil_div(P.L, BD_CROWS)), dim3(BD_BLOCK), 0, st, P);
    if (int rc = launched("body_coef_partial")) return rc;
    hipLaunchKernelGGL(body_coef_finish, dim3(ceil_div(P.L, BD_BLOCK)), dim3(BD_BLOCK), 0, st, P);
    return launched("body_coef_finish");
}

// the forward's workspace, in floats from its start (every section on a 256-byte boundary)
struct BodyFwdLayout {
    uint64_t v_shaped, v_posed, Jr, A, zero3, rot, T, posed, bytes;
};

// the backward's, in bytes
struct BodyBwdLayout {
    uint64_t gB, gpA, gJA, gJC, gA, gm, gvp, dvs, up, skin, partial, bytes;
    uint64_t up_bytes, skin_bytes;
};

int body_check(const ExaMeshBody* b) {
    if (!b) return fail(EXA_MESH_E_NULLPTR, "body is NULL");
    if (b->V < 1 || (int64_t)b->V > BD_MAXV) return fail(EXA_MESH_E_INVALID, "V (vertices) must be 1 .. 2^24");
    if (b->L < 1 || b->L > BD_MAXL) return fail(EXA_MESH_E_INVALID, "L (coefficients) must be 1 .. 512");
    if (b->J < 1 || b->J > BD_MAXJ) return fail(EXA_MESH_E_INVALID, "J (joints) must be 1 .. 64");
    if (b->nnz < 0 || (int64_t)b->nnz > (int64_t)b->J * b->V)
        return fail(EXA_MESH_E_INVALID, "nnz (regressor non-zeros) must be 0 .. J V");
    if (b->root < 0 || b->root >= b->J) return fail(EXA_MESH_E_INVALID, "root must lie in [0, J)");
    if (int rc = up_check(b->up, 3)) return rc;
    if (b->up->V0 != b->V) return fail(EXA_MESH_E_INVALID, "the upsampling plan's V0 is not V");
    return 0;
}

int body_layouts(const ExaMeshBody* b, BodyFwdLayout* f, BodyBwdLayout* w) {
    const uint64_t V3 = 3 * (uint64_t)b->V, J = (uint64_t)b->J, F = sizeof(float);
    uint64_t at = 0;
    auto take = [&at](uint64_t bytes) {
        const uint64_t here = at;
        at += align256(bytes);
        return here;
    };
    f->v_shaped = take(V3 * F) / F;
    f->v_posed = take(V3 * F) / F;
    f->Jr = take(3 * J * F) / F;
    f->A = take(16 * J * F) / F;
    f->zero3 = take(3 * F) / F;
    f->rot = take(9 * J * F) / F;
    f->T = take(16 * J * F) / F;
    f->posed = take(3 * J * F) / F;
    f->bytes = at;
    uint64_t skin = 0;
    if (exa_skin_workspace_size(b->V, b->J, &skin) != 0)
        return fail(EXA_MESH_E_INVALID, "the skinning refuses these sizes (exa_skin_workspace_size)");
    at = 0;
    w->gB = take(3 * J * F);
    w->gpA = take(3 * J * F);
    w->gJA = take(3 * J * F);
    w->gJC = take(3 * J * F);
    w->gA = take(16 * J * F);
    w->gm = take(V3 * F);
    w->gvp = take(V3 * F);
    w->dvs = take(V3 * F);
    w->up_bytes = up_workspace_bytes(b->up, 3);
    w->up = take(w->up_bytes);
    w->skin_bytes = skin;
    w->skin = take(skin);
    w->partial = take((uint64_t)ceil_div((int64_t)V3, BD_CHUNK) * b->L * F);
    w->bytes = at;
    return 0;
}

// a failing call of the skinning reports through its own ABI: carry its text over
int skin_failed(int rc) {
    char what[exa::ABI_ERR_BYTES - 32];
    snprintf(what, sizeof(what), "skinning: %s", exa_skin_last_error());
    return fail(rc, what);
}

}  // namespace exa_mesh_impl

using namespace exa_mesh_impl;

extern "C" {

int exa_mesh_upsample_plan(int32_t V0, int32_t F0, const int32_t* faces, int32_t levels, int32_t* counts, int32_t* par,
                           int32_t* faces_out, int32_t* off1, int32_t* dep1, int32_t* off2, int32_t* dep2) {
    if (levels != 1 && levels != 2) return fail(EXA_MESH_E_INVALID, "levels (subdivide_num) must be 1 or 2");
    if (V0 < 0 || F0 < 0) return fail(EXA_MESH_E_INVALID, "negative size");
    if ((int64_t)V0 + 3 * (int64_t)F0 * (levels == 2 ? 5 : 1) > UP_MAXV)
        return fail(EXA_MESH_E_INVALID, "the fine mesh may exceed 2^26 vertices");
    if (!counts) return fail(EXA_MESH_E_NULLPTR, "counts is NULL");
    if (F0 > 0 && !faces) return fail(EXA_MESH_E_NULLPTR, "faces is NULL");
    const bool fill = par || faces_out || off1 || dep1 || (levels == 2 && (off2 || dep2));
    if (fill && (!par || !faces_out || !off1 || !dep1 || (levels == 2 && (!off2 || !dep2))))
        return fail(EXA_MESH_E_NULLPTR, "the output arrays must be all given or all NULL");
    for (int64_t i = 0; i < 3 * (int64_t)F0; ++i) {
        if (faces[i] < 0 || faces[i] >= V0) {
            char what[96];
            snprintf(what, sizeof(what), "faces[%lld][%d] = %d lies outside [0, %d)", (long long)(i / 3), (int)(i % 3),
                     (int)faces[i], (int)V0);
            return fail(EXA_MESH_E_INVALID, what);
        }
    }
    std::vector<int32_t> f0(faces, faces + 3 * (size_t)F0), e0, f1, e1, f2;
    up_round(V0, f0, e0, f1);
    const int32_t V1 = V0 + (int32_t)(e0.size() / 2);
    int32_t Vn = V1;
    if (levels == 2) {
        up_round(V1, f1, e1, f2);
        Vn = V1 + (int32_t)(e1.size() / 2);
    }
    const std::vector<int32_t>& last = levels == 2 ? f2 : f1;
    counts[0] = V1;
    counts[1] = Vn;
    counts[2] = (int32_t)(last.size() / 3);
    if (!fill) return 0;
    std::copy(e0.begin(), e0.end(), par);
    std::copy(e1.begin(), e1.end(), par + e0.size());
    std::copy(last.begin(), last.end(), faces_out);
    up_transpose(V0, e0, off1, dep1);
    if (levels == 2) up_transpose(V1, e1, off2, dep2);
    return 0;
}

int exa_mesh_upsample_forward(const ExaMeshUpsample* up, int32_t C, const float* x, float* out, void* stream) {
    return up_forward(up, C, x, out, (hipStream_t)stream);
}

int exa_mesh_upsample_backward(const ExaMeshUpsample* up, int32_t C, const float* g, const float* g_extra, void* ws,
                               uint64_t ws_bytes, float* dx, void* stream) {
    return up_backward(up, C, g, g_extra, ws, ws_bytes, dx, (hipStream_t)stream);
}

int exa_mesh_body_workspace_sizes(const ExaMeshBody* body, uint64_t* fwd_bytes, uint64_t* bwd_bytes) {
    if (int rc = body_check(body)) return rc;
    if (!fwd_bytes || !bwd_bytes) return fail(EXA_MESH_E_NULLPTR, "fwd_bytes / bwd_bytes is NULL");
    BodyFwdLayout f;
    BodyBwdLayout w;
    if (int rc = body_layouts(body, &f, &w)) return rc;
    *fwd_bytes = f.bytes;
    *bwd_bytes = w.bytes;
    return 0;
}

int exa_mesh_body_forward(const ExaMeshBody* body, const float* coef, const float* joint_offset, void* fwd_ws,
                          uint64_t fwd_ws_bytes, float* mesh_upsampled, float* mesh, float* joint_neutral_pose,
                          float* transform_mat_neutral_pose, float* joint_zero_pose, void* stream) {
    if (int rc = body_check(body)) return rc;
    const ExaMeshBody& b = *body;
    BodyFwdLayout f;
    BodyBwdLayout w;
    if (int rc = body_layouts(body, &f, &w)) return rc;
    int32_t depth[BD_MAXJ];
    if (int rc = exa_mesh_kinematics_depths(b.J, b.parents, depth)) return rc;
    if (!coef || !joint_offset) return fail(EXA_MESH_E_NULLPTR, "coef / joint_offset is NULL");
    if (!b.v_base || !b.dirs || !b.weights) return fail(EXA_MESH_E_NULLPTR, "v_base / dirs / weights is NULL");
    if (!b.jreg_off || (b.nnz > 0 && (!b.jreg_col || !b.jreg_val)))
        return fail(EXA_MESH_E_NULLPTR, "jreg_off / jreg_col / jreg_val is NULL");
    if (!b.rot_pose || !b.rot_inverse || !b.rot_identity)
        return fail(EXA_MESH_E_NULLPTR, "rot_pose / rot_inverse / rot_identity is NULL");
    if (!mesh_upsampled || !mesh || !joint_neutral_pose || !transform_mat_neutral_pose || !joint_zero_pose)
        return fail(EXA_MESH_E_NULLPTR, "an output is NULL");
    if (!fwd_ws) return fail(EXA_MESH_E_NULLPTR, "fwd_ws (workspace) is NULL");
    if (fwd_ws_bytes < f.bytes) return fail(EXA_MESH_E_INVALID, "fwd_ws is smaller than exa_mesh_body_workspace_sizes");
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)fwd_ws;
    float* v_shaped = ws + f.v_shaped;
    float* v_posed = b.pose_offsets ? ws + f.v_posed : v_shaped;
    const int M = 3 * b.V;

    const ShapeParams S = {b.L, M, b.L, coef, nullptr, b.dirs, b.v_base, b.pose_offsets, v_shaped, ws + f.v_posed,
                           ws + f.zero3};
    if (int rc = launch_body_shape(S, st)) return rc;
    const JregParams R = {b.V, b.nnz, b.root, b.jreg_off, b.jreg_col, b.jreg_val, v_shaped, joint_offset, ws + f.Jr};
    if (int rc = launch_body_jreg(R, b.J, st)) return rc;
    if (int rc = exa_mesh_kinematics_forward(1, b.J, b.parents, nullptr, b.rot_pose, ws + f.Jr, nullptr, ws + f.A,
                                             joint_neutral_pose, ws + f.rot, stream))
        return rc;
    const float* pts[1] = {v_posed};
    float* outs[1] = {mesh};
    if (int rc = exa_skin_forward(b.V, 1, b.J, b.V, pts, b.weights, nullptr, ws + f.A, ws + f.zero3, nullptr, nullptr,
                                  outs, stream))
        return skin_failed(rc);
    if (int rc = up_forward(b.up, 3, mesh, mesh_upsampled, st)) return rc;
    if (int rc = exa_mesh_kinematics_forward(1, b.J, b.parents, nullptr, b.rot_inverse, joint_neutral_pose, nullptr,
                                             transform_mat_neutral_pose, ws + f.posed, ws + f.rot, stream))
        return rc;
    return exa_mesh_kinematics_forward(1, b.J, b.parents, nullptr, b.rot_identity, ws + f.Jr, nullptr, ws + f.T,
                                       joint_zero_pose, ws + f.rot, stream);
}

int exa_mesh_body_backward(const ExaMeshBody* body, const void* fwd_ws, uint64_t fwd_ws_bytes,
                           const float* joint_neutral_pose, const float* g_mesh_upsampled, const float* g_mesh,
                           const float* g_joint_neutral_pose, const float* g_transform_mat_neutral_pose,
                           const float* g_joint_zero_pose, void* bwd_ws, uint64_t bwd_ws_bytes, float* dL_dcoef,
                           float* dL_djoint_offset, void* stream) {
    if (int rc = body_check(body)) return rc;
    const ExaMeshBody& b = *body;
    BodyFwdLayout f;
    BodyBwdLayout w;
    if (int rc = body_layouts(body, &f, &w)) return rc;
    int32_t depth[BD_MAXJ];
    if (int rc = exa_mesh_kinematics_depths(b.J, b.parents, depth)) return rc;
    if (!dL_dcoef && !dL_djoint_offset) return 0;
    if (!b.dirs || !b.weights) return fail(EXA_MESH_E_NULLPTR, "dirs / weights is NULL");
    if (!b.jregT_off || (b.nnz > 0 && (!b.jregT_row || !b.jregT_val)))
        return fail(EXA_MESH_E_NULLPTR, "jregT_off / jregT_row / jregT_val is NULL");
    if (!b.rot_pose || !b.rot_inverse || !b.rot_identity)
        return fail(EXA_MESH_E_NULLPTR, "rot_pose / rot_inverse / rot_identity is NULL");
    if (!joint_neutral_pose) return fail(EXA_MESH_E_NULLPTR, "joint_neutral_pose is NULL");
    if (!fwd_ws || !bwd_ws) return fail(EXA_MESH_E_NULLPTR, "fwd_ws / bwd_ws (workspace) is NULL");
    if (fwd_ws_bytes < f.bytes) return fail(EXA_MESH_E_INVALID, "fwd_ws is smaller than exa_mesh_body_workspace_sizes");
    if (bwd_ws_bytes < w.bytes) return fail(EXA_MESH_E_INVALID, "bwd_ws is smaller than exa_mesh_body_workspace_sizes");
    hipStream_t st = (hipStream_t)stream;
    const float* fw = (const float*)fwd_ws;
    const float* v_posed = fw + (b.pose_offsets ? f.v_posed : f.v_shaped);
    const float* Jr = fw + f.Jr;
    char* base = (char*)bwd_ws;
    auto at = [base](uint64_t off) { return (float*)(base + off); };
    const int M = 3 * b.V, J3 = 3 * b.J;
    const bool have_mesh = g_mesh_upsampled || g_mesh;

    // chain B: what reaches the neutral-pose joints through transform_mat_neutral_pose
    if (g_transform_mat_neutral_pose) {
        if (int rc = exa_mesh_kinematics_backward(1, b.J, b.parents, nullptr, b.rot_inverse, joint_neutral_pose, nullptr,
                                                  g_transform_mat_neutral_pose, nullptr, nullptr, nullptr, at(w.gB),
                                                  nullptr, stream))
            return rc;
    }
    // the mesh's cotangent, and through the skinning to v_posed and to chain A's transforms
    if (have_mesh) {
        const float* gm = g_mesh;
        if (g_mesh_upsampled) {
            if (int rc = up_backward(b.up, 3, g_mesh_upsampled, g_mesh, at(w.up), w.up_bytes, at(w.gm), st)) return rc;
            gm = at(w.gm);
        }
        const float* pts[1] = {v_posed};
        const float* gouts[1] = {gm};
        float* gpts[1] = {dL_dcoef ? at(w.gvp) : nullptr};
        if (int rc = exa_skin_backward(b.V, 1, b.J, b.V, pts, b.weights, nullptr, fw + f.A, nullptr, gouts, gpts,
                                       at(w.gA), nullptr, at(w.skin), w.skin_bytes, stream))
            return skin_failed(rc);
    }
    const float* gpA = g_joint_neutral_pose;
    if (g_joint_neutral_pose && g_transform_mat_neutral_pose) {
        hipLaunchKernelGGL(body_add, dim3(ceil_div(J3, BD_BLOCK)), dim3(BD_BLOCK), 0, st, J3, g_joint_neutral_pose,
                           (const float*)at(w.gB), at(w.gpA));
        if (int rc = launched("body_add")) return rc;
        gpA = at(w.gpA);
    } else if (g_transform_mat_neutral_pose) {
        gpA = at(w.gB);
    }
    const float* gJA = nullptr;
    if (have_mesh || gpA) {
        if (int rc = exa_mesh_kinematics_backward(1, b.J, b.parents, nullptr, b.rot_pose, Jr, nullptr,
                                                  have_mesh ? at(w.gA) : nullptr, gpA, nullptr, nullptr, at(w.gJA),
                                                  nullptr, stream))
            return rc;
        gJA = at(w.gJA);
    }
    const float* gJC = nullptr;
    if (g_joint_zero_pose) {
        if (int rc = exa_mesh_kinematics_backward(1, b.J, b.parents, nullptr, b.rot_identity, Jr, nullptr, nullptr,
                                                  g_joint_zero_pose, nullptr, nullptr, at(w.gJC), nullptr, stream))
            return rc;
        gJC = at(w.gJC);
    }
    const JregBwdParams Q = {b.V, b.J, b.nnz, b.root, b.jregT_off, b.jregT_row, b.jregT_val, gJA, gJC,
                             (have_mesh && dL_dcoef) ? at(w.gvp) : nullptr, dL_djoint_offset,
                             dL_dcoef ? at(w.dvs) : nullptr};
    if (int rc = launch_body_jreg_bwd(Q, dL_dcoef != nullptr, st)) return rc;
    if (!dL_dcoef) return 0;
    const int chunks = (int)ceil_div(M, BD_CHUNK);
    const CoefParams C = {b.L, M, chunks, b.L, b.dirs, at(w.dvs), at(w.partial), dL_dcoef, nullptr};
    return launch_body_coef(C, st);
}

}  // extern "C"
