// The posed SMPL-X stage (include/exa_mesh.h, exa_mesh_posed_*): the reference's get_smplx_outputs (model.py:37-58), the
// smplx_layer call whose pose varies per frame.  The semantics -- the op-by-op fp32 forward and the order of every sum of
// the backward -- are written out in the header; this file implements them.
//
//   posed_rodrigues   one lane per joint: pose + pose_mean, smplx's batch_rodrigues, rot, (sin, cos) and the pose
//                     feature rot[1:] - I.
//   posed_finish      joints = posed joints + transl; vertices_world = Rinv (vertices - t).
//   posed_gvert       the vertices' cotangent: g_vertices + Rinv^T g_vertices_world.
//   posed_pose_bwd    one lane per joint: the cotangent of rot (the chain's and the correctives') through Rodrigues'
//                     formula to the pose; lane 0 also adds up dL/dtransl.
// The shape blend, the pose correctives (the same kernel over posedirs with the pose feature as coefficients), the joint
// regression, their backward passes and the two-level sums are body.hip's launches (body.h); the chain and the skinning
// are the library's own entry points (exa_mesh_kinematics_*, exa_skin_*), called on the caller's stream.  No atomics, no
// memsets, no allocation, no synchronisation.  Compiled with -ffp-contract=off (build.py): no product is contracted into
// a fused multiply-add.  sinf / cosf are the device library's: the one step that is not bit-equal to a CPU evaluation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "../../include/exa_mesh.h"
#include "../../include/exa_skin.h"
#include "abi_status.h"
#include "body.h"

namespace exa_mesh_impl {

using exa::align256;
using exa::ceil_div;

EXA_ABI_STATUS_SHARED("exa_mesh")         // exa_mesh_last_error() and its buffer are mesh_raster.hip's

constexpr int PB_BLOCK = 256;
constexpr int PB_MAXJ = EXA_MESH_KIN_MAX_JOINTS;
constexpr int PB_MAXL = EXA_MESH_BODY_MAX_COEF;
constexpr int64_t PB_MAXV = EXA_MESH_BODY_MAX_VERTS;
constexpr int PB_CHUNK = EXA_MESH_BODY_CHUNK;
constexpr float PB_EPS = 1e-8f;
static_assert(PB_MAXJ == 64, "one lane per joint");

// what the forward and the backward of Rodrigues' formula share: the header's steps 1 and 2 up to the angle
struct RodRow {
    float f[3], e[3], a, d[3], K[9], KK[9];
};

__device__ __forceinline__ void rod_row(const float* pose, const float* mean, int j, RodRow& r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float f = pose[3 * j + c];
        if (mean) f = f + mean[3 * j + c];
        r.f[c] = f;
        r.e[c] = f + PB_EPS;
    }
    r.a = sqrtf((r.e[0] * r.e[0] + r.e[1] * r.e[1]) + r.e[2] * r.e[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) r.d[c] = r.f[c] / r.a;
    const float K[9] = {0.0f, -r.d[2], r.d[1], r.d[2], 0.0f, -r.d[0], -r.d[1], r.d[0], 0.0f};
#pragma unroll
    for (int k = 0; k < 9; ++k) r.K[k] = K[k];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            r.KK[3 * i + c] = (K[3 * i + 0] * K[0 + c] + K[3 * i + 1] * K[3 + c]) + K[3 * i + 2] * K[6 + c];
}

struct RodParams {
    int32_t J;
    const float* pose;
    const float* mean;                        // [J, 3] or NULL
    float* sincos;                            // [J, 2]
    float* rot;                               // [J, 3, 3]
    float* feat;                              // [9 (J - 1)]
};

__global__ __launch_bounds__(64) void posed_rodrigues(RodParams P) {
    const int j = threadIdx.x;
    if (j >= P.J) return;
    RodRow r;
    rod_row(P.pose, P.mean, j, r);
    const float s = sinf(r.a), c = cosf(r.a);
    const float m = 1.0f - c;
    P.sincos[2 * j] = s;
    P.sincos[2 * j + 1] = c;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float eye = (k == 0 || k == 4 || k == 8) ? 1.0f : 0.0f;
        const float R = (eye + s * r.K[k]) + m * r.KK[k];
        P.rot[9 * j + k] = R;
        if (j >= 1) P.feat[9 * (j - 1) + k] = R - eye;
    }
}

struct FinishParams {
    int32_t V, J;
    const float* posed;                       // [J, 3]
    const float* transl;                      // [3]
    const float* vertices;                    // [V, 3]
    const float* Rinv;                        // [3, 3] or NULL
    const float* t;                           // [3]
    float* joints;                            // [J, 3]
    float* world;                             // [V, 3]
};

__global__ __launch_bounds__(PB_BLOCK) void posed_finish(FinishParams P) {
    const int i = blockIdx.x * PB_BLOCK + threadIdx.x;
    if (i < 3 * P.J) P.joints[i] = P.posed[i] + P.transl[i % 3];
    if (!P.Rinv || i >= P.V) return;
    const float* x = P.vertices + 3 * (int64_t)i;
    const float d0 = x[0] - P.t[0], d1 = x[1] - P.t[1], d2 = x[2] - P.t[2];
    const float* R = P.Rinv;
#pragma unroll
    for (int r = 0; r < 3; ++r) P.world[3 * (int64_t)i + r] = (R[r * 3 + 0] * d0 + R[r * 3 + 1] * d1) + R[r * 3 + 2] * d2;
}

struct GvertParams {
    int32_t V;
    const float* g_vertices;                  // [V, 3] or NULL
    const float* g_world;                     // [V, 3]
    const float* Rinv;
    float* gv;
};

__global__ __launch_bounds__(PB_BLOCK) void posed_gvert(GvertParams P) {
    const int v = blockIdx.x * PB_BLOCK + threadIdx.x;
    if (v >= P.V) return;
    const float* g = P.g_world + 3 * (int64_t)v;
    const float g0 = g[0], g1 = g[1], g2 = g[2];
    const float* R = P.Rinv;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float gp = (R[0 * 3 + c] * g0 + R[1 * 3 + c] * g1) + R[2 * 3 + c] * g2;
        P.gv[3 * (int64_t)v + c] = P.g_vertices ? P.g_vertices[3 * (int64_t)v + c] + gp : gp;
    }
}

struct PoseBwdParams {
    int32_t J;
    const float* pose;
    const float* mean;
    const float* sincos;
    const float* grot;                        // [J, 3, 3] or NULL
    const float* gfeat;                       // [9 (J - 1)] or NULL
    float* dpose;                             // [J, 3] or NULL
    const float* gtrans;                      // [3] the skinning's, or NULL
    const float* g_joints;                    // [J, 3] or NULL
    float* dtransl;                           // [3] or NULL
};

__global__ __launch_bounds__(64) void posed_pose_bwd(PoseBwdParams P) {
    const int j = threadIdx.x;
    if (j == 0 && P.dtransl) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float t = 0.0f;
            if (P.g_joints)
                for (int i = 0; i < P.J; ++i) t = t + P.g_joints[3 * i + c];
            P.dtransl[c] = (P.gtrans && P.g_joints) ? P.gtrans[c] + t : P.gtrans ? P.gtrans[c] : t;
        }
    }
    if (j >= P.J || !P.dpose) return;
    RodRow r;
    rod_row(P.pose, P.mean, j, r);
    const float s = P.sincos[2 * j], c = P.sincos[2 * j + 1];
    const float m = 1.0f - c;
    const bool corr = P.gfeat && j >= 1;
    float G[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        float g = P.grot ? P.grot[9 * j + k] : 0.0f;
        if (corr) g = P.grot ? g + P.gfeat[9 * (j - 1) + k] : P.gfeat[9 * (j - 1) + k];
        G[k] = g;
    }
    float gs = 0.0f, gm = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        gs = gs + G[k] * r.K[k];
        gm = gm + G[k] * r.KK[k];
    }
    float gK[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float GKt = (G[3 * i + 0] * r.K[3 * k + 0] + G[3 * i + 1] * r.K[3 * k + 1]) + G[3 * i + 2] * r.K[3 * k + 2];
            const float KtG = (r.K[0 + i] * G[0 + k] + r.K[3 + i] * G[3 + k]) + r.K[6 + i] * G[6 + k];
            gK[3 * i + k] = s * G[3 * i + k] + m * (GKt + KtG);
        }
    const float gd[3] = {gK[7] - gK[5], gK[2] - gK[6], gK[3] - gK[1]};
    const float dot = (gd[0] * r.d[0] + gd[1] * r.d[1]) + gd[2] * r.d[2];
    const float ga = (gs * c + gm * s) - dot / r.a;
#pragma unroll
    for (int k = 0; k < 3; ++k) P.dpose[3 * j + k] = gd[k] / r.a + ga * (r.e[k] / r.a);
}

// the forward's workspace, in floats from its start (every section on a 256-byte boundary; sincos comes first)
struct PosedFwdLayout {
    uint64_t sincos, rot, feat, v_shaped, v_posed, Jr, A, posed, bytes;
};

// the backward's, in bytes
struct PosedBwdLayout {
    uint64_t gv, gvp, gA, gtrans, grot, gJ, dvs, gfeat, skin, partial, bytes;
    uint64_t skin_bytes;
};

int posed_check(const ExaMeshPosed* b) {
    if (!b) return fail(EXA_MESH_E_NULLPTR, "posed (the descriptor) is NULL");
    if (b->V < 1 || (int64_t)b->V > PB_MAXV) return fail(EXA_MESH_E_INVALID, "V (vertices) must be 1 .. 2^24");
    if (b->L < 1 || b->L > PB_MAXL) return fail(EXA_MESH_E_INVALID, "L (coefficients) must be 1 .. 512");
    if (b->J < 1 || b->J > PB_MAXJ) return fail(EXA_MESH_E_INVALID, "J (joints) must be 1 .. 64");
    if (b->nnz < 0 || (int64_t)b->nnz > (int64_t)b->J * b->V)
        return fail(EXA_MESH_E_INVALID, "nnz (regressor non-zeros) must be 0 .. J V");
    return 0;
}

int posed_layouts(const ExaMeshPosed* b, PosedFwdLayout* f, PosedBwdLayout* w) {
    const uint64_t V3 = 3 * (uint64_t)b->V, J = (uint64_t)b->J, F = sizeof(float);
    const uint64_t P = 9 * (J - 1);
    uint64_t at = 0;
    auto take = [&at](uint64_t bytes) {
        const uint64_t here = at;
        at += align256(bytes);
        return here;
    };
    f->sincos = take(2 * J * F) / F;
    f->rot = take(9 * J * F) / F;
    f->feat = take(std::max<uint64_t>(P, 1) * F) / F;
    f->v_shaped = take(V3 * F) / F;
    f->v_posed = take(V3 * F) / F;
    f->Jr = take(3 * J * F) / F;
    f->A = take(16 * J * F) / F;
    f->posed = take(3 * J * F) / F;
    f->bytes = at;
    uint64_t skin = 0;
    if (exa_skin_workspace_size(b->V, b->J, &skin) != 0)
        return fail(EXA_MESH_E_INVALID, "the skinning refuses these sizes (exa_skin_workspace_size)");
    at = 0;
    w->gv = take(V3 * F);
    w->gvp = take(V3 * F);
    w->gA = take(16 * J * F);
    w->gtrans = take(3 * F);
    w->grot = take(9 * J * F);
    w->gJ = take(3 * J * F);
    w->dvs = take(V3 * F);
    w->gfeat = take(std::max<uint64_t>(P, 1) * F);
    w->skin_bytes = skin;
    w->skin = take(skin);
    w->partial = take((uint64_t)ceil_div((int64_t)V3, PB_CHUNK) * std::max<uint64_t>((uint64_t)b->L, P) * F);
    w->bytes = at;
    return 0;
}

// everything both directions check before any GPU work
int posed_common(const ExaMeshPosed* b, int32_t Lb, PosedFwdLayout* f, PosedBwdLayout* w) {
    if (int rc = posed_check(b)) return rc;
    if (Lb < 0 || Lb > b->L) return fail(EXA_MESH_E_INVALID, "Lb (betas) must be 0 .. L");
    if (!b->parents) return fail(EXA_MESH_E_NULLPTR, "parents is NULL");
    int32_t depth[PB_MAXJ];
    if (int rc = exa_mesh_kinematics_depths(b->J, b->parents, depth)) return rc;
    if (!b->v_base || !b->dirs || !b->weights) return fail(EXA_MESH_E_NULLPTR, "v_base / dirs / weights is NULL");
    if (b->J > 1 && !b->posedirs) return fail(EXA_MESH_E_NULLPTR, "posedirs is NULL");
    return posed_layouts(b, f, w);
}

}  // namespace exa_mesh_impl

using namespace exa_mesh_impl;

extern "C" {

int exa_mesh_posed_workspace_sizes(const ExaMeshPosed* posed, uint64_t* fwd_bytes, uint64_t* bwd_bytes) {
    if (int rc = posed_check(posed)) return rc;
    if (!fwd_bytes || !bwd_bytes) return fail(EXA_MESH_E_NULLPTR, "fwd_bytes / bwd_bytes is NULL");
    PosedFwdLayout f;
    PosedBwdLayout w;
    if (int rc = posed_layouts(posed, &f, &w)) return rc;
    *fwd_bytes = f.bytes;
    *bwd_bytes = w.bytes;
    return 0;
}

int exa_mesh_posed_forward(const ExaMeshPosed* posed, int32_t Lb, const float* pose, const float* betas,
                           const float* expression, const float* transl, const float* joint_offset, const float* Rinv,
                           const float* t, void* fwd_ws, uint64_t fwd_ws_bytes, float* vertices, float* joints,
                           float* vertices_world, float* rot, void* stream) {
    PosedFwdLayout f;
    PosedBwdLayout w;
    if (int rc = posed_common(posed, Lb, &f, &w)) return rc;
    const ExaMeshPosed& b = *posed;
    if (!b.jreg_off || (b.nnz > 0 && (!b.jreg_col || !b.jreg_val)))
        return fail(EXA_MESH_E_NULLPTR, "jreg_off / jreg_col / jreg_val is NULL");
    if (!pose || !transl) return fail(EXA_MESH_E_NULLPTR, "pose / transl is NULL");
    if ((Lb > 0 && !betas) || (Lb < b.L && !expression)) return fail(EXA_MESH_E_NULLPTR, "betas / expression is NULL");
    if (!Rinv != !t) return fail(EXA_MESH_E_INVALID, "Rinv and t must be given together");
    if (!Rinv != !vertices_world) return fail(EXA_MESH_E_INVALID, "vertices_world needs Rinv and t, and they need it");
    if (!vertices || !joints || !rot) return fail(EXA_MESH_E_NULLPTR, "vertices / joints / rot is NULL");
    if (!fwd_ws) return fail(EXA_MESH_E_NULLPTR, "fwd_ws (workspace) is NULL");
    if (fwd_ws_bytes < f.bytes) return fail(EXA_MESH_E_INVALID, "fwd_ws is smaller than exa_mesh_posed_workspace_sizes");
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)fwd_ws;
    const int M = 3 * b.V, P = 9 * (b.J - 1);
    float* v_shaped = ws + f.v_shaped;
    float* v_posed = b.J > 1 ? ws + f.v_posed : v_shaped;

    const RodParams R = {b.J, pose, b.pose_mean, ws + f.sincos, ws + f.rot, ws + f.feat};
    hipLaunchKernelGGL(posed_rodrigues, dim3(1), dim3(64), 0, st, R);
    if (int rc = launched("posed_rodrigues")) return rc;
    const ShapeParams S = {b.L, M, Lb, betas, expression, b.dirs, b.v_base, nullptr, v_shaped, nullptr, nullptr};
    if (int rc = launch_body_shape(S, st)) return rc;
    const JregParams Q = {b.V, b.nnz, -1, b.jreg_off, b.jreg_col, b.jreg_val, v_shaped, joint_offset, ws + f.Jr};
    if (int rc = launch_body_jreg(Q, b.J, st)) return rc;
    if (b.J > 1) {                            // the pose correctives: the same sum over posedirs, from the pose feature
        const ShapeParams C = {P, M, P, ws + f.feat, nullptr, b.posedirs, v_shaped, nullptr, v_posed, nullptr, nullptr};
        if (int rc = launch_body_shape(C, st)) return rc;
    }
    if (int rc = exa_mesh_kinematics_forward(1, b.J, b.parents, nullptr, ws + f.rot, ws + f.Jr, nullptr, ws + f.A,
                                             ws + f.posed, rot, stream))
        return rc;
    const float* pts[1] = {v_posed};
    float* outs[1] = {vertices};
    if (int rc = exa_skin_forward(b.V, 1, b.J, b.V, pts, b.weights, nullptr, ws + f.A, transl, nullptr, nullptr, outs,
                                  stream))
        return skin_failed(rc);
    const FinishParams E = {b.V, b.J, ws + f.posed, transl, vertices, Rinv, t, joints, vertices_world};
    hipLaunchKernelGGL(posed_finish, dim3(ceil_div(Rinv ? std::max(b.V, 3 * b.J) : 3 * b.J, PB_BLOCK)), dim3(PB_BLOCK), 0,
                       st, E);
    return launched("posed_finish");
}

int exa_mesh_posed_backward(const ExaMeshPosed* posed, int32_t Lb, const float* pose, const float* Rinv,
                            const void* fwd_ws, uint64_t fwd_ws_bytes, const float* g_vertices, const float* g_joints,
                            const float* g_vertices_world, void* bwd_ws, uint64_t bwd_ws_bytes, float* dL_dpose,
                            float* dL_dbetas, float* dL_dexpression, float* dL_dtransl, float* dL_djoint_offset,
                            void* stream) {
    PosedFwdLayout f;
    PosedBwdLayout w;
    if (int rc = posed_common(posed, Lb, &f, &w)) return rc;
    const ExaMeshPosed& b = *posed;
    if (Lb == 0) dL_dbetas = nullptr;         // nothing to write
    if (Lb == b.L) dL_dexpression = nullptr;
    const bool want_coef = dL_dbetas || dL_dexpression;
    const bool want_chain = dL_dpose || want_coef || dL_djoint_offset;
    if (!want_chain && !dL_dtransl) return 0;
    const bool have_mesh = g_vertices || g_vertices_world;
    if (!b.jregT_off || (b.nnz > 0 && (!b.jregT_row || !b.jregT_val)))
        return fail(EXA_MESH_E_NULLPTR, "jregT_off / jregT_row / jregT_val is NULL");
    if (dL_dpose && !pose) return fail(EXA_MESH_E_NULLPTR, "pose is NULL");
    if (g_vertices_world && !Rinv) return fail(EXA_MESH_E_NULLPTR, "g_vertices_world needs Rinv");
    if (!fwd_ws || !bwd_ws) return fail(EXA_MESH_E_NULLPTR, "fwd_ws / bwd_ws (workspace) is NULL");
    if (fwd_ws_bytes < f.bytes) return fail(EXA_MESH_E_INVALID, "fwd_ws is smaller than exa_mesh_posed_workspace_sizes");
    if (bwd_ws_bytes < w.bytes) return fail(EXA_MESH_E_INVALID, "bwd_ws is smaller than exa_mesh_posed_workspace_sizes");
    hipStream_t st = (hipStream_t)stream;
    const float* fw = (const float*)fwd_ws;
    const float* v_posed = fw + (b.J > 1 ? f.v_posed : f.v_shaped);
    char* base = (char*)bwd_ws;
    auto at = [base](uint64_t off) { return (float*)(base + off); };
    const int M = 3 * b.V, P = 9 * (b.J - 1);
    const int chunks = (int)ceil_div(M, PB_CHUNK);
    const bool corr = dL_dpose && have_mesh && b.J > 1;       // the correctives carry a cotangent to the pose
    const bool want_gvp = have_mesh && (corr || want_coef);

    // the vertices' cotangent, and through the skinning to v_posed, to the transforms and to transl
    if (have_mesh) {
        const float* gv = g_vertices;
        if (g_vertices_world) {
            const GvertParams G = {b.V, g_vertices, g_vertices_world, Rinv, at(w.gv)};
            hipLaunchKernelGGL(posed_gvert, dim3(ceil_div(b.V, PB_BLOCK)), dim3(PB_BLOCK), 0, st, G);
            if (int rc = launched("posed_gvert")) return rc;
            gv = at(w.gv);
        }
        const float* pts[1] = {v_posed};
        const float* gouts[1] = {gv};
        float* gpts[1] = {want_gvp ? at(w.gvp) : nullptr};
        if (int rc = exa_skin_backward(b.V, 1, b.J, b.V, pts, b.weights, nullptr, fw + f.A, nullptr, gouts, gpts,
                                       want_chain ? at(w.gA) : nullptr, dL_dtransl ? at(w.gtrans) : nullptr, at(w.skin),
                                       w.skin_bytes, stream))
            return skin_failed(rc);
    }
    const bool kin = want_chain && (have_mesh || g_joints);
    const bool want_gJ = want_coef || dL_djoint_offset;
    if (kin) {
        if (int rc = exa_mesh_kinematics_backward(1, b.J, b.parents, nullptr, fw + f.rot, fw + f.Jr, nullptr,
                                                  have_mesh ? at(w.gA) : nullptr, g_joints, nullptr,
                                                  dL_dpose ? at(w.grot) : nullptr, want_gJ ? at(w.gJ) : nullptr, nullptr,
                                                  stream))
            return rc;
    }
    if (want_gJ) {
        const JregBwdParams Q = {b.V, b.J, b.nnz, -1, b.jregT_off, b.jregT_row, b.jregT_val, kin ? at(w.gJ) : nullptr,
                                 nullptr, (have_mesh && want_coef) ? at(w.gvp) : nullptr, dL_djoint_offset,
                                 want_coef ? at(w.dvs) : nullptr};
        if (int rc = launch_body_jreg_bwd(Q, want_coef, st)) return rc;
    }
    if (want_coef) {                          // the rows of the wanted coefficients only
        const int l0 = dL_dbetas ? 0 : Lb, l1 = dL_dexpression ? b.L : Lb;
        const CoefParams C = {l1 - l0, M, chunks, Lb - l0, b.dirs + (int64_t)l0 * M, at(w.dvs), at(w.partial), dL_dbetas,
                              dL_dexpression};
        if (int rc = launch_body_coef(C, st)) return rc;
    }
    if (corr) {                               // the correctives' transpose: 3 V terms per pose feature
        const CoefParams C = {P, M, chunks, P, b.posedirs, at(w.gvp), at(w.partial), at(w.gfeat), nullptr};
        if (int rc = launch_body_coef(C, st)) return rc;
    }
    if (!dL_dpose && !dL_dtransl) return 0;
    const PoseBwdParams B = {b.J, pose, b.pose_mean, fw + f.sincos, (dL_dpose && kin) ? at(w.grot) : nullptr,
                             corr ? at(w.gfeat) : nullptr, dL_dpose, (dL_dtransl && have_mesh) ? at(w.gtrans) : nullptr,
                             g_joints, dL_dtransl};
    hipLaunchKernelGGL(posed_pose_bwd, dim3(1), dim3(64), 0, st, B);
    return launched("posed_pose_bwd");
}

}  // extern "C"
