// Forward kinematics (include/exa_mesh.h, exa_mesh_kinematics_*): the pose -> joint-transform chain of the reference's
// get_transform_mat_joint (module.py:389-411) -- axis_angle_to_matrix, smplx's batch_rigid_transform (lbs.py:361-417)
// and the bmm with the big-pose transforms -- and its backward.  The semantics -- the op-by-op fp32 forward, the level
// order and the order of every sum of the backward -- are written out in the header; this file implements them.
//
//   kin_fwd   one workgroup of one wave per skeleton, lane j = joint j.  The lane forms its rotation and its local
//             translation, then the world transforms are composed level by level through LDS (a lane of depth d reads
//             its parent's three rows, written at depth d - 1, and writes its own), one barrier per level; the rest
//             location is removed and `pre` applied in registers.
//   kin_bwd   the same shape.  It recomputes the world transforms as kin_fwd does, seeds every joint's dL/dW from the
//             incoming gradients, then walks the levels from the deepest to the root: the lanes of depth d leave
//             dL/dW_child L_child^T in LDS and, after the barrier, every parent adds its children's in ascending child
//             index (a first-child / next-sibling list the host made from `parents`).  dL/dL = W_parent^T dL/dW, the
//             joint gradients meet through LDS in the same child order, and the axis-angle Jacobian runs in registers.
// The tree (parent, depth, first child, next sibling: 64 int8 each) travels BY VALUE in the argument block: no device
// buffer, no copy, no state between calls.  No atomics, no memsets, no workspace: every output element is one lane's
// value in the header's order.  Compiled with -ffp-contract=off (build.py): no product is contracted into a fused
// multiply-add.  sinf / cosf are the device library's: the one step that is not bit-equal to a CPU evaluation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/exa_mesh.h"
#include "abi_status.h"
#include "axis_angle.h"

namespace exa_mesh_impl {

EXA_ABI_STATUS_SHARED("exa_mesh")         // exa_mesh_last_error() and its buffer are mesh_raster.hip's

constexpr int KJ = EXA_MESH_KIN_MAX_JOINTS;
constexpr int KLD = 13;                       // LDS stride of a joint's 3 x 4 rows (odd: lanes do not share a bank)
constexpr int KIN_MAX_B = 1 << 20;            // skeletons per launch
static_assert(KJ == 64, "one lane of one wave per joint");

struct KinTree {
    int8_t parent[KJ];                        // -1 for the root
    int8_t depth[KJ];
    int8_t first_child[KJ];                   // smallest i with parent[i] == j, -1 without children
    int8_t next_sibling[KJ];                  // smallest i > j with parent[i] == parent[j], -1 for the last child
    int32_t max_depth;
};

struct KinFwdParams {
    int32_t J;
    const float* pose;                        // exactly one of pose / rot_in
    const float* rot_in;
    const float* joints;
    const float* pre;                         // NULL: out = A
    float* transforms;
    float* posed;
    float* rot;
    KinTree tree;
};

struct KinBwdParams {
    int32_t J;
    const float* pose;                        // needed for g_pose only
    const float* rot;
    const float* joints;
    const float* pre;
    const float* g_transforms;                // NULL: zero
    const float* g_posed;                     // NULL: zero
    float* g_pose;
    float* g_rot;
    float* g_joints;
    float* g_pre;
    KinTree tree;
};

// Step 1 of the header -- the quaternion of an axis-angle vector, its matrix and the analytic backward -- is
// axis_angle.h (shared with fit_terms.hip).
using exa::aa_backward;
using exa::aa_quaternion;
using exa::quaternion_matrix;

// Steps 2 and 3 of the header, shared by both kernels: t = the local translation, W = the lane's world transform (rows
// 0-2, W[r * 4 + c]); on return every joint's W is in Wl and every joint's rest location in jl.
__device__ __forceinline__ void kin_world(int max_depth, bool live, int j, int par, int dep, const float* R,
                                          const float* jt, float* Wl, float* jl, float* W, float* t) {
    if (live) {
#pragma unroll
        for (int c = 0; c < 3; ++c) jl[j * 3 + c] = jt[c];
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c] = par >= 0 ? jt[c] - jl[par * 3 + c] : jt[c];
        if (dep == 0) {
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) W[r * 4 + c] = R[r * 3 + c];
                W[r * 4 + 3] = t[r];
            }
#pragma unroll
            for (int q = 0; q < 12; ++q) Wl[j * KLD + q] = W[q];
        }
    }
    for (int d = 1; d <= max_depth; ++d) {
        __syncthreads();
        if (live && dep == d) {
            float Wp[12];
#pragma unroll
            for (int q = 0; q < 12; ++q) Wp[q] = Wl[par * KLD + q];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    W[r * 4 + c] = (Wp[r * 4 + 0] * R[0 * 3 + c] + Wp[r * 4 + 1] * R[1 * 3 + c]) + Wp[r * 4 + 2] * R[2 * 3 + c];
                W[r * 4 + 3] = ((Wp[r * 4 + 0] * t[0] + Wp[r * 4 + 1] * t[1]) + Wp[r * 4 + 2] * t[2]) + Wp[r * 4 + 3];
            }
#pragma unroll
            for (int q = 0; q < 12; ++q) Wl[j * KLD + q] = W[q];
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(KJ) void kin_fwd(KinFwdParams P) {
    __shared__ float Wl[KJ * KLD];
    __shared__ float jl[KJ * 3];
    const int j = threadIdx.x;
    const bool live = j < P.J;
    const int64_t bj = (int64_t)blockIdx.x * P.J + j;
    const int par = live ? P.tree.parent[j] : -1, dep = live ? P.tree.depth[j] : -1;
    float R[9], jt[3], W[12], t[3];
#pragma unroll
    for (int q = 0; q < 12; ++q) W[q] = 0.0f;
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = 0.0f;
    jt[0] = jt[1] = jt[2] = t[0] = t[1] = t[2] = 0.0f;
    if (live) {
        if (P.pose) {
            quaternion_matrix(aa_quaternion(P.pose[bj * 3 + 0], P.pose[bj * 3 + 1], P.pose[bj * 3 + 2]), R);
        } else {
#pragma unroll
            for (int q = 0; q < 9; ++q) R[q] = P.rot_in[bj * 9 + q];
        }
#pragma unroll
        for (int q = 0; q < 9; ++q) P.rot[bj * 9 + q] = R[q];
#pragma unroll
        for (int c = 0; c < 3; ++c) jt[c] = P.joints[bj * 3 + c];
    }
    kin_world(P.tree.max_depth, live, j, par, dep, R, jt, Wl, jl, W, t);
    if (!live) return;
    float A[16];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        P.posed[bj * 3 + r] = W[r * 4 + 3];
#pragma unroll
        for (int c = 0; c < 3; ++c) A[r * 4 + c] = W[r * 4 + c];
        A[r * 4 + 3] = W[r * 4 + 3] - ((W[r * 4 + 0] * jt[0] + W[r * 4 + 1] * jt[1]) + W[r * 4 + 2] * jt[2]);
    }
    A[12] = A[13] = A[14] = 0.0f;
    A[15] = 1.0f;
    float* out = P.transforms + bj * 16;
    if (P.pre) {
        float p[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) p[q] = P.pre[bj * 16 + q];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                out[r * 4 + c] = ((A[r * 4 + 0] * p[0 * 4 + c] + A[r * 4 + 1] * p[1 * 4 + c]) + A[r * 4 + 2] * p[2 * 4 + c]) +
                                 A[r * 4 + 3] * p[3 * 4 + c];
#pragma unroll
        for (int c = 0; c < 4; ++c) out[12 + c] = p[12 + c];
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) out[q] = A[q];
    }
}

__global__ __launch_bounds__(KJ) void kin_bwd(KinBwdParams P) {
    __shared__ float Wl[KJ * KLD];
    __shared__ float Cl[KJ * KLD];            // dL/dW_child L_child^T, then (first three of a row) dL/dt
    __shared__ float jl[KJ * 3];
    __shared__ int nsl[KJ];
    const int j = threadIdx.x;
    const bool live = j < P.J;
    const int64_t bj = (int64_t)blockIdx.x * P.J + j;
    const int par = live ? P.tree.parent[j] : -1, dep = live ? P.tree.depth[j] : -1;
    const int fc = live ? P.tree.first_child[j] : -1;
    nsl[j] = live ? P.tree.next_sibling[j] : -1;
    float R[9], jt[3], W[12], t[3];
#pragma unroll
    for (int q = 0; q < 12; ++q) W[q] = 0.0f;
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = 0.0f;
    jt[0] = jt[1] = jt[2] = t[0] = t[1] = t[2] = 0.0f;
    if (live) {
#pragma unroll
        for (int q = 0; q < 9; ++q) R[q] = P.rot[bj * 9 + q];
#pragma unroll
        for (int c = 0; c < 3; ++c) jt[c] = P.joints[bj * 3 + c];
    }
    kin_world(P.tree.max_depth, live, j, par, dep, R, jt, Wl, jl, W, t);

    // dL/dA (rows 0-2) from dL/dtransforms, and dL/dpre
    float g[16], GA[12];
#pragma unroll
    for (int q = 0; q < 16; ++q) g[q] = (live && P.g_transforms) ? P.g_transforms[bj * 16 + q] : 0.0f;
    if (P.pre) {
        float p[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) p[q] = live ? P.pre[bj * 16 + q] : 0.0f;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                GA[r * 4 + k] = ((g[r * 4 + 0] * p[k * 4 + 0] + g[r * 4 + 1] * p[k * 4 + 1]) + g[r * 4 + 2] * p[k * 4 + 2]) +
                                g[r * 4 + 3] * p[k * 4 + 3];
    } else {
#pragma unroll
        for (int q = 0; q < 12; ++q) GA[q] = g[q];
    }
    if (P.g_pre && live) {
        float A3[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            A3[r] = W[r * 4 + 3] - ((W[r * 4 + 0] * jt[0] + W[r * 4 + 1] * jt[1]) + W[r * 4 + 2] * jt[2]);
        float* gpre = P.g_pre + bj * 16;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                gpre[k * 4 + c] = (W[0 * 4 + k] * g[0 * 4 + c] + W[1 * 4 + k] * g[1 * 4 + c]) + W[2 * 4 + k] * g[2 * 4 + c];
            gpre[12 + c] = ((A3[0] * g[0 * 4 + c] + A3[1] * g[1 * 4 + c]) + A3[2] * g[2 * 4 + c]) + g[12 + c];
        }
    }
    // the joint's own dL/dW: the rest-location step and posed_joints
    float GW[12], rest[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float gp = (live && P.g_posed) ? P.g_posed[bj * 3 + r] : 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) GW[r * 4 + c] = GA[r * 4 + c] - GA[r * 4 + 3] * jt[c];
        GW[r * 4 + 3] = GA[r * 4 + 3] + gp;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        rest[c] = (GA[0 * 4 + 3] * W[0 * 4 + c] + GA[1 * 4 + 3] * W[1 * 4 + c]) + GA[2 * 4 + 3] * W[2 * 4 + c];

    // deepest level first: children leave dL/dW_child L_child^T, parents add them in ascending child index
    for (int d = P.tree.max_depth; d >= 1; --d) {
        if (live && dep == d) {
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    Cl[j * KLD + r * 4 + k] = ((GW[r * 4 + 0] * R[k * 3 + 0] + GW[r * 4 + 1] * R[k * 3 + 1]) +
                                               GW[r * 4 + 2] * R[k * 3 + 2]) + GW[r * 4 + 3] * t[k];
                Cl[j * KLD + r * 4 + 3] = GW[r * 4 + 3];
            }
        }
        __syncthreads();
        if (live && dep == d - 1) {
            for (int c = fc; c >= 0; c = nsl[c]) {
#pragma unroll
                for (int q = 0; q < 12; ++q) GW[q] = GW[q] + Cl[c * KLD + q];
            }
        }
    }
    // dL/dL = W_parent^T dL/dW (the root's W is its L)
    float GL[12];
    if (par >= 0) {
        float Wp[12];
#pragma unroll
        for (int q = 0; q < 12; ++q) Wp[q] = Wl[par * KLD + q];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                GL[k * 4 + c] = (Wp[0 * 4 + k] * GW[0 * 4 + c] + Wp[1 * 4 + k] * GW[1 * 4 + c]) + Wp[2 * 4 + k] * GW[2 * 4 + c];
    } else {
#pragma unroll
        for (int q = 0; q < 12; ++q) GL[q] = GW[q];
    }
    float GR[9];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) GR[k * 3 + c] = GL[k * 4 + c];
    if (P.g_rot && live) {
#pragma unroll
        for (int q = 0; q < 9; ++q) P.g_rot[bj * 9 + q] = GR[q];
    }
    if (P.g_joints) {
        __syncthreads();                      // every parent has read its children's Cl rows
        if (live) {
#pragma unroll
            for (int k = 0; k < 3; ++k) Cl[j * KLD + k] = GL[k * 4 + 3];
        }
        __syncthreads();
        if (live) {
            float gj[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) gj[c] = -rest[c] + GL[c * 4 + 3];
            for (int ch = fc; ch >= 0; ch = nsl[ch]) {
#pragma unroll
                for (int c = 0; c < 3; ++c) gj[c] = gj[c] - Cl[ch * KLD + c];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) P.g_joints[bj * 3 + c] = gj[c];
        }
    }
    if (P.g_pose && live) {
        float gp[3];
        aa_backward(P.pose[bj * 3 + 0], P.pose[bj * 3 + 1], P.pose[bj * 3 + 2], GR, gp);
#pragma unroll
        for (int c = 0; c < 3; ++c) P.g_pose[bj * 3 + c] = gp[c];
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

// Validates the tree and fills `tree` (and `depth_out`, when given).
int kin_tree(int32_t J, const int32_t* parents, KinTree* tree, int32_t* depth_out) {
    if (J < 1 || J > KJ) return fail(EXA_MESH_E_INVALID, "J (joints) must be 1 .. 64");
    if (!parents) return fail(EXA_MESH_E_NULLPTR, "parents is NULL");
    if (parents[0] != -1) return fail(EXA_MESH_E_INVALID, "parents[0] must be -1 (joint 0 is the root)");
    for (int i = 1; i < J; ++i) {
        if (parents[i] < 0 || parents[i] >= i) {
            char what[96];
            snprintf(what, sizeof(what), "parents[%d] = %d must lie in [0, %d): parents come before their children", i,
                     (int)parents[i], i);
            return fail(EXA_MESH_E_INVALID, what);
        }
    }
    int depth[KJ];
    int max_depth = 0;
    for (int i = 0; i < J; ++i) {
        depth[i] = i == 0 ? 0 : depth[parents[i]] + 1;
        if (depth[i] > max_depth) max_depth = depth[i];
        if (depth_out) depth_out[i] = depth[i];
    }
    if (tree) {
        for (int i = 0; i < KJ; ++i) {
            tree->parent[i] = -1;
            tree->depth[i] = 0;
            tree->first_child[i] = -1;
            tree->next_sibling[i] = -1;
        }
        tree->max_depth = max_depth;
        for (int i = J - 1; i >= 1; --i) {    // descending: the lists end up ascending
            const int p = parents[i];
            tree->parent[i] = (int8_t)p;
            tree->depth[i] = (int8_t)depth[i];
            tree->next_sibling[i] = tree->first_child[p];
            tree->first_child[p] = (int8_t)i;
        }
    }
    return 0;
}

int kin_check_batch(int32_t B) {
    if (B < 0) return fail(EXA_MESH_E_INVALID, "negative size");
    if (B > KIN_MAX_B) return fail(EXA_MESH_E_INVALID, "B (skeletons) exceeds 2^20");
    return 0;
}

}  // namespace exa_mesh_impl

using namespace exa_mesh_impl;

extern "C" {

int exa_mesh_kinematics_depths(int32_t J, const int32_t* parents, int32_t* depth_out) {
    if (!depth_out) return fail(EXA_MESH_E_NULLPTR, "depth_out is NULL");
    return kin_tree(J, parents, nullptr, depth_out);
}

int exa_mesh_kinematics_forward(int32_t B, int32_t J, const int32_t* parents, const float* pose, const float* rot_in,
                                const float* joints, const float* pre, float* transforms, float* posed_joints,
                                float* rot, void* stream) {
    KinFwdParams P;
    if (int rc = kin_check_batch(B)) return rc;
    if (int rc = kin_tree(J, parents, &P.tree, nullptr)) return rc;
    if (B == 0) return 0;
    if ((pose != nullptr) == (rot_in != nullptr))
        return fail(EXA_MESH_E_INVALID, "exactly one of pose / rot_in must be given");
    if (!joints) return fail(EXA_MESH_E_NULLPTR, "joints is NULL");
    if (!transforms || !posed_joints || !rot) return fail(EXA_MESH_E_NULLPTR, "transforms / posed_joints / rot is NULL");
    P.J = J;
    P.pose = pose;
    P.rot_in = rot_in;
    P.joints = joints;
    P.pre = pre;
    P.transforms = transforms;
    P.posed = posed_joints;
    P.rot = rot;
    hipLaunchKernelGGL(kin_fwd, dim3(B), dim3(KJ), 0, (hipStream_t)stream, P);
    return launched("kin_fwd");
}

int exa_mesh_kinematics_backward(int32_t B, int32_t J, const int32_t* parents, const float* pose, const float* rot,
                                 const float* joints, const float* pre, const float* grad_transforms,
                                 const float* grad_posed_joints, float* grad_pose, float* grad_rot, float* grad_joints,
                                 float* grad_pre, void* stream) {
    KinBwdParams P;
    if (int rc = kin_check_batch(B)) return rc;
    if (int rc = kin_tree(J, parents, &P.tree, nullptr)) return rc;
    if (B == 0 || (!grad_pose && !grad_rot && !grad_joints && !grad_pre)) return 0;
    if (!rot || !joints) return fail(EXA_MESH_E_NULLPTR, "rot / joints is NULL");
    if (grad_pose && !pose) return fail(EXA_MESH_E_NULLPTR, "grad_pose needs pose");
    if (grad_pre && !pre) return fail(EXA_MESH_E_NULLPTR, "grad_pre needs pre");
    P.J = J;
    P.pose = pose;
    P.rot = rot;
    P.joints = joints;
    P.pre = pre;
    P.g_transforms = grad_transforms;
    P.g_posed = grad_posed_joints;
    P.g_pose = grad_pose;
    P.g_rot = grad_rot;
    P.g_joints = grad_joints;
    P.g_pre = grad_pre;
    hipLaunchKernelGGL(kin_bwd, dim3(B), dim3(KJ), 0, (hipStream_t)stream, P);
    return launched("kin_bwd");
}

}  // extern "C"
