// The pose-parameter stage for gfx950 (include/exa_mesh.h, exa_mesh_pose_*): SMPLXParamDict.forward of the reference
// (avatar/common/nets/module.py:673-684) -- matrix_to_axis_angle(rotation_6d_to_matrix(p)) for the seven pose tensors of
// every frame of a call -- in one launch each way, and the two detached pose features HumanGaussian rebuilds from the
// kinematics' rotations (module.py:464,484,498).  The header writes out every operation and the order of every sum;
// tests/pose_oracle.py restates them in numpy.  Compiled with -ffp-contract=off.
//
//   pose_fwd / pose_bwd   one 6D row per lane, 64 lanes a workgroup: a frame's 55 rows are one wave, and the frames of a
//             call spread over the chip.  The rows live in up to 64 separately allocated segments (the nn.Parameters as
//             they are): row counts and pointers travel BY VALUE in the argument block, so there is no device buffer,
//             no copy and no state between calls.  Every lane walks the segment table with wave-uniform loads and keeps
//             the one entry its row falls into -- no table is indexed by a lane's own value.  A row is 24 bytes in and 12
//             out: everything stays in registers, there is no LDS and no barrier.  Nothing is summed across rows: no
//             atomics, no workspace, the same inputs give the same bits.  The 6D -> quaternion functions are rot6d.h's,
//             bit for bit those of the scene-Gaussian stage; atan2f / sinf / cosf are the device library's: the steps a
//             CPU does not reproduce bit for bit.
//   pose_features         one lane per element of rot[1:]: a copy and a subtraction.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/exa_mesh.h"
#include "abi_status.h"
#include "rot6d.h"

namespace exa_mesh_impl {

EXA_ABI_STATUS_SHARED("exa_mesh")         // exa_mesh_last_error() and its buffer are mesh_raster.hip's

using namespace exa::rot6d;

constexpr int PS = EXA_MESH_POSE_MAX_SEGMENTS;
constexpr int PB = 64;                        // lanes (rows) per workgroup: one wave
constexpr float SMALL = 1e-6f;

struct PoseFwdParams {
    int32_t n_seg, R;
    int32_t start[PS + 1];                    // first packed row of every segment; start[n_seg] = R
    const float* d6[PS];
    float* out[PS];                           // NULL: only packed / quat
    float* packed;
    float* quat;
};

struct PoseBwdParams {
    int32_t n_seg, R;
    int32_t start[PS + 1];
    const float* d6[PS];
    const float* g_out[PS];                   // NULL: absent
    float* g_d6[PS];                          // NULL: not wanted, the segment's lanes leave
    const float* g_packed;
};

// quaternion_to_axis_angle and what its backward reads again
struct AxisAngleOut {
    float n, half, angle, s;
    bool small;
};

__device__ __forceinline__ AxisAngleOut axis_angle(const float q[4], float out[3]) {
    AxisAngleOut A;
    A.n = sqrtf((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3]);
    A.half = atan2f(A.n, q[0]);
    A.angle = 2.0f * A.half;
    A.small = fabsf(A.angle) < SMALL;
    A.s = A.small ? 0.5f - (A.angle * A.angle) / 48.0f : sinf(A.half) / A.angle;
    out[0] = q[1] / A.s; out[1] = q[2] / A.s; out[2] = q[3] / A.s;
    return A;
}

// dL/dq from the axis-angle row's cotangent: no gradient through `small`, norm's gradient 0 at 0
__device__ __forceinline__ void axis_angle_backward(const float q[4], const AxisAngleOut& A, const float g[3], float gq[4]) {
    const float T = (g[0] * q[1] + g[1] * q[2]) + g[2] * q[3];
    const float gs = -(T / (A.s * A.s));
    float g_angle, g_half;
    if (A.small) {
        g_angle = -(gs * (A.angle / 24.0f));
        g_half = 2.0f * g_angle;
    } else {
        g_angle = -(gs * (A.s / A.angle));
        g_half = 2.0f * g_angle + (gs / A.angle) * cosf(A.half);
    }
    const float den = A.n * A.n + q[0] * q[0];
    const float gn = g_half * (q[0] / den);
    gq[0] = -(g_half * (A.n / den));
    const float k = A.n > 0.0f ? gn / A.n : 0.0f;
    gq[1] = g[0] / A.s + q[1] * k;
    gq[2] = g[1] / A.s + q[2] * k;
    gq[3] = g[2] / A.s + q[3] * k;
}

__global__ __launch_bounds__(PB) void pose_fwd(PoseFwdParams P) {
    const int r = blockIdx.x * PB + threadIdx.x;
    if (r >= P.R) return;
    const float* src = nullptr;
    float* dst = nullptr;
    int local = 0;
    for (int s = 0; s < P.n_seg; ++s) {       // wave-uniform loads of the table, one select per entry
        const int lo = P.start[s], hi = P.start[s + 1];
        if (r >= lo && r < hi) { src = P.d6[s]; dst = P.out[s]; local = r - lo; }
    }
    if (!src) return;                         // unreachable: the starts cover [0, R)
    float a[6], q[4], aa[3];
#pragma unroll
    for (int j = 0; j < 6; ++j) a[j] = src[(size_t)local * 6 + j];
    Frame f;
    Quat Q;
    frame(a, f);
    quaternion(f, Q, q);
    axis_angle(q, aa);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (dst) dst[(size_t)local * 3 + c] = aa[c];
        if (P.packed) P.packed[(size_t)r * 3 + c] = aa[c];
    }
    if (P.quat) {
#pragma unroll
        for (int j = 0; j < 4; ++j) P.quat[(size_t)r * 4 + j] = q[j];
    }
}

__global__ __launch_bounds__(PB) void pose_bwd(PoseBwdParams P) {
    const int r = blockIdx.x * PB + threadIdx.x;
    if (r >= P.R) return;
    const float* src = nullptr;
    const float* gsrc = nullptr;
    float* dst = nullptr;
    int local = 0;
    for (int s = 0; s < P.n_seg; ++s) {
        const int lo = P.start[s], hi = P.start[s + 1];
        if (r >= lo && r < hi) { src = P.d6[s]; gsrc = P.g_out[s]; dst = P.g_d6[s]; local = r - lo; }
    }
    if (!src || !dst) return;
    float a[6], q[4], aa[3], g[3], gq[4], ga[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) a[j] = src[(size_t)local * 6 + j];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (gsrc && P.g_packed) g[c] = gsrc[(size_t)local * 3 + c] + P.g_packed[(size_t)r * 3 + c];
        else if (gsrc) g[c] = gsrc[(size_t)local * 3 + c];
        else if (P.g_packed) g[c] = P.g_packed[(size_t)r * 3 + c];
        else g[c] = 0.0f;
    }
    Frame f;
    Quat Q;
    frame(a, f);
    quaternion(f, Q, q);
    const AxisAngleOut A = axis_angle(q, aa);
    axis_angle_backward(q, A, g, gq);
    rotation_backward(a, f, Q, gq, ga);
#pragma unroll
    for (int j = 0; j < 6; ++j) dst[(size_t)local * 6 + j] = ga[j];
}

// lane e = element e of rot[1:] (9 (J - 1) of them)
__global__ __launch_bounds__(PB) void pose_features(int32_t J, int32_t n_body, const float* __restrict__ rot,
                                                    float* __restrict__ pose6d, float* __restrict__ pose_feat) {
    const int e = blockIdx.x * PB + threadIdx.x;
    if (e >= 9 * (J - 1)) return;
    const int j = e / 9, k = e - 9 * j;       // joint j + 1, element k of its matrix
    const float v = rot[9 + e];
    if (pose_feat) pose_feat[e] = v - ((k == 0 || k == 4 || k == 8) ? 1.0f : 0.0f);
    if (pose6d && j < n_body && k < 6) pose6d[6 * j + k] = v;
}

// rows and starts of a call; < 0 with the message set
int pose_table(int32_t n_seg, const int32_t* rows, int32_t* start, int32_t* R) {
    if (n_seg < 0 || n_seg > PS) return fail(EXA_MESH_E_INVALID, "n_seg must be 0 .. 64 (EXA_MESH_POSE_MAX_SEGMENTS)");
    if (n_seg > 0 && !rows) return fail(EXA_MESH_E_NULLPTR, "rows is NULL");
    int64_t total = 0;
    for (int s = 0; s < n_seg; ++s) {
        if (rows[s] < 0) return fail(EXA_MESH_E_INVALID, "negative row count");
        start[s] = (int32_t)total;
        total += rows[s];
        if (total > EXA_MESH_POSE_MAX_ROWS) return fail(EXA_MESH_E_INVALID, "more than 2^24 rows (EXA_MESH_POSE_MAX_ROWS)");
    }
    for (int s = n_seg; s <= PS; ++s) start[s] = (int32_t)total;
    *R = (int32_t)total;
    return 0;
}

}  // namespace exa_mesh_impl

using namespace exa_mesh_impl;

extern "C" {

int exa_mesh_pose_params_forward(int32_t n_seg, const int32_t* rows, const float* const* d6, float* const* out,
                                 float* packed, float* quat, void* stream) {
    PoseFwdParams P;
    if (int rc = pose_table(n_seg, rows, P.start, &P.R)) return rc;
    if (P.R == 0) return 0;
    if (!d6) return fail(EXA_MESH_E_NULLPTR, "d6 is NULL");
    bool any = packed || quat;
    for (int s = 0; s < PS; ++s) {
        const bool live = s < n_seg && rows[s] > 0;
        if (live && !d6[s]) return fail(EXA_MESH_E_NULLPTR, "d6 holds a NULL pointer for a segment with rows");
        P.d6[s] = live ? d6[s] : nullptr;
        P.out[s] = live && out ? out[s] : nullptr;
        any = any || P.out[s];
    }
    if (!any) return 0;
    P.n_seg = n_seg;
    P.packed = packed;
    P.quat = quat;
    hipLaunchKernelGGL(pose_fwd, dim3(exa::ceil_div(P.R, PB)), dim3(PB), 0, (hipStream_t)stream, P);
    return launched("pose_fwd");
}

int exa_mesh_pose_params_backward(int32_t n_seg, const int32_t* rows, const float* const* d6,
                                  const float* const* grad_out, const float* grad_packed, float* const* grad_d6,
                                  void* stream) {
    PoseBwdParams P;
    if (int rc = pose_table(n_seg, rows, P.start, &P.R)) return rc;
    if (P.R == 0 || !grad_d6) return 0;
    if (!d6) return fail(EXA_MESH_E_NULLPTR, "d6 is NULL");
    bool any = false;
    for (int s = 0; s < PS; ++s) {
        const bool live = s < n_seg && rows[s] > 0 && grad_d6[s];
        if (live && !d6[s]) return fail(EXA_MESH_E_NULLPTR, "d6 holds a NULL pointer for a segment with rows");
        P.d6[s] = live ? d6[s] : nullptr;
        P.g_out[s] = live && grad_out ? grad_out[s] : nullptr;
        P.g_d6[s] = live ? grad_d6[s] : nullptr;
        any = any || live;
    }
    if (!any) return 0;
    P.n_seg = n_seg;
    P.g_packed = grad_packed;
    hipLaunchKernelGGL(pose_bwd, dim3(exa::ceil_div(P.R, PB)), dim3(PB), 0, (hipStream_t)stream, P);
    return launched("pose_bwd");
}

int exa_mesh_pose_features(int32_t J, int32_t n_body, const float* rot, float* pose6d, float* pose_feat, void* stream) {
    if (J < 1 || J > EXA_MESH_KIN_MAX_JOINTS) return fail(EXA_MESH_E_INVALID, "J (joints) must be 1 .. 64");
    if (n_body < 0 || n_body > J - 1) return fail(EXA_MESH_E_INVALID, "n_body must be 0 .. J - 1: rot has no more rows");
    if (J == 1 || (!pose6d && !pose_feat)) return 0;
    if (!rot) return fail(EXA_MESH_E_NULLPTR, "rot is NULL");
    hipLaunchKernelGGL(pose_features, dim3(exa::ceil_div(9 * (J - 1), PB)), dim3(PB), 0, (hipStream_t)stream, J, n_body,
                       rot, pose6d, pose_feat);
    return launched("pose_features");
}

}  // extern "C"
