// The axis-angle -> quaternion -> rotation matrix route of pytorch3d (axis_angle_to_matrix) and its backward, as device
// functions: one rotation per lane, everything in registers.  Shared by the forward kinematics (kinematics.hip, step 1 of
// exa_mesh_kinematics_*) and the fitting's PoseLoss (fit_terms.hip, exa_mesh_pose_loss_*); include/exa_mesh.h writes out
// every operation, and both sources are compiled with -ffp-contract=off: tests/kin_oracle.py and tests/fit_oracle.py
// restate the arithmetic below line for line.  sinf / cosf are the device library's: the one step that is not bit-equal
// to a CPU evaluation.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace exa {

// The quaternion of an axis-angle vector and everything its backward reads again.
struct AxisAngle {
    float angle, sh, ch, s, r, i, j, k, n, two_s;
    bool small;
};

__device__ __forceinline__ AxisAngle aa_quaternion(float x, float y, float z) {
    AxisAngle q;
    q.angle = sqrtf((x * x + y * y) + z * z);
    const float half = 0.5f * q.angle;
    q.small = q.angle < 1e-6f;
    q.sh = sinf(half);
    q.ch = cosf(half);
    q.s = q.small ? 0.5f - (q.angle * q.angle) / 48.0f : q.sh / q.angle;
    q.r = q.ch;
    q.i = q.s * x;
    q.j = q.s * y;
    q.k = q.s * z;
    q.n = ((q.r * q.r + q.i * q.i) + q.j * q.j) + q.k * q.k;
    q.two_s = 2.0f / q.n;
    return q;
}

__device__ __forceinline__ void quaternion_matrix(const AxisAngle& q, float* R) {
    const float r = q.r, i = q.i, j = q.j, k = q.k, t = q.two_s;
    R[0] = 1.0f - t * (j * j + k * k);
    R[1] = t * (i * j - k * r);
    R[2] = t * (i * k + j * r);
    R[3] = t * (i * j + k * r);
    R[4] = 1.0f - t * (i * i + k * k);
    R[5] = t * (j * k - i * r);
    R[6] = t * (i * k - j * r);
    R[7] = t * (j * k + i * r);
    R[8] = 1.0f - t * (i * i + j * j);
}

// dL/d(x, y, z) from G = dL/dR: the analytic Jacobian of the route above, d angle / d x := 0 at angle == 0.
__device__ __forceinline__ void aa_backward(float x, float y, float z, const float* G, float* gp) {
    const AxisAngle q = aa_quaternion(x, y, z);
    const float r = q.r, i = q.i, j = q.j, k = q.k, t = q.two_s;
    // R = [1 - t m00, t m01, ...]: dL/dt, then h = dL/dm
    const float m00 = j * j + k * k, m01 = i * j - k * r, m02 = i * k + j * r;
    const float m10 = i * j + k * r, m11 = i * i + k * k, m12 = j * k - i * r;
    const float m20 = i * k - j * r, m21 = j * k + i * r, m22 = i * i + j * j;
    const float g_t = (((((((G[1] * m01 + G[2] * m02) + G[3] * m10) + G[5] * m12) + G[6] * m20) + G[7] * m21) -
                        G[0] * m00) - G[4] * m11) - G[8] * m22;
    const float h00 = -(t * G[0]), h01 = t * G[1], h02 = t * G[2];
    const float h10 = t * G[3], h11 = -(t * G[4]), h12 = t * G[5];
    const float h20 = t * G[6], h21 = t * G[7], h22 = -(t * G[8]);
    float g_r = ((((k * h10 - k * h01) + j * h02) - i * h12) - j * h20) + i * h21;
    float g_i = ((((((j * h01 + k * h02) + j * h10) + (2.0f * i) * h11) - r * h12) + k * h20) + r * h21) + (2.0f * i) * h22;
    float g_j = ((((((2.0f * j) * h00 + i * h01) + r * h02) + i * h10) + k * h12) - r * h20) + k * h21 + (2.0f * j) * h22;
    float g_k = ((((((2.0f * k) * h00 - r * h01) + i * h02) + r * h10) + (2.0f * k) * h11) + j * h12) + i * h20 + j * h21;
    // t = 2 / n, n = |q|^2
    const float g_n = -(g_t * t) / q.n;
    g_r = g_r + (2.0f * r) * g_n;
    g_i = g_i + (2.0f * i) * g_n;
    g_j = g_j + (2.0f * j) * g_n;
    g_k = g_k + (2.0f * k) * g_n;
    // q = (cos(half), s x, s y, s z)
    const float g_s = (g_i * x + g_j * y) + g_k * z;
    float g_half = -(q.sh * g_r);
    float g_angle;
    if (q.small) {
        g_angle = 0.5f * g_half - g_s * (q.angle / 24.0f);
    } else {
        g_half = g_half + g_s * (q.ch / q.angle);
        g_angle = 0.5f * g_half - g_s * (q.s / q.angle);
    }
    const bool zero = q.angle == 0.0f;
    const float ux = zero ? 0.0f : x / q.angle, uy = zero ? 0.0f : y / q.angle, uz = zero ? 0.0f : z / q.angle;
    gp[0] = q.s * g_i + g_angle * ux;
    gp[1] = q.s * g_j + g_angle * uy;
    gp[2] = q.s * g_k + g_angle * uz;
}

}  // namespace exa
