// The 6D rotation -> quaternion route of pytorch3d (rotation_6d_to_matrix, matrix_to_quaternion) and its backward, as
// device functions: one row per lane, everything in registers.  Shared by the scene-Gaussian stage (scene_assets.hip,
// include/exa_raster.h) and the pose-parameter stage (pose_params.hip, include/exa_mesh.h); both headers write out every
// operation and the order of every sum, and both sources are compiled with -ffp-contract=off: tests/scene_oracle.py
// restates the arithmetic below line for line in float32 numpy and the kernels equal it bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace exa {
namespace rot6d {

constexpr float EPS = 1e-12f;      // F.normalize's eps

// ---- v / max(|v|, eps) and its backward --------------------------------------------------------------------------------
struct Unit { float n, d; };

__device__ __forceinline__ Unit unit(const float v[3], float out[3]) {
    Unit u;
    u.n = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    u.d = fmaxf(u.n, EPS);
    out[0] = v[0] / u.d; out[1] = v[1] / u.d; out[2] = v[2] / u.d;
    return u;
}

// torch's conventions: clamp_min passes the gradient where n >= eps, norm's gradient is 0 at n == 0
__device__ __forceinline__ void unit_backward(const float v[3], Unit u, const float g[3], float gv[3]) {
    const float s = (g[0] * v[0] + g[1] * v[1]) + g[2] * v[2];
    const float gd = -(s / (u.d * u.d));
    const float gn = u.n >= EPS ? gd : 0.0f;
    const float k = u.n > 0.0f ? gn / u.n : 0.0f;
    gv[0] = g[0] / u.d + v[0] * k;
    gv[1] = g[1] / u.d + v[1] * k;
    gv[2] = g[2] / u.d + v[2] * k;
}

// ---- rotation_6d_to_matrix and matrix_to_quaternion --------------------------------------------------------------------
struct Frame {
    float b1[3], b2[3], b3[3], c[3], dot;
    Unit u1, u2;
};

__device__ __forceinline__ void frame(const float a[6], Frame& f) {
    f.u1 = unit(a, f.b1);
    f.dot = (f.b1[0] * a[3] + f.b1[1] * a[4]) + f.b1[2] * a[5];
    f.c[0] = a[3] - f.dot * f.b1[0]; f.c[1] = a[4] - f.dot * f.b1[1]; f.c[2] = a[5] - f.dot * f.b1[2];
    f.u2 = unit(f.c, f.b2);
    f.b3[0] = f.b1[1] * f.b2[2] - f.b1[2] * f.b2[1];
    f.b3[1] = f.b1[2] * f.b2[0] - f.b1[0] * f.b2[2];
    f.b3[2] = f.b1[0] * f.b2[1] - f.b1[1] * f.b2[0];
}

struct Quat {
    float row[4], q, D;
    int i;
    bool neg;
};

// The selected x_i is >= 1 (the four sum to 4), so neither the 0.1 floor on q nor the positive-part branch of the sqrt
// can bind for it: they are not carried.
__device__ __forceinline__ void quaternion(const Frame& f, Quat& Q, float out[4]) {
    const float m00 = f.b1[0], m01 = f.b1[1], m02 = f.b1[2], m10 = f.b2[0], m11 = f.b2[1], m12 = f.b2[2],
                m20 = f.b3[0], m21 = f.b3[1], m22 = f.b3[2];
    const float x0 = ((1.0f + m00) + m11) + m22, x1 = ((1.0f + m00) - m11) - m22, x2 = ((1.0f - m00) + m11) - m22,
                x3 = ((1.0f - m00) - m11) + m22;
    int i = 0;
    float xm = x0;
    if (x1 > xm) { i = 1; xm = x1; }
    if (x2 > xm) { i = 2; xm = x2; }
    if (x3 > xm) { i = 3; xm = x3; }
    const float q = sqrtf(xm), qq = q * q;
    const float A = m21 - m12, B = m02 - m20, C = m10 - m01, E = m10 + m01, F = m02 + m20, G = m12 + m21;
    if (i == 0)      { Q.row[0] = qq; Q.row[1] = A;  Q.row[2] = B;  Q.row[3] = C; }
    else if (i == 1) { Q.row[0] = A;  Q.row[1] = qq; Q.row[2] = E;  Q.row[3] = F; }
    else if (i == 2) { Q.row[0] = B;  Q.row[1] = E;  Q.row[2] = qq; Q.row[3] = G; }
    else             { Q.row[0] = C;  Q.row[1] = F;  Q.row[2] = G;  Q.row[3] = qq; }
    Q.q = q;
    Q.D = 2.0f * q;
    Q.i = i;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = Q.row[j] / Q.D;
    Q.neg = out[0] < 0.0f;
    if (Q.neg) {
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = -out[j];
    }
}

// dL/d(rotation row) from the quaternion's cotangent: no gradient through the candidate index or the sign
__device__ __forceinline__ void rotation_backward(const float a[6], const Frame& f, const Quat& Q, const float g[4],
                                                  float ga[6]) {
    float gs[4], gr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        gs[j] = Q.neg ? -g[j] : g[j];
        gr[j] = gs[j] / Q.D;
    }
    const float S = ((gs[0] * Q.row[0] + gs[1] * Q.row[1]) + gs[2] * Q.row[2]) + gs[3] * Q.row[3];
    const float gD = -(S / (Q.D * Q.D));
    const int i = Q.i;
    const float gri = i == 0 ? gr[0] : i == 1 ? gr[1] : i == 2 ? gr[2] : gr[3];
    const float gq = 2.0f * gD + (gri * 2.0f) * Q.q;
    const float gx = gq / Q.D;
    float gA = 0.0f, gB = 0.0f, gC = 0.0f, gE = 0.0f, gF = 0.0f, gG = 0.0f;
    if (i == 0)      { gA = gr[1]; gB = gr[2]; gC = gr[3]; }
    else if (i == 1) { gA = gr[0]; gE = gr[2]; gF = gr[3]; }
    else if (i == 2) { gB = gr[0]; gE = gr[1]; gG = gr[3]; }
    else             { gC = gr[0]; gF = gr[1]; gG = gr[2]; }
    float gb1[3], gb2[3], gb3[3];
    gb1[0] = i < 2 ? gx : -gx;                    // m00
    gb2[1] = (i == 0 || i == 2) ? gx : -gx;       // m11
    gb3[2] = (i == 0 || i == 3) ? gx : -gx;       // m22
    gb3[1] = gA + gG; gb2[2] = gG - gA;           // m21, m12
    gb1[2] = gB + gF; gb3[0] = gF - gB;           // m02, m20
    gb2[0] = gC + gE; gb1[1] = gE - gC;           // m10, m01
    // b3 = b1 x b2
    gb1[0] = gb1[0] + (f.b2[1] * gb3[2] - f.b2[2] * gb3[1]);
    gb1[1] = gb1[1] + (f.b2[2] * gb3[0] - f.b2[0] * gb3[2]);
    gb1[2] = gb1[2] + (f.b2[0] * gb3[1] - f.b2[1] * gb3[0]);
    gb2[0] = gb2[0] + (gb3[1] * f.b1[2] - gb3[2] * f.b1[1]);
    gb2[1] = gb2[1] + (gb3[2] * f.b1[0] - gb3[0] * f.b1[2]);
    gb2[2] = gb2[2] + (gb3[0] * f.b1[1] - gb3[1] * f.b1[0]);
    // b2 = c / max(|c|, eps), c = a2 - dot b1, dot = b1 . a2
    float gc[3];
    unit_backward(f.c, f.u2, gb2, gc);
    const float gdot = -((gc[0] * f.b1[0] + gc[1] * f.b1[1]) + gc[2] * f.b1[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        gb1[k] = (gb1[k] - f.dot * gc[k]) + gdot * a[3 + k];
        ga[3 + k] = gc[k] + gdot * f.b1[k];
    }
    unit_backward(a, f.u1, gb1, ga);
}

}  // namespace rot6d
}  // namespace exa
