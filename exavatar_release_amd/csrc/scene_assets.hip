// The scene-Gaussian stage for gfx950: SceneGaussian.forward (reference avatar/common/nets/module.py:253-272) in one
// launch each way -- sigmoid / exp activations, the 6D rotation -> quaternion route of pytorch3d, and the SH colour seen
// from the camera centre -- behind exa_raster_scene_assets_forward / _backward (include/exa_raster.h, which writes out
// every operation and the order of every sum).  Compiled with -ffp-contract=off: tests/scene_oracle.py restates the
// arithmetic below line for line in float32 numpy, and everything but the two expf-based outputs equals it bit for bit.
//
// One Gaussian is one lane, 256 lanes a workgroup; nothing is summed across Gaussians, so there are no atomics and the
// same inputs give the same bits.  The 6-, 3- and 3*Mr-float rows travel through LDS: wave-wide loads and stores of
// consecutive dwords on the HBM side, one row per lane on the LDS side with odd row strides (7, 3, 3 * Mr | 1), so the
// lanes' row accesses fall into different banks.  Quaternions (one float4) and colours leave as whole-row stores.
// HBM traffic per Gaussian at degree 3 (Mr = 15): forward reads 12 + 4 + 12 + 24 + 12 + 180 = 244 B and writes
// 4 + 12 + 16 + 12 = 44 B; backward reads the 228 B of (mean, rotation, dc, rest), 16 B of saved outputs and 44 B of
// cotangents and writes 12 + 4 + 12 + 24 + 12 + 180 = 244 B.
#include "../../include/exa_raster.h"
#include "abi_status.h"
#include "rot6d.h"

namespace exa {
namespace scene {

// unit / unit_backward (v / max(|v|, eps), F.normalize's eps), frame / quaternion / rotation_backward: the 6D rotation ->
// quaternion route, shared with pose_params.hip
using namespace rot6d;

constexpr int SB = 256;            // lanes (Gaussians) per workgroup
constexpr int ROT_S = 7;         // LDS stride of a 6-float rotation row

constexpr float C0 = 0.28209479177387814f, C1 = 0.4886025119029199f;
constexpr float C2_0 = 1.0925484305920792f, C2_1 = -1.0925484305920792f, C2_2 = 0.31539156525252005f,
                C2_3 = -1.0925484305920792f, C2_4 = 0.5462742152960396f;
constexpr float C3_0 = -0.5900435899266435f, C3_1 = 2.890611442640554f, C3_2 = -0.4570457994644658f,
                C3_3 = 0.3731763325901154f, C3_4 = -0.4570457994644658f, C3_5 = 1.445305721320277f,
                C3_6 = -0.5900435899266435f;

struct FwdArgs {
    int P;
    const float *mean, *opacity, *scale, *rotation, *dc, *rest, *cam_R, *cam_t;
    float *opacity_out, *scale_out, *rotation_out, *rgb;
};

struct BwdArgs {
    int P;
    const float *mean, *rotation, *dc, *rest, *cam_R, *cam_t, *opacity_out, *scale_out;
    const float *g_opacity_out, *g_scale_out, *g_rotation_out, *g_rgb;
    float *g_mean, *g_opacity, *g_scale, *g_rotation, *g_dc, *g_rest;
};

// rows [0, nrows) of W floats: global (row stride GS, consecutive dwords per wave) <-> LDS (row stride S)
template <int W, int S>
__device__ __forceinline__ void stage_in(float* __restrict__ lds, const float* __restrict__ g, int nrows, int GS) {
    if constexpr (W > 0) {
        for (int i = threadIdx.x; i < nrows * W; i += SB) {
            const int r = i / W, j = i - r * W;
            lds[r * S + j] = g[(size_t)r * GS + j];
        }
    }
}

template <int W, int S>
__device__ __forceinline__ void stage_out(float* __restrict__ g, const float* __restrict__ lds, int nrows) {
    if constexpr (W > 0) {
        for (int i = threadIdx.x; i < nrows * W; i += SB) {
            const int r = i / W, j = i - r * W;
            g[i] = lds[r * S + j];
        }
    }
}

// cam_pos = inverse(R) (-t) by cofactors: lane 0, broadcast through LDS (the caller synchronises)
__device__ __forceinline__ void camera_centre(const float* __restrict__ R, const float* __restrict__ t, float* s_cam) {
    if (threadIdx.x == 0) {
        const float r00 = R[0], r01 = R[1], r02 = R[2], r10 = R[3], r11 = R[4], r12 = R[5], r20 = R[6], r21 = R[7], r22 = R[8];
        const float c00 = r11 * r22 - r12 * r21, c01 = r12 * r20 - r10 * r22, c02 = r10 * r21 - r11 * r20;
        const float c10 = r02 * r21 - r01 * r22, c11 = r00 * r22 - r02 * r20, c12 = r01 * r20 - r00 * r21;
        const float c20 = r01 * r12 - r02 * r11, c21 = r02 * r10 - r00 * r12, c22 = r00 * r11 - r01 * r10;
        const float det = (r00 * c00 + r01 * c01) + r02 * c02;
        const float n0 = -t[0], n1 = -t[1], n2 = -t[2];
        s_cam[0] = ((c00 / det) * n0 + (c10 / det) * n1) + (c20 / det) * n2;
        s_cam[1] = ((c01 / det) * n0 + (c11 / det) * n1) + (c21 / det) * n2;
        s_cam[2] = ((c02 / det) * n0 + (c12 / det) * n1) + (c22 / det) * n2;
    }
}

// ---- SH colour ---------------------------------------------------------------------------------------------------------
// b[k], k = 1 .. (DEG + 1)^2 - 1: the polynomial factor of coefficient k as transforms.py:112-155 multiplies it out
template <int DEG>
__device__ __forceinline__ void sh_basis(float x, float y, float z, float b[16]) {
    if constexpr (DEG > 0) {
        b[1] = C1 * y; b[2] = C1 * z; b[3] = C1 * x;
    }
    if constexpr (DEG > 1) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        b[4] = C2_0 * xy;
        b[5] = C2_1 * yz;
        b[6] = C2_2 * ((2.0f * zz - xx) - yy);
        b[7] = C2_3 * xz;
        b[8] = C2_4 * (xx - yy);
        if constexpr (DEG > 2) {
            b[9] = (C3_0 * y) * (3.0f * xx - yy);
            b[10] = (C3_1 * xy) * z;
            b[11] = (C3_2 * y) * ((4.0f * zz - xx) - yy);
            b[12] = (C3_3 * z) * ((2.0f * zz - 3.0f * xx) - 3.0f * yy);
            b[13] = (C3_4 * x) * ((4.0f * zz - xx) - yy);
            b[14] = (C3_5 * z) * (xx - yy);
            b[15] = (C3_6 * x) * (xx - 3.0f * yy);
        }
    }
}

// the unclamped colour of one channel: dc = the channel's degree-0 coefficient, rest[3 * (k - 1)] its coefficient k
template <int DEG>
__device__ __forceinline__ float sh_unclamped(const float b[16], float dc, const float* rest) {
    float res = C0 * dc;
    if constexpr (DEG > 0) {
        res = res - b[1] * rest[0];
        res = res + b[2] * rest[3];
        res = res - b[3] * rest[6];
#pragma unroll
        for (int k = 4; k < (DEG + 1) * (DEG + 1); ++k) res = res + b[k] * rest[3 * (k - 1)];
    }
    return res + 0.5f;
}

// dL/d(direction) from w[k] = the signed channel sums of cotangent x coefficient
template <int DEG>
__device__ __forceinline__ void sh_direction_backward(float x, float y, float z, const float w[16], float gd[3]) {
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    if constexpr (DEG > 0) {
        gx = C1 * w[3]; gy = C1 * w[1]; gz = C1 * w[2];
    }
    if constexpr (DEG > 1) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        gx = gx + (C2_0 * y) * w[4]; gx = gx - (C2_2 * (2.0f * x)) * w[6]; gx = gx + (C2_3 * z) * w[7];
        gx = gx + (C2_4 * (2.0f * x)) * w[8];
        gy = gy + (C2_0 * x) * w[4]; gy = gy + (C2_1 * z) * w[5]; gy = gy - (C2_2 * (2.0f * y)) * w[6];
        gy = gy - (C2_4 * (2.0f * y)) * w[8];
        gz = gz + (C2_1 * y) * w[5]; gz = gz + (C2_2 * (4.0f * z)) * w[6]; gz = gz + (C2_3 * x) * w[7];
        if constexpr (DEG > 2) {
            gx = gx + (C3_0 * (6.0f * xy)) * w[9]; gx = gx + (C3_1 * yz) * w[10]; gx = gx - (C3_2 * (2.0f * xy)) * w[11];
            gx = gx - (C3_3 * (6.0f * xz)) * w[12]; gx = gx + (C3_4 * ((4.0f * zz - 3.0f * xx) - yy)) * w[13];
            gx = gx + (C3_5 * (2.0f * xz)) * w[14]; gx = gx + (C3_6 * (3.0f * xx - 3.0f * yy)) * w[15];
            gy = gy + (C3_0 * (3.0f * xx - 3.0f * yy)) * w[9]; gy = gy + (C3_1 * xz) * w[10];
            gy = gy + (C3_2 * ((4.0f * zz - xx) - 3.0f * yy)) * w[11]; gy = gy - (C3_3 * (6.0f * yz)) * w[12];
            gy = gy - (C3_4 * (2.0f * xy)) * w[13]; gy = gy - (C3_5 * (2.0f * yz)) * w[14];
            gy = gy - (C3_6 * (6.0f * xy)) * w[15];
            gz = gz + (C3_1 * xy) * w[10]; gz = gz + (C3_2 * (8.0f * yz)) * w[11];
            gz = gz + (C3_3 * ((6.0f * zz - 3.0f * xx) - 3.0f * yy)) * w[12]; gz = gz + (C3_4 * (8.0f * xz)) * w[13];
            gz = gz + (C3_5 * (xx - yy)) * w[14];
        }
    }
    gd[0] = gx; gd[1] = gy; gd[2] = gz;
}

constexpr int rest_stride(int MR) { return (3 * MR) | 1; }

// ---- forward -----------------------------------------------------------------------------------------------------------
template <int MR, int DEG>
__global__ __launch_bounds__(SB) void scene_fwd(FwdArgs a) {
    constexpr int NA = (DEG + 1) * (DEG + 1) - 1, WA = 3 * NA, SA = WA | 1;      // the active rows of feature_rest
    static_assert(NA <= MR, "sh_degree needs more coefficients than feature_rest has");
    __shared__ float s_rot[SB * ROT_S], s_mean[SB * 3], s_dc[SB * 3], s_rest[SB * SA], s_cam[3];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * SB;
    const int nrows = min(SB, a.P - (int)base);

    camera_centre(a.cam_R, a.cam_t, s_cam);
    stage_in<6, ROT_S>(s_rot, a.rotation + base * 6, nrows, 6);
    stage_in<3, 3>(s_mean, a.mean + base * 3, nrows, 3);
    stage_in<3, 3>(s_dc, a.dc + base * 3, nrows, 3);
    stage_in<WA, SA>(s_rest, a.rest + base * (3 * MR), nrows, 3 * MR);
    // the activations are elementwise: consecutive lanes, consecutive dwords
    for (int i = tid; i < nrows; i += SB) a.opacity_out[base + i] = 1.0f / (1.0f + expf(-a.opacity[base + i]));
    for (int i = tid; i < nrows * 3; i += SB) a.scale_out[base * 3 + i] = expf(a.scale[base * 3 + i]);
    __syncthreads();
    if (tid >= nrows) return;

    float rot[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) rot[j] = s_rot[tid * ROT_S + j];
    Frame f;
    Quat Q;
    float q[4];
    frame(rot, f);
    quaternion(f, Q, q);
    reinterpret_cast<float4*>(a.rotation_out)[base + tid] = make_float4(q[0], q[1], q[2], q[3]);

    const float v[3] = {s_mean[tid * 3 + 0] - s_cam[0], s_mean[tid * 3 + 1] - s_cam[1], s_mean[tid * 3 + 2] - s_cam[2]};
    float d[3], b[16];
    unit(v, d);
    sh_basis<DEG>(d[0], d[1], d[2], b);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float u = sh_unclamped<DEG>(b, s_dc[tid * 3 + c], s_rest + tid * SA + c);
        a.rgb[(base + tid) * 3 + c] = u < 0.0f ? 0.0f : u;
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
template <int MR, int DEG>
__global__ __launch_bounds__(SB) void scene_bwd(BwdArgs a) {
    constexpr int NA = (DEG + 1) * (DEG + 1) - 1, WA = 3 * NA, SR = rest_stride(MR);
    static_assert(NA <= MR, "sh_degree needs more coefficients than feature_rest has");
    __shared__ float s_rot[SB * ROT_S], s_mean[SB * 3], s_dc[SB * 3], s_grgb[SB * 3], s_rest[SB * SR], s_cam[3];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * SB;
    const int nrows = min(SB, a.P - (int)base);
    const bool colour = a.g_mean || a.g_dc || a.g_rest;

    if (a.g_rotation) stage_in<6, ROT_S>(s_rot, a.rotation + base * 6, nrows, 6);
    if (colour) {
        camera_centre(a.cam_R, a.cam_t, s_cam);
        stage_in<3, 3>(s_mean, a.mean + base * 3, nrows, 3);
        stage_in<3, 3>(s_dc, a.dc + base * 3, nrows, 3);
        stage_in<WA, SR>(s_rest, a.rest + base * (3 * MR), nrows, 3 * MR);
        if (a.g_rgb) {
            stage_in<3, 3>(s_grgb, a.g_rgb + base * 3, nrows, 3);
        } else {
            for (int i = tid; i < nrows * 3; i += SB) s_grgb[i] = 0.0f;
        }
    }
    // sigmoid and exp from the saved outputs, as torch forms them; a missing cotangent is zero
    if (a.g_opacity) {
        for (int i = tid; i < nrows; i += SB) {
            const float y = a.opacity_out[base + i], g = a.g_opacity_out ? a.g_opacity_out[base + i] : 0.0f;
            a.g_opacity[base + i] = (g * (1.0f - y)) * y;
        }
    }
    if (a.g_scale) {
        for (int i = tid; i < nrows * 3; i += SB) {
            const float y = a.scale_out[base * 3 + i], g = a.g_scale_out ? a.g_scale_out[base * 3 + i] : 0.0f;
            a.g_scale[base * 3 + i] = g * y;
        }
    }
    __syncthreads();

    if (tid < nrows && a.g_rotation) {
        float rot[6], q[4], ga[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) rot[j] = s_rot[tid * ROT_S + j];
        float4 g4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (a.g_rotation_out) g4 = reinterpret_cast<const float4*>(a.g_rotation_out)[base + tid];
        const float g[4] = {g4.x, g4.y, g4.z, g4.w};
        Frame f;
        Quat Q;
        frame(rot, f);
        quaternion(f, Q, q);
        rotation_backward(rot, f, Q, g, ga);
#pragma unroll
        for (int j = 0; j < 6; ++j) s_rot[tid * ROT_S + j] = ga[j];      // the lane's own row: no hazard
    }
    if (tid < nrows && colour) {
        const float v[3] = {s_mean[tid * 3 + 0] - s_cam[0], s_mean[tid * 3 + 1] - s_cam[1], s_mean[tid * 3 + 2] - s_cam[2]};
        float d[3], b[16], gm[3];
        const Unit u = unit(v, d);
        sh_basis<DEG>(d[0], d[1], d[2], b);
        float* rest = s_rest + tid * SR;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float uc = sh_unclamped<DEG>(b, s_dc[tid * 3 + c], rest + c);
            gm[c] = uc < 0.0f ? 0.0f : s_grgb[tid * 3 + c];      // clamp_min passes the gradient at equality
            s_dc[tid * 3 + c] = C0 * gm[c];
        }
        float w[16];
#pragma unroll
        for (int k = 1; k <= NA; ++k) {
            float* r = rest + 3 * (k - 1);
            const float wk = (gm[0] * r[0] + gm[1] * r[1]) + gm[2] * r[2];
            const bool minus = k == 1 || k == 3;
            w[k] = minus ? -wk : wk;
#pragma unroll
            for (int c = 0; c < 3; ++c) r[c] = minus ? -(b[k] * gm[c]) : b[k] * gm[c];
        }
#pragma unroll
        for (int j = WA; j < 3 * MR; ++j) rest[j] = 0.0f;      // the rows above the active degree: exactly +0
        float gd[3], gv[3];
        sh_direction_backward<DEG>(d[0], d[1], d[2], w, gd);
        unit_backward(v, u, gd, gv);
#pragma unroll
        for (int c = 0; c < 3; ++c) s_mean[tid * 3 + c] = gv[c];
    }
    __syncthreads();
    if (a.g_rotation) stage_out<6, ROT_S>(a.g_rotation + base * 6, s_rot, nrows);
    if (a.g_mean) stage_out<3, 3>(a.g_mean + base * 3, s_mean, nrows);
    if (a.g_dc) stage_out<3, 3>(a.g_dc + base * 3, s_dc, nrows);
    if (a.g_rest) stage_out<3 * MR, SR>(a.g_rest + base * (3 * MR), s_rest, nrows);
}

}  // namespace scene

}  // namespace exa

// ---- C entry points (include/exa_raster.h): checks, then the launch --------------------------------------------------------
namespace exa_raster_impl {

using namespace exa;

EXA_ABI_STATUS_SHARED("exa_raster")       // exa_raster_last_error() and its buffer are api.hip's

// (check_scene has let through Mr in {0, 3, 8, 15}, 0 <= deg <= 3 and (deg + 1)^2 <= 1 + Mr: the default is never taken)
#define EXA_SCENE_DISPATCH(KERNEL, ARGS, WHERE)                                                                        \
    switch (Mr * 4 + sh_degree) {                                                                                      \
        case 0 * 4 + 0: scene::KERNEL<0, 0><<<grid, scene::SB, 0, s>>>(ARGS); break;                                   \
        case 3 * 4 + 0: scene::KERNEL<3, 0><<<grid, scene::SB, 0, s>>>(ARGS); break;                                   \
        case 3 * 4 + 1: scene::KERNEL<3, 1><<<grid, scene::SB, 0, s>>>(ARGS); break;                                   \
        case 8 * 4 + 0: scene::KERNEL<8, 0><<<grid, scene::SB, 0, s>>>(ARGS); break;                                   \
        case 8 * 4 + 1: scene::KERNEL<8, 1><<<grid, scene::SB, 0, s>>>(ARGS); break;                                   \
        case 8 * 4 + 2: scene::KERNEL<8, 2><<<grid, scene::SB, 0, s>>>(ARGS); break;                                   \
        case 15 * 4 + 0: scene::KERNEL<15, 0><<<grid, scene::SB, 0, s>>>(ARGS); break;                                 \
        case 15 * 4 + 1: scene::KERNEL<15, 1><<<grid, scene::SB, 0, s>>>(ARGS); break;                                 \
        case 15 * 4 + 2: scene::KERNEL<15, 2><<<grid, scene::SB, 0, s>>>(ARGS); break;                                 \
        case 15 * 4 + 3: scene::KERNEL<15, 3><<<grid, scene::SB, 0, s>>>(ARGS); break;                                 \
        default: return fail_hip(hipErrorInvalidValue, WHERE);                                                         \
    }

static int check_scene(int32_t P, int32_t Mr, int32_t sh_degree) {
    if (P < 0) return fail(EXA_RASTER_E_INVALID, "scene_assets: P < 0");
    if (Mr != 0 && Mr != 3 && Mr != 8 && Mr != 15)
        return fail(EXA_RASTER_E_INVALID, "scene_assets: Mr (rows of feature_rest) must be 0, 3, 8 or 15");
    if (sh_degree < 0 || sh_degree > 3) return fail(EXA_RASTER_E_INVALID, "scene_assets: sh_degree must be 0 .. 3");
    if ((sh_degree + 1) * (sh_degree + 1) > 1 + Mr)
        return fail(EXA_RASTER_E_INVALID, "scene_assets: sh_degree needs (sh_degree + 1)^2 <= 1 + Mr coefficients");
    return 0;
}

}  // namespace exa_raster_impl

using namespace exa_raster_impl;

extern "C" {

int exa_raster_scene_assets_forward(int32_t P, int32_t Mr, int32_t sh_degree, const float* mean, const float* opacity,
                                    const float* scale, const float* rotation, const float* feature_dc,
                                    const float* feature_rest, const float* cam_R, const float* cam_t,
                                    float* opacity_out, float* scale_out, float* rotation_out, float* rgb,
                                    void* stream) {
    if (int rc = check_scene(P, Mr, sh_degree)) return rc;
    if (P == 0) return 0;
    if (!mean || !opacity || !scale || !rotation || !feature_dc || (Mr > 0 && !feature_rest))
        return fail(EXA_RASTER_E_NULLPTR, "scene_assets: a parameter array is NULL");
    if (!cam_R || !cam_t) return fail(EXA_RASTER_E_NULLPTR, "scene_assets: cam_R / cam_t is NULL");
    if (!opacity_out || !scale_out || !rotation_out || !rgb)
        return fail(EXA_RASTER_E_NULLPTR, "scene_assets: an output array is NULL");
    const scene::FwdArgs a = {P, mean, opacity, scale, rotation, feature_dc, feature_rest, cam_R, cam_t,
                              opacity_out, scale_out, rotation_out, rgb};
    const unsigned grid = ceil_div(P, scene::SB);
    hipStream_t s = static_cast<hipStream_t>(stream);
    EXA_SCENE_DISPATCH(scene_fwd, a, "scene_fwd")
    return launched("scene_fwd");
}

int exa_raster_scene_assets_backward(int32_t P, int32_t Mr, int32_t sh_degree, const float* mean, const float* rotation,
                                     const float* feature_dc, const float* feature_rest, const float* cam_R,
                                     const float* cam_t, const float* opacity_out, const float* scale_out,
                                     const float* grad_opacity_out, const float* grad_scale_out,
                                     const float* grad_rotation_out, const float* grad_rgb, float* grad_mean,
                                     float* grad_opacity, float* grad_scale, float* grad_rotation,
                                     float* grad_feature_dc, float* grad_feature_rest, void* stream) {
    if (int rc = check_scene(P, Mr, sh_degree)) return rc;
    if (Mr == 0) grad_feature_rest = nullptr;
    if (P == 0 || (!grad_mean && !grad_opacity && !grad_scale && !grad_rotation && !grad_feature_dc && !grad_feature_rest))
        return 0;
    if (grad_opacity && !opacity_out) return fail(EXA_RASTER_E_NULLPTR, "scene_assets: grad_opacity needs opacity_out");
    if (grad_scale && !scale_out) return fail(EXA_RASTER_E_NULLPTR, "scene_assets: grad_scale needs scale_out");
    if (grad_rotation && !rotation) return fail(EXA_RASTER_E_NULLPTR, "scene_assets: grad_rotation needs rotation");
    if ((grad_mean || grad_feature_dc || grad_feature_rest) &&
        (!mean || !feature_dc || (Mr > 0 && !feature_rest) || !cam_R || !cam_t))
        return fail(EXA_RASTER_E_NULLPTR,
                    "scene_assets: the colour gradients need mean, feature_dc, feature_rest, cam_R and cam_t");
    const scene::BwdArgs a = {P, mean, rotation, feature_dc, feature_rest, cam_R, cam_t, opacity_out, scale_out,
                              grad_opacity_out, grad_scale_out, grad_rotation_out, grad_rgb,
                              grad_mean, grad_opacity, grad_scale, grad_rotation, grad_feature_dc, grad_feature_rest};
    const unsigned grid = ceil_div(P, scene::SB);
    hipStream_t s = static_cast<hipStream_t>(stream);
    EXA_SCENE_DISPATCH(scene_bwd, a, "scene_bwd")
    return launched("scene_bwd");
}

}  // extern "C"
