// Face-texture unwrap (include/exa_mesh.h; the reference's XY2UV.forward, fitting/common/nets/layer.py:53-102, and the
// accumulation of fitting/main/unwrap.py:76-83).  The semantics -- every operation in fp32 in a stated order -- are written
// out in the header; this file implements them.  The UV-space raster in front of it is mesh_raster.hip's ORTHO mode.
//
//   unwrap_clear   one thread per 4 bytes of the [B, F] visibility flags: zero (the library clears its own workspaces).
//   unwrap_mark    one thread per image pixel: the face its pix_to_face_xy holds is visible; a background pixel marks the
//                  LAST face (the reference's `valid_face_mask[-1] = 1`).  Every writer stores the byte 1 with a plain
//                  vector store: whichever lands last, the flag reads 1.  No atomics.
//   unwrap_texels  one thread per texel, all B items in index order and all C channels: projects the face's three
//                  vertices (cheaper than a launch of its own at V ~ 5 000), blends them with the texel's barycentrics,
//                  reads the four taps and writes the maps and / or adds into the persistent sums.
// No allocation, no synchronisation.  Compiled with -ffp-contract=off (build.py): the sample position and the bilinear
// blend are the expressions the reference evaluates, so no product is contracted into a fused multiply-add.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/exa_mesh.h"
#include "abi_status.h"

namespace exa_mesh_impl {

using exa::align256;
using exa::ceil_div;

EXA_ABI_STATUS_SHARED("exa_mesh")         // exa_mesh_last_error() and its buffer are mesh_raster.hip's

namespace {

constexpr int UW_BLOCK = 256;
constexpr int UW_MAX_SIDE = 8192;             // rows / columns of the image and of the map
constexpr int64_t UW_MAX_FACES = 1 << 24;     // B * F, as the raster
constexpr float UW_MIN_Z = 1e-6f;             // the raster's cull

struct UnwrapArgs {
    ExaMeshUnwrap u;
    uint8_t* flags;
    uint32_t flag_words;
    float* uvmap;
    uint8_t* mask;
    float* tex_sum;
    float* mask_sum;
};

__global__ void __launch_bounds__(UW_BLOCK) unwrap_clear(UnwrapArgs a) {
    const uint32_t i = blockIdx.x * UW_BLOCK + threadIdx.x;
    if (i < a.flag_words) reinterpret_cast<uint32_t*>(a.flags)[i] = 0u;
}

__global__ void __launch_bounds__(UW_BLOCK) unwrap_mark(UnwrapArgs a) {
    const int64_t plane = (int64_t)a.u.H * a.u.W;
    const int64_t i = (int64_t)blockIdx.x * UW_BLOCK + threadIdx.x;
    if (i >= plane * a.u.B) return;
    const int64_t n = i / plane;
    const int64_t p = a.u.pix_to_face_xy[i];
    const int64_t f = p == -1 ? (int64_t)a.u.F - 1 : p - n * a.u.F;      // -1 indexes the last face, as in the reference
    if (f >= 0 && f < a.u.F) a.flags[n * a.u.F + f] = 1;
}

__global__ void __launch_bounds__(UW_BLOCK) unwrap_texels(UnwrapArgs a) {
    const ExaMeshUnwrap& u = a.u;
    const int64_t texels = (int64_t)u.Hu * u.Wu;
    const int64_t t = (int64_t)blockIdx.x * UW_BLOCK + threadIdx.x;
    if (t >= texels) return;
    const int64_t f = u.pix_to_face_uv[t];
    bool covered = f >= 0 && f < u.F;
    int v[3] = {0, 0, 0};
    float b[3] = {0.f, 0.f, 0.f};
    if (covered) {
        for (int k = 0; k < 3; ++k) {
            v[k] = u.faces[3 * f + k];
            b[k] = u.bary_uv[3 * t + k];
            covered = covered && v[k] >= 0 && v[k] < u.V;
        }
    }
    const bool sums = a.tex_sum != nullptr;
    float acc[EXA_MESH_MAX_CHANNELS], macc[EXA_MESH_MAX_CHANNELS];
    if (sums)
        for (int c = 0; c < u.C; ++c) {
            acc[c] = a.tex_sum[c * texels + t];
            macc[c] = a.mask_sum[c * texels + t];
        }
    const float uvw = sums ? u.uv_weight[t] : 0.f;
    const float wm1 = (float)(u.W - 1), hm1 = (float)(u.H - 1);
    const size_t plane = (size_t)u.H * u.W;
    for (int n = 0; n < u.B; ++n) {
        bool sampled = covered && a.flags[(int64_t)n * u.F + f] != 0;
        float x[3], y[3];
        if (sampled) {
            const float fx = u.focal[2 * n], fy = u.focal[2 * n + 1];
            const float cx = u.princpt[2 * n], cy = u.princpt[2 * n + 1];
            for (int k = 0; k < 3; ++k) {
                const float* p = u.verts + ((size_t)n * u.V + v[k]) * 3;
                const float Z = p[2];
                sampled = sampled && Z > UW_MIN_Z;         // a wrap-around-marked face the raster culled (header)
                x[k] = p[0] / Z * fx + cx;
                y[k] = p[1] / Z * fy + cy;
            }
        }
        float nw = 0.f, ne = 0.f, sw = 0.f, se = 0.f;
        bool in_x0 = false, in_x1 = false, in_y0 = false, in_y1 = false;
        int x0 = 0, y0 = 0;
        if (sampled) {
            const float px = (x[0] * b[0] + x[1] * b[1]) + x[2] * b[2];
            const float py = (y[0] * b[0] + y[1] * b[1]) + y[2] * b[2];
            const float gx = px / wm1 * 2.f - 1.f, gy = py / hm1 * 2.f - 1.f;
            const float ix = ((gx + 1.f) / 2.f) * wm1, iy = ((gy + 1.f) / 2.f) * hm1;
            const float fx0 = floorf(ix), fy0 = floorf(iy);
            const float fx1 = fx0 + 1.f, fy1 = fy0 + 1.f;
            nw = (fx1 - ix) * (fy1 - iy);
            ne = (ix - fx0) * (fy1 - iy);
            sw = (fx1 - ix) * (iy - fy0);
            se = (ix - fx0) * (iy - fy0);
            // decided in float: a NaN or a huge position compares false everywhere and is never converted to an index
            in_x0 = fx0 >= 0.f && fx0 <= wm1;
            in_x1 = fx0 >= -1.f && fx0 <= wm1 - 1.f;
            in_y0 = fy0 >= 0.f && fy0 <= hm1;
            in_y1 = fy0 >= -1.f && fy0 <= hm1 - 1.f;
            x0 = (in_x0 || in_x1) ? (int)fx0 : 0;
            y0 = (in_y0 || in_y1) ? (int)fy0 : 0;
        }
        const float valid = (sums && u.face_valid) ? u.face_valid[n] : 1.f;
        for (int c = 0; c < u.C; ++c) {
            float value = 0.f;
            bool m = false;
            if (sampled) {
                const float* pl = u.img + ((size_t)n * u.C + c) * plane;
                float o = 0.f;          // F.grid_sample's accumulation: nw, ne, sw, se, each tap only when inside the image
                if (in_x0 && in_y0) o += pl[(size_t)y0 * u.W + x0] * nw;
                if (in_x1 && in_y0) o += pl[(size_t)y0 * u.W + x0 + 1] * ne;
                if (in_x0 && in_y1) o += pl[(size_t)(y0 + 1) * u.W + x0] * sw;
                if (in_x1 && in_y1) o += pl[(size_t)(y0 + 1) * u.W + x0 + 1] * se;
                m = o != -1.f;
                value = m ? o : 0.f;
            }
            const size_t out = ((size_t)n * u.C + c) * texels + t;
            if (a.uvmap) {
                a.uvmap[out] = value;
                a.mask[out] = m ? 1 : 0;
            }
            if (sums) {
                acc[c] = acc[c] + (value * uvw) * valid;
                macc[c] = macc[c] + ((m ? 1.f : 0.f) * uvw) * valid;
            }
        }
    }
    if (sums)
        for (int c = 0; c < u.C; ++c) {
            a.tex_sum[c * texels + t] = acc[c];
            a.mask_sum[c * texels + t] = macc[c];
        }
}

int check_unwrap_shape(int32_t B, int32_t F) {
    if (B < 0 || F < 0) return fail(EXA_MESH_E_INVALID, "negative size");
    if ((int64_t)B * F > UW_MAX_FACES) return fail(EXA_MESH_E_INVALID, "more than 2^24 faces (B * F) in one call");
    return 0;
}

}  // namespace
}  // namespace exa_mesh_impl

using namespace exa_mesh_impl;

extern "C" {

int exa_mesh_unwrap_workspace_size(int32_t B, int32_t F, uint64_t* out_bytes) {
    if (!out_bytes) return fail(EXA_MESH_E_NULLPTR, "out_bytes is NULL");
    if (int rc = check_unwrap_shape(B, F)) return rc;
    *out_bytes = align256((uint64_t)B * F);
    return 0;
}

int exa_mesh_unwrap(const ExaMeshUnwrap* u, void* flag_ws, uint64_t ws_bytes, float* uvmap, uint8_t* mask, float* tex_sum,
                    float* mask_sum, void* stream) {
    if (!u) return fail(EXA_MESH_E_NULLPTR, "unwrap descriptor is NULL");
    if (u->B < 0 || u->V < 0 || u->F < 0 || u->H < 0 || u->W < 0 || u->Hu < 0 || u->Wu < 0)
        return fail(EXA_MESH_E_INVALID, "negative size");
    if (int rc = check_unwrap_shape(u->B, u->F)) return rc;
    if (u->C < 1 || u->C > EXA_MESH_MAX_CHANNELS) return fail(EXA_MESH_E_INVALID, "unwrap: channels must be 1 .. 8");
    if (u->H > UW_MAX_SIDE || u->W > UW_MAX_SIDE || u->Hu > UW_MAX_SIDE || u->Wu > UW_MAX_SIDE)
        return fail(EXA_MESH_E_INVALID, "unwrap: image or map larger than 8192 x 8192");
    if ((int64_t)u->B * u->V > UW_MAX_FACES * 3) return fail(EXA_MESH_E_INVALID, "unwrap: more than 3 * 2^24 vertices (B * V)");
    if ((uvmap == nullptr) != (mask == nullptr)) return fail(EXA_MESH_E_INVALID, "unwrap: pass uvmap and mask, or neither");
    if ((tex_sum == nullptr) != (mask_sum == nullptr))
        return fail(EXA_MESH_E_INVALID, "unwrap: pass tex_sum and mask_sum, or neither");
    if (!uvmap && !tex_sum) return fail(EXA_MESH_E_NULLPTR, "unwrap: no output (uvmap / mask and tex_sum / mask_sum are NULL)");
    const int64_t texels = (int64_t)u->Hu * u->Wu, pixels = (int64_t)u->B * u->H * u->W;
    if (u->B == 0 || texels == 0) return 0;
    if (!u->pix_to_face_uv || !u->bary_uv) return fail(EXA_MESH_E_NULLPTR, "unwrap: pix_to_face_uv / bary_uv is NULL");
    if (tex_sum && !u->uv_weight) return fail(EXA_MESH_E_NULLPTR, "unwrap: uv_weight is NULL");
    if (u->F > 0 && (!u->faces || !u->verts || !u->focal || !u->princpt))
        return fail(EXA_MESH_E_NULLPTR, "unwrap: faces / verts / focal / princpt is NULL");
    if (pixels > 0 && (!u->img || !u->pix_to_face_xy)) return fail(EXA_MESH_E_NULLPTR, "unwrap: img / pix_to_face_xy is NULL");
    const uint64_t need = align256((uint64_t)u->B * u->F);
    if (need > 0 && !flag_ws) return fail(EXA_MESH_E_NULLPTR, "unwrap: flag_ws is NULL");
    if (ws_bytes < need) return fail(EXA_MESH_E_INVALID, "unwrap: flag_ws is smaller than exa_mesh_unwrap_workspace_size");
    UnwrapArgs a;
    a.u = *u;
    a.flags = static_cast<uint8_t*>(flag_ws);
    a.flag_words = (uint32_t)(need / 4);
    a.uvmap = uvmap; a.mask = mask; a.tex_sum = tex_sum; a.mask_sum = mask_sum;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a.flag_words > 0) {
        hipLaunchKernelGGL(unwrap_clear, dim3(ceil_div(a.flag_words, UW_BLOCK)), dim3(UW_BLOCK), 0, st, a);
        if (int rc = launched("unwrap_clear")) return rc;
        if (pixels > 0) {
            hipLaunchKernelGGL(unwrap_mark, dim3(ceil_div(pixels, UW_BLOCK)), dim3(UW_BLOCK), 0, st, a);
            if (int rc = launched("unwrap_mark")) return rc;
        }
    }
    hipLaunchKernelGGL(unwrap_texels, dim3(ceil_div(texels, UW_BLOCK)), dim3(UW_BLOCK), 0, st, a);
    return launched("unwrap_texels");
}

}  // extern "C"
