// Differentiable triangle rasterizer with a fused UV-texture sample (include/exa_mesh.h): the face render of ExAvatar
// (pytorch3d MeshRasterizer + TexturesUV at reference layer.py:23-68), and a Phong-shaded forward for the mesh panel of
// the reference's render_mesh (vis.py:73-109).  The conventions are derived in the docstring of
// exavatar_release_amd/mesh.py; this file implements them.
//
// Pipeline (wave = 64 lanes, every kernel a plain launch on the caller's stream, no atomics, no memsets):
//   mesh_prep        one thread per (mesh, face): project the corners (fp64), cull, write a 64-byte FaceRec (screen corners
//                    relative to the bbox origin, z,
//                    1/area, inclusive pixel bbox; an empty bbox marks a culled face).
//   mesh_bin         one thread per (mesh, 32-face word, 64x64 cell): the word of the cell's face bitmask.  The mask
//                    array is cells x ceil(F/32) words per mesh -- a size the host knows, so no capacity, no overflow.
//   mesh_raster_fwd  one workgroup per 16x16 tile: filters its cell's mask against the tile into LDS, then every pixel
//                    walks the surviving faces in index order and keeps the nearest (strict <, so the lower index wins
//                    a tie).  Writes pix_to_face, zbuf, bary and -- TEX -- samples the texture into the NCHW render,
//                    or -- SHADE -- Phong-shades the nearest face into the NHWC image (no barycentrics written out).
//                    ORTHO (exa_mesh_forward_ortho, the UV-space raster of the texture unwrap): mesh_prep takes x, y as
//                    they are, and the fragment carries the plain screen barycentrics and their blend of the depths.
//   mesh_vertex_normals  one thread per (mesh, vertex): sums its corners' edge cross products in CSR order, normalises.
//   mesh_bwd_faces   one wave per (mesh, face): walks the face's bbox, keeps the pixels whose pix_to_face is this face,
//                    chains dL/d(bary, zbuf[, render]) to the three corners' camera-space xyz, sums per lane in pixel
//                    order and across the wave by a fixed butterfly.  9 floats per face into grad_ws.
//   mesh_bwd_gather  one thread per (mesh, vertex): sums its (face, corner) entries in CSR order.
// Both backward steps fix their summation order, so the result is bit-identical from call to call.
//
// Compiled with -ffp-contract=off (build.py): the forward's bilinear blend is the expression F.grid_sample evaluates, so
// a blend of four taps that all equal 1 rounds as PyTorch's does (the reference tests `mask == 1`, model.py:200).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/exa_mesh.h"
#include "abi_status.h"
#include "fixed_sum.h"
#include "index_transpose.h"

namespace exa_mesh_impl {

using exa::align256;
using exa::ceil_div;

constexpr int CELL = EXA_MESH_CELL;
constexpr int TILE = EXA_MESH_TILE;
constexpr int BLOCK = 256;
constexpr int MAX_IMAGE = 8192;              // rows / columns
constexpr int64_t MAX_FACES = 1 << 24;       // N * F
constexpr float MIN_Z = 1e-6f;               // faces with any corner at z <= MIN_Z are culled
constexpr float MIN_AREA = 1e-8f;            // |screen area| in square pixels below this: degenerate, skipped

struct alignas(16) FaceRec {
    int bx0, by0, bx1, by1;                  // inclusive pixel bbox; bx0 > bx1 when culled
    float x[3], y[3];                        // screen corners relative to (bx0, by0)
    float z[3];
    float inv_area;
    float pad[2];
};
static_assert(sizeof(FaceRec) == 64, "FaceRec is 64 bytes");

inline int cells_x(int W) { return (W + CELL - 1) / CELL; }
inline int cells_y(int H) { return (H + CELL - 1) / CELL; }
inline int words_of(int F) { return (F + 31) / 32; }

// ---- device helpers ------------------------------------------------------------------------------------------------

struct Bary {
    float b[3];      // screen-space barycentrics
    float w[3];      // b_k / z_k
    float S;         // sum of w
    float p[3];      // perspective-correct barycentrics w_k / S
    float z;         // sum p_k z_k
};

__device__ __forceinline__ void screen_bary(const FaceRec& r, float px, float py, float b[3]) {
    const float e0 = (r.x[1] - px) * (r.y[2] - py) - (r.y[1] - py) * (r.x[2] - px);
    const float e1 = (r.x[2] - px) * (r.y[0] - py) - (r.y[2] - py) * (r.x[0] - px);
    const float e2 = (r.x[0] - px) * (r.y[1] - py) - (r.y[0] - py) * (r.x[1] - px);
    b[0] = e0 * r.inv_area;
    b[1] = e1 * r.inv_area;
    b[2] = e2 * r.inv_area;
}

__device__ __forceinline__ void perspective(const FaceRec& r, Bary& q) {
    q.w[0] = q.b[0] / r.z[0];
    q.w[1] = q.b[1] / r.z[1];
    q.w[2] = q.b[2] / r.z[2];
    q.S = q.w[0] + q.w[1] + q.w[2];
    q.p[0] = q.w[0] / q.S;
    q.p[1] = q.w[1] / q.S;
    q.p[2] = q.w[2] / q.S;
    q.z = q.p[0] * r.z[0] + q.p[1] * r.z[1] + q.p[2] * r.z[2];
}

// The barycentrics a fragment carries.  pytorch3d corrects for perspective only under a perspective camera: with ORTHO
// (exa_mesh_forward_ortho) they are the plain screen barycentrics, and z their blend of the corners' depths.
template <bool ORTHO>
__device__ __forceinline__ void interpolate(const FaceRec& r, Bary& q) {
    if constexpr (ORTHO) {
        q.p[0] = q.b[0];
        q.p[1] = q.b[1];
        q.p[2] = q.b[2];
        q.z = q.p[0] * r.z[0] + q.p[1] * r.z[1] + q.p[2] * r.z[2];
    } else {
        perspective(r, q);
    }
}

// F.grid_sample(flip(map, rows), 2 * uv - 1, bilinear, border, align_corners=True) at one pixel: coordinates and weights.
struct Sample {
    float ix, iy;                // clipped source coordinates in the flipped map
    float fx0, fy0;              // floor(ix), floor(iy)
    int x0, y0;
    bool grad_x, grad_y;         // false where the border clamp is active (zero derivative)
    float nw, ne, sw, se;
};

__device__ __forceinline__ Sample make_sample(float u, float v, int tW, int tH) {
    Sample s;
    const float gx = u * 2.f - 1.f, gy = v * 2.f - 1.f;
    float ix = ((gx + 1.f) / 2.f) * (float)(tW - 1);
    float iy = ((gy + 1.f) / 2.f) * (float)(tH - 1);
    s.grad_x = ix > 0.f && ix < (float)(tW - 1);
    s.grad_y = iy > 0.f && iy < (float)(tH - 1);
    ix = fminf((float)(tW - 1), fmaxf(ix, 0.f));
    iy = fminf((float)(tH - 1), fmaxf(iy, 0.f));
    s.ix = ix;
    s.iy = iy;
    s.fx0 = floorf(ix);
    s.fy0 = floorf(iy);
    s.x0 = (int)s.fx0;
    s.y0 = (int)s.fy0;
    const float fx1 = s.fx0 + 1.f, fy1 = s.fy0 + 1.f;
    s.nw = (fx1 - ix) * (fy1 - iy);
    s.ne = (ix - s.fx0) * (fy1 - iy);
    s.sw = (fx1 - ix) * (iy - s.fy0);
    s.se = (ix - s.fx0) * (iy - s.fy0);
    return s;
}

// tap (x, y) of the FLIPPED map = row tH - 1 - y of the stored one; 0 outside (PyTorch's within_bounds)
__device__ __forceinline__ float tap(const float* plane, int tW, int tH, int x, int y) {
    if (x < 0 || x >= tW || y < 0 || y >= tH) return 0.f;
    return plane[(size_t)(tH - 1 - y) * tW + x];
}

__device__ __forceinline__ bool in_map(int x, int y, int tW, int tH) { return x >= 0 && x < tW && y >= 0 && y < tH; }

struct Params {
    int N, V, F, H, W;
    const float* verts;
    const int32_t* faces;
    const float* focal;
    const float* princpt;
    FaceRec* recs;
    uint32_t* bins;
    int cx, cells, words;
    int ortho;                               // verts hold screen x, y in pixels and the depth: no projection, no focal / princpt
    // outputs / gradients
    int64_t* pix_to_face;
    float* zbuf;
    float* bary;
    float* render;
    const float* dzbuf;
    const float* dbary;
    const float* drender;
    // texture
    int C, tH, tW, tN;
    const float* tex;
    const float* face_uvs;
    // backward
    float* grad;
    const int32_t* offsets;
    const int32_t* entries;
    float* dverts;
    // shaded forward
    const float* normals;
    float* normals_out;
    float* image;
    ExaMeshShading sh;
};

// ---- forward -------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(BLOCK) mesh_prep(Params P) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (int64_t)P.N * P.F) return;
    const int n = (int)(i / P.F), f = (int)(i % P.F);
    FaceRec r;
    r.bx0 = 0; r.by0 = 0; r.bx1 = -1; r.by1 = -1;
    r.pad[0] = r.pad[1] = 0.f;
    // projected in fp64 and stored relative to the face's integer bbox origin: the edge functions then subtract small,
    // exactly representable numbers, and a thin face 500 px off the principal point keeps fp32's relative precision
    double fx = 1.0, fy = 1.0, cx = 0.0, cy = 0.0;
    if (!P.ortho) {
        fx = P.focal[2 * n]; fy = P.focal[2 * n + 1];
        cx = P.princpt[2 * n]; cy = P.princpt[2 * n + 1];
    }
    double sx[3], sy[3];
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        const int v = P.faces[3 * f + k];
        sx[k] = sy[k] = 0.0;
        r.z[k] = 1.f;
        if (v < 0 || v >= P.V) {                 // out-of-range index: culled, nothing read
            ok = false;
            continue;
        }
        const float* p = P.verts + ((size_t)n * P.V + v) * 3;
        const float Z = p[2];
        sx[k] = P.ortho ? (double)p[0] : fx * ((double)p[0] / Z) + cx;
        sy[k] = P.ortho ? (double)p[1] : fy * ((double)p[1] / Z) + cy;
        r.z[k] = Z;
        ok = ok && Z > MIN_Z && isfinite(sx[k]) && isfinite(sy[k]) && isfinite(Z);
    }
    const double area = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sy[1] - sy[0]) * (sx[2] - sx[0]);
    ok = ok && fabs(area) >= (double)MIN_AREA && isfinite(area);
    r.inv_area = ok ? (float)(1.0 / area) : 0.f;
    for (int k = 0; k < 3; ++k) r.x[k] = r.y[k] = 0.f;
    if (ok) {
        // pixel (row i, col j) has its centre at (j + 0.5, i + 0.5); one pixel of slack each way (the inside test decides)
        const double mnx = fmin(sx[0], fmin(sx[1], sx[2])), mxx = fmax(sx[0], fmax(sx[1], sx[2]));
        const double mny = fmin(sy[0], fmin(sy[1], sy[2])), mxy = fmax(sy[0], fmax(sy[1], sy[2]));
        const double jlo = fmax(floor(mnx - 0.5), 0.0), jhi = fmin(ceil(mxx - 0.5), (double)(P.W - 1));
        const double ilo = fmax(floor(mny - 0.5), 0.0), ihi = fmin(ceil(mxy - 0.5), (double)(P.H - 1));
        if (jlo <= jhi && ilo <= ihi) {
            r.bx0 = (int)jlo; r.bx1 = (int)jhi;
            r.by0 = (int)ilo; r.by1 = (int)ihi;
            for (int k = 0; k < 3; ++k) {
                r.x[k] = (float)(sx[k] - jlo);
                r.y[k] = (float)(sy[k] - ilo);
            }
        }
    }
    P.recs[i] = r;
}

__global__ void __launch_bounds__(BLOCK) mesh_bin(Params P) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (int64_t)P.N * P.words * P.cells) return;
    const int c = (int)(i % P.cells);
    const int64_t nw = i / P.cells;
    const int w = (int)(nw % P.words), n = (int)(nw / P.words);
    const int x0 = (c % P.cx) * CELL, y0 = (c / P.cx) * CELL;
    const int x1 = x0 + CELL - 1, y1 = y0 + CELL - 1;
    uint32_t m = 0;
    const int fend = min(32, P.F - 32 * w);
    const FaceRec* recs = P.recs + (size_t)n * P.F + 32 * w;
    for (int b = 0; b < fend; ++b) {
        const int4 bb = *reinterpret_cast<const int4*>(&recs[b].bx0);
        if (bb.x <= x1 && bb.z >= x0 && bb.y <= y1 && bb.w >= y0) m |= 1u << b;
    }
    P.bins[((size_t)n * P.cells + c) * P.words + w] = m;
}

// x / max(|x|, 1e-6): F.normalize's eps, as pytorch3d's lighting applies it
__device__ __forceinline__ void normalize3(float v[3]) {
    const float d = fmaxf(sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), 1e-6f);
    v[0] = v[0] / d;
    v[1] = v[1] / d;
    v[2] = v[2] / d;
}

// pytorch3d phong_shading at one pixel (include/exa_mesh.h, ExaMeshShading): pos / nrm are the interpolated position and
// normal in the caller's camera frame
__device__ __forceinline__ void phong(const ExaMeshShading& sh, const float pos[3], const float nrm[3], float out[3]) {
    float n[3] = {nrm[0], nrm[1], nrm[2]};
    float l[3] = {sh.light_location[0] - pos[0], sh.light_location[1] - pos[1], sh.light_location[2] - pos[2]};
    float v[3] = {-pos[0], -pos[1], -pos[2]};
    normalize3(n);
    normalize3(l);
    normalize3(v);
    const float cosv = n[0] * l[0] + n[1] * l[1] + n[2] * l[2];
    const float diff = fmaxf(cosv, 0.f);
    float vr = 0.f;
    for (int k = 0; k < 3; ++k) vr += v[k] * (-l[k] + 2.f * cosv * n[k]);
    const float a = cosv > 0.f ? fmaxf(vr, 0.f) : 0.f;
    const float spec = powf(a, sh.shininess);          // powf(0, 0) = 1, as torch.pow
    for (int c = 0; c < 3; ++c)
        out[c] = (sh.light_ambient[c] * sh.material_ambient[c] + sh.material_diffuse[c] * (sh.light_diffuse[c] * diff)) +
                 sh.material_specular[c] * (sh.light_specular[c] * spec);
}

template <bool TEX, bool SHADE = false, bool ORTHO = false>
__global__ void __launch_bounds__(BLOCK) mesh_raster_fwd(Params P) {
    __shared__ uint32_t s_mask[BLOCK];
    __shared__ uint64_t s_nz[BLOCK / 64];
    const int t = threadIdx.x, n = blockIdx.z;
    const int tx0 = blockIdx.x * TILE, ty0 = blockIdx.y * TILE;
    const int tx1 = min(tx0 + TILE - 1, P.W - 1), ty1 = min(ty0 + TILE - 1, P.H - 1);
    const int x = tx0 + (t % TILE), y = ty0 + (t / TILE);
    const int cell = (ty0 / CELL) * P.cx + tx0 / CELL;
    const uint32_t* cm = P.bins + ((size_t)n * P.cells + cell) * P.words;
    const FaceRec* recs = P.recs + (size_t)n * P.F;
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;

    int best = -1;
    float bz = INFINITY;
    for (int c0 = 0; c0 < P.words; c0 += BLOCK) {
        // the cell's word c0 + t, filtered to the faces whose bbox meets this tile
        uint32_t m = 0;
        if (c0 + t < P.words) {
            uint32_t cw = cm[c0 + t];
            while (cw) {
                const int b = __ffs(cw) - 1;
                cw &= cw - 1;
                const int4 bb = *reinterpret_cast<const int4*>(&recs[(c0 + t) * 32 + b].bx0);
                if (bb.x <= tx1 && bb.z >= tx0 && bb.y <= ty1 && bb.w >= ty0) m |= 1u << b;
            }
        }
        s_mask[t] = m;
        const uint64_t nz = __ballot(m != 0);
        if ((t & 63) == 0) s_nz[t >> 6] = nz;
        __syncthreads();
        for (int q = 0; q < BLOCK / 64; ++q) {
            uint64_t wz = s_nz[q];
            wz = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(wz >> 32)) << 32) |
                 (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)wz);
            while (wz) {
                const int l = __ffsll((unsigned long long)wz) - 1;
                wz &= wz - 1;
                uint32_t mm = __builtin_amdgcn_readfirstlane(s_mask[q * 64 + l]);
                while (mm) {
                    const int b = __ffs(mm) - 1;
                    mm &= mm - 1;
                    const int f = (c0 + q * 64 + l) * 32 + b;
                    const FaceRec r = recs[f];
                    float bb[3];
                    screen_bary(r, px - (float)r.bx0, py - (float)r.by0, bb);
                    if (bb[0] > 0.f && bb[1] > 0.f && bb[2] > 0.f) {
                        Bary qb;
                        qb.b[0] = bb[0]; qb.b[1] = bb[1]; qb.b[2] = bb[2];
                        interpolate<ORTHO>(r, qb);
                        if (qb.z < bz) {          // faces arrive in index order: strict < keeps the lower index on a tie
                            bz = qb.z;
                            best = f;
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    if (x >= P.W || y >= P.H) return;
    const size_t pix = ((size_t)n * P.H + y) * P.W + x;
    Bary qb;
    if (best >= 0) {
        const FaceRec r = recs[best];
        screen_bary(r, px - (float)r.bx0, py - (float)r.by0, qb.b);
        interpolate<ORTHO>(r, qb);
    }
    if (!SHADE || P.pix_to_face) P.pix_to_face[pix] = best >= 0 ? (int64_t)n * P.F + best : -1;
    if (P.zbuf) P.zbuf[pix] = best >= 0 ? qb.z : -1.f;
    if (P.bary) {
        P.bary[3 * pix + 0] = best >= 0 ? qb.p[0] : -1.f;
        P.bary[3 * pix + 1] = best >= 0 ? qb.p[1] : -1.f;
        P.bary[3 * pix + 2] = best >= 0 ? qb.p[2] : -1.f;
    }
    if constexpr (TEX) {
        const size_t plane = (size_t)P.H * P.W, out0 = (size_t)n * P.C * plane + (size_t)y * P.W + x;
        if (best < 0) {
            for (int c = 0; c < P.C; ++c) P.render[out0 + c * plane] = -1.f;
            return;
        }
        const float* uv = P.face_uvs + (size_t)best * 6;
        const float u = qb.p[0] * uv[0] + qb.p[1] * uv[2] + qb.p[2] * uv[4];
        const float v = qb.p[0] * uv[1] + qb.p[1] * uv[3] + qb.p[2] * uv[5];
        const Sample s = make_sample(u, v, P.tW, P.tH);
        const size_t tplane = (size_t)P.tH * P.tW;
        const float* tex = P.tex + (P.tN == 1 ? 0 : (size_t)n * P.C * tplane);
        for (int c = 0; c < P.C; ++c) {
            const float* pl = tex + c * tplane;
            float o = 0.f;          // F.grid_sample's accumulation: nw, ne, sw, se, each tap only when inside the map
            if (in_map(s.x0, s.y0, P.tW, P.tH)) o += tap(pl, P.tW, P.tH, s.x0, s.y0) * s.nw;
            if (in_map(s.x0 + 1, s.y0, P.tW, P.tH)) o += tap(pl, P.tW, P.tH, s.x0 + 1, s.y0) * s.ne;
            if (in_map(s.x0, s.y0 + 1, P.tW, P.tH)) o += tap(pl, P.tW, P.tH, s.x0, s.y0 + 1) * s.sw;
            if (in_map(s.x0 + 1, s.y0 + 1, P.tW, P.tH)) o += tap(pl, P.tW, P.tH, s.x0 + 1, s.y0 + 1) * s.se;
            P.render[out0 + c * plane] = o;
        }
    }
    if constexpr (SHADE) {
        float* out = P.image + 3 * pix;
        if (best < 0) {
            for (int c = 0; c < 3; ++c) out[c] = P.sh.background[c];
            return;
        }
        // the winner passed mesh_prep, so its three indices are in [0, V)
        float pos[3] = {0.f, 0.f, 0.f}, nrm[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < 3; ++k) {
            const size_t o = ((size_t)n * P.V + P.faces[3 * best + k]) * 3;
            for (int d = 0; d < 3; ++d) {
                pos[d] += qb.p[k] * P.verts[o + d];
                nrm[d] += qb.p[k] * P.normals[o + d];
            }
        }
        float rgb[3];
        phong(P.sh, pos, nrm, rgb);
        for (int c = 0; c < 3; ++c) out[c] = rgb[c];
    }
}

// ---- vertex normals ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(BLOCK) mesh_vertex_normals(Params P) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (int64_t)P.N * P.V) return;
    const int n = (int)(i / P.V), v = (int)(i % P.V);
    const float* verts = P.verts + (size_t)n * P.V * 3;
    float s[3] = {0.f, 0.f, 0.f};
    for (int e = P.offsets[v]; e < P.offsets[v + 1]; ++e) {
        const int fc = P.entries[e];
        if (fc < 0 || fc >= 3 * P.F) continue;
        const int f = fc / 3, k = fc % 3;
        const int a = P.faces[3 * f + k], b = P.faces[3 * f + (k + 1) % 3], c = P.faces[3 * f + (k + 2) % 3];
        if (a < 0 || a >= P.V || b < 0 || b >= P.V || c < 0 || c >= P.V) continue;
        // corner k adds (v_{k+1} - v_k) x (v_{k+2} - v_k)
        const float* pa = verts + 3 * (size_t)a;
        const float* pb = verts + 3 * (size_t)b;
        const float* pc = verts + 3 * (size_t)c;
        const float e1[3] = {pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]};
        const float e2[3] = {pc[0] - pa[0], pc[1] - pa[1], pc[2] - pa[2]};
        s[0] += e1[1] * e2[2] - e1[2] * e2[1];
        s[1] += e1[2] * e2[0] - e1[0] * e2[2];
        s[2] += e1[0] * e2[1] - e1[1] * e2[0];
    }
    normalize3(s);
    P.normals_out[3 * i + 0] = s[0];
    P.normals_out[3 * i + 1] = s[1];
    P.normals_out[3 * i + 2] = s[2];
}

// ---- backward ------------------------------------------------------------------------------------------------------

template <bool TEX>
__global__ void __launch_bounds__(BLOCK) mesh_bwd_faces(Params P) {
    const int lane = threadIdx.x & 63;
    const int64_t gw = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (gw >= (int64_t)P.N * P.F) return;                   // whole waves leave together
    const int n = (int)(gw / P.F), f = (int)(gw % P.F);
    const FaceRec r = P.recs[gw];
    float acc[9];                                           // d/d(screen x, screen y, z) of corners 0, 1, 2
    for (int k = 0; k < 9; ++k) acc[k] = 0.f;
    const int bw = r.bx1 - r.bx0 + 1, bh = r.by1 - r.by0 + 1;
    const int area = (bw > 0 && bh > 0) ? bw * bh : 0;
    const float* uv = P.face_uvs + (size_t)f * 6;
    const size_t tplane = (size_t)P.tH * P.tW, plane = (size_t)P.H * P.W;
    for (int idx = lane; idx < area; idx += 64) {
        const int x = r.bx0 + idx % bw, y = r.by0 + idx / bw;
        const size_t pix = ((size_t)n * P.H + y) * P.W + x;
        if (P.pix_to_face[pix] != gw) continue;
        const float px = (float)(x - r.bx0) + 0.5f, py = (float)(y - r.by0) + 0.5f;     // face-relative
        Bary q;
        screen_bary(r, px, py, q.b);
        perspective(r, q);
        float G[3] = {0.f, 0.f, 0.f}, dz[3];
        if (P.dbary) {
            G[0] = P.dbary[3 * pix + 0];
            G[1] = P.dbary[3 * pix + 1];
            G[2] = P.dbary[3 * pix + 2];
        }
        if constexpr (TEX) {
            if (P.drender) {
                const float u = q.p[0] * uv[0] + q.p[1] * uv[2] + q.p[2] * uv[4];
                const float v = q.p[0] * uv[1] + q.p[1] * uv[3] + q.p[2] * uv[5];
                const Sample s = make_sample(u, v, P.tW, P.tH);
                const float* tex = P.tex + (P.tN == 1 ? 0 : (size_t)n * P.C * tplane);
                const float fx1 = s.fx0 + 1.f, fy1 = s.fy0 + 1.f;
                float gix = 0.f, giy = 0.f;
                for (int c = 0; c < P.C; ++c) {
                    const float g = P.drender[((size_t)n * P.C + c) * plane + (size_t)y * P.W + x];
                    const float* pl = tex + c * tplane;
                    const float vnw = tap(pl, P.tW, P.tH, s.x0, s.y0), vne = tap(pl, P.tW, P.tH, s.x0 + 1, s.y0);
                    const float vsw = tap(pl, P.tW, P.tH, s.x0, s.y0 + 1), vse = tap(pl, P.tW, P.tH, s.x0 + 1, s.y0 + 1);
                    gix += g * (-vnw * (fy1 - s.iy) + vne * (fy1 - s.iy) - vsw * (s.iy - s.fy0) + vse * (s.iy - s.fy0));
                    giy += g * (-vnw * (fx1 - s.ix) - vne * (s.ix - s.fx0) + vsw * (fx1 - s.ix) + vse * (s.ix - s.fx0));
                }
                const float du = s.grad_x ? gix * (float)(P.tW - 1) : 0.f;
                const float dv = s.grad_y ? giy * (float)(P.tH - 1) : 0.f;
                G[0] += du * uv[0] + dv * uv[1];
                G[1] += du * uv[2] + dv * uv[3];
                G[2] += du * uv[4] + dv * uv[5];
            }
        }
        const float gz = P.dzbuf ? P.dzbuf[pix] : 0.f;
        // zbuf = sum p_k z_k
        for (int k = 0; k < 3; ++k) {
            G[k] += gz * r.z[k];
            dz[k] = gz * q.p[k];
        }
        // p_k = w_k / S, w_k = b_k / z_k
        const float dot = G[0] * q.p[0] + G[1] * q.p[1] + G[2] * q.p[2];
        const float invS = 1.f / q.S;
        float db[3];
        for (int k = 0; k < 3; ++k) {
            const float dw = (G[k] - dot) * invS;
            db[k] = dw / r.z[k];
            dz[k] -= dw * q.w[k] / r.z[k];
        }
        // b_k = E_k / A,  E_k = cross(s_{k+1} - p, s_{k+2} - p),  A = cross(s_1 - s_0, s_2 - s_0)
        const float dA = -(db[0] * q.b[0] + db[1] * q.b[1] + db[2] * q.b[2]) * r.inv_area;
        for (int k = 0; k < 3; ++k) {
            const int k1 = k == 2 ? 0 : k + 1, k2 = k == 0 ? 2 : k - 1;
            const float dE = db[k] * r.inv_area;
            acc[3 * k1 + 0] += dE * (r.y[k2] - py);
            acc[3 * k1 + 1] -= dE * (r.x[k2] - px);
            acc[3 * k2 + 0] -= dE * (r.y[k1] - py);
            acc[3 * k2 + 1] += dE * (r.x[k1] - px);
            acc[3 * k + 0] += dA * (r.y[k1] - r.y[k2]);
            acc[3 * k + 1] += dA * (r.x[k2] - r.x[k1]);
            acc[3 * k + 2] += dz[k];
        }
    }
    for (int k = 0; k < 9; ++k) exa::wave_sum_all(acc[k]);
    if (lane != 0) return;
    float* out = P.grad + gw * 9;
    if (area == 0) {
        for (int k = 0; k < 9; ++k) out[k] = 0.f;
        return;
    }
    const float fx = P.focal[2 * n], fy = P.focal[2 * n + 1];
    for (int k = 0; k < 3; ++k) {           // u = fx X / Z + cx, v = fy Y / Z + cy, z = Z
        const float* p = P.verts + ((size_t)n * P.V + P.faces[3 * f + k]) * 3;
        const float X = p[0], Y = p[1], Z = p[2];
        const float gu = acc[3 * k], gv = acc[3 * k + 1];
        out[3 * k + 0] = gu * fx / Z;
        out[3 * k + 1] = gv * fy / Z;
        out[3 * k + 2] = acc[3 * k + 2] - (gu * fx * X + gv * fy * Y) / (Z * Z);
    }
}

__global__ void __launch_bounds__(BLOCK) mesh_bwd_gather(Params P) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (int64_t)P.N * P.V) return;
    const int n = (int)(i / P.V), v = (int)(i % P.V);
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    const float* grad = P.grad + (size_t)n * P.F * 9;
    for (int e = P.offsets[v]; e < P.offsets[v + 1]; ++e) {
        const int fc = P.entries[e];
        const float* src = grad + (size_t)(fc / 3) * 9 + (fc % 3) * 3;
        g0 += src[0];
        g1 += src[1];
        g2 += src[2];
    }
    P.dverts[3 * i + 0] = g0;
    P.dverts[3 * i + 1] = g1;
    P.dverts[3 * i + 2] = g2;
}

// ---- host side -----------------------------------------------------------------------------------------------------

EXA_ABI_STATUS("exa_mesh")

int check_shape(int32_t N, int32_t V, int32_t F, int32_t H, int32_t W) {
    if (N < 0 || V < 0 || F < 0 || H < 0 || W < 0) return fail(EXA_MESH_E_INVALID, "negative size");
    if (H > MAX_IMAGE || W > MAX_IMAGE) return fail(EXA_MESH_E_INVALID, "image larger than 8192 x 8192");
    if ((int64_t)N * F > MAX_FACES || (int64_t)N * V > MAX_FACES * 3)
        return fail(EXA_MESH_E_INVALID, "more than 2^24 faces (N * F) in one call");
    return 0;
}

int fill(const ExaMeshGeometry* g, const ExaMeshTexture* tex, Params& P, bool ortho = false) {
    if (!g) return fail(EXA_MESH_E_NULLPTR, "geometry is NULL");
    if (int rc = check_shape(g->N, g->V, g->F, g->H, g->W)) return rc;
    memset(&P, 0, sizeof(P));
    P.N = g->N; P.V = g->V; P.F = g->F; P.H = g->H; P.W = g->W;
    P.verts = g->verts; P.faces = g->faces; P.focal = g->focal; P.princpt = g->princpt;
    P.cx = cells_x(g->W);
    P.cells = P.cx * cells_y(g->H);
    P.words = words_of(g->F);
    if (g->N > 0 && g->F > 0) {
        if (g->V > 0 && !g->verts) return fail(EXA_MESH_E_NULLPTR, "verts is NULL");
        if (!g->faces || (!ortho && (!g->focal || !g->princpt)))
            return fail(EXA_MESH_E_NULLPTR, "faces / focal / princpt is NULL");
    }
    P.ortho = ortho ? 1 : 0;
    if (tex) {
        if (tex->C < 1 || tex->C > EXA_MESH_MAX_CHANNELS) return fail(EXA_MESH_E_INVALID, "texture channels must be 1 .. 8");
        if (tex->tex_H < 1 || tex->tex_W < 1 || tex->tex_H > 65536 || tex->tex_W > 65536)
            return fail(EXA_MESH_E_INVALID, "texture size must be 1 .. 65536 per side");
        if (tex->tex_N != 1 && tex->tex_N != g->N) return fail(EXA_MESH_E_INVALID, "tex_N must be 1 or N");
        if (!tex->texture || (g->F > 0 && !tex->face_uvs)) return fail(EXA_MESH_E_NULLPTR, "texture / face_uvs is NULL");
        P.C = tex->C; P.tH = tex->tex_H; P.tW = tex->tex_W; P.tN = tex->tex_N;
        P.tex = tex->texture; P.face_uvs = tex->face_uvs;
    }
    return 0;
}

// mesh_prep + mesh_bin of a forward (nothing to do without faces)
int launch_prep_bin(const Params& P, hipStream_t st) {
    const int64_t nf = (int64_t)P.N * P.F;
    if (nf == 0) return 0;
    hipLaunchKernelGGL(mesh_prep, dim3(ceil_div(nf, BLOCK)), dim3(BLOCK), 0, st, P);
    if (int rc = launched("mesh_prep")) return rc;
    hipLaunchKernelGGL(mesh_bin, dim3(ceil_div((int64_t)P.N * P.words * P.cells, BLOCK)), dim3(BLOCK), 0, st, P);
    return launched("mesh_bin");
}

dim3 raster_grid(const Params& P) { return dim3((P.W + TILE - 1) / TILE, (P.H + TILE - 1) / TILE, P.N); }

}  // namespace exa_mesh_impl

using namespace exa_mesh_impl;

extern "C" {

int exa_mesh_version(void) { return EXA_MESH_VERSION; }

const char* exa_mesh_last_error(void) { return g_err; }

int exa_mesh_workspace_sizes(int32_t N, int32_t F, int32_t H, int32_t W, ExaMeshWorkspaceSizes* out) {
    if (!out) return fail(EXA_MESH_E_NULLPTR, "out is NULL");
    if (int rc = check_shape(N, 0, F, H, W)) return rc;
    out->face_bytes = align256((uint64_t)N * F * sizeof(FaceRec));
    out->bin_bytes = align256((uint64_t)N * cells_x(W) * cells_y(H) * words_of(F) * 4);
    out->grad_bytes = align256((uint64_t)N * F * 9 * 4);
    return 0;
}

int exa_mesh_vertex_faces(int32_t V, int32_t F, const int32_t* faces, int32_t* offsets, int32_t* entries) {
    if (V < 0 || F < 0 || (int64_t)F * 3 > INT32_MAX) return fail(EXA_MESH_E_INVALID, "bad V / F");
    if (!offsets || (F > 0 && (!faces || !entries))) return fail(EXA_MESH_E_NULLPTR, "NULL argument");
    // ascending (face, corner) per vertex: the shared index transpose (index_transpose.h)
    if (exa::index_transpose(V, (int64_t)F * 3, faces, false, offsets, entries) >= 0)
        return fail(EXA_MESH_E_INVALID, "face index out of range");
    return 0;
}

int exa_mesh_forward(const ExaMeshGeometry* g, const ExaMeshTexture* tex, void* face_ws, void* bin_ws,
                     int64_t* pix_to_face, float* zbuf, float* bary, float* render, void* stream) {
    Params P;
    if (int rc = fill(g, tex, P)) return rc;
    const int64_t npix = (int64_t)P.N * P.H * P.W;
    if (npix == 0) return 0;
    if (!pix_to_face) return fail(EXA_MESH_E_NULLPTR, "pix_to_face is NULL");
    if (tex && !render) return fail(EXA_MESH_E_NULLPTR, "render is NULL");
    if (P.F > 0 && (!face_ws || !bin_ws)) return fail(EXA_MESH_E_NULLPTR, "workspace is NULL");
    P.recs = static_cast<FaceRec*>(face_ws);
    P.bins = static_cast<uint32_t*>(bin_ws);
    P.pix_to_face = pix_to_face; P.zbuf = zbuf; P.bary = bary; P.render = render;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = launch_prep_bin(P, st)) return rc;
    const dim3 grid = raster_grid(P);
    if (tex)
        hipLaunchKernelGGL(mesh_raster_fwd<true>, grid, dim3(BLOCK), 0, st, P);
    else
        hipLaunchKernelGGL(mesh_raster_fwd<false>, grid, dim3(BLOCK), 0, st, P);
    return launched("mesh_raster_fwd");
}

int exa_mesh_forward_ortho(const ExaMeshGeometry* g, void* face_ws, void* bin_ws, int64_t* pix_to_face, float* zbuf,
                           float* bary, void* stream) {
    Params P;
    if (int rc = fill(g, nullptr, P, true)) return rc;
    const int64_t npix = (int64_t)P.N * P.H * P.W;
    if (npix == 0) return 0;
    if (!pix_to_face) return fail(EXA_MESH_E_NULLPTR, "pix_to_face is NULL");
    if (P.F > 0 && (!face_ws || !bin_ws)) return fail(EXA_MESH_E_NULLPTR, "workspace is NULL");
    P.recs = static_cast<FaceRec*>(face_ws);
    P.bins = static_cast<uint32_t*>(bin_ws);
    P.pix_to_face = pix_to_face; P.zbuf = zbuf; P.bary = bary;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = launch_prep_bin(P, st)) return rc;
    hipLaunchKernelGGL((mesh_raster_fwd<false, false, true>), raster_grid(P), dim3(BLOCK), 0, st, P);
    return launched("mesh_raster_fwd (ortho)");
}

int exa_mesh_backward(const ExaMeshGeometry* g, const ExaMeshTexture* tex, const void* face_ws,
                      const int64_t* pix_to_face, const float* dL_dzbuf, const float* dL_dbary, const float* dL_drender,
                      const int32_t* vert_offsets, const int32_t* vert_entries, void* grad_ws, float* dL_dverts,
                      void* stream) {
    Params P;
    if (int rc = fill(g, tex, P)) return rc;
    if (dL_drender && !tex) return fail(EXA_MESH_E_INVALID, "dL_drender needs the texture");
    const int64_t nv = (int64_t)P.N * P.V, nf = (int64_t)P.N * P.F;
    if (nv == 0) return 0;
    if (!dL_dverts || !vert_offsets) return fail(EXA_MESH_E_NULLPTR, "dL_dverts / vert_offsets is NULL");
    if (nf > 0 && (!face_ws || !grad_ws || !vert_entries || (P.H * P.W > 0 && !pix_to_face)))
        return fail(EXA_MESH_E_NULLPTR, "face_ws / grad_ws / vert_entries / pix_to_face is NULL");
    P.recs = const_cast<FaceRec*>(static_cast<const FaceRec*>(face_ws));
    P.pix_to_face = const_cast<int64_t*>(pix_to_face);
    P.dzbuf = dL_dzbuf; P.dbary = dL_dbary; P.drender = dL_drender;
    P.grad = static_cast<float*>(grad_ws);
    P.offsets = vert_offsets; P.entries = vert_entries; P.dverts = dL_dverts;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nf > 0) {
        const dim3 grid(ceil_div(nf, BLOCK / 64));
        if (tex && dL_drender)
            hipLaunchKernelGGL(mesh_bwd_faces<true>, grid, dim3(BLOCK), 0, st, P);
        else
            hipLaunchKernelGGL(mesh_bwd_faces<false>, grid, dim3(BLOCK), 0, st, P);
        if (int rc = launched("mesh_bwd_faces")) return rc;
    }
    hipLaunchKernelGGL(mesh_bwd_gather, dim3(ceil_div(nv, BLOCK)), dim3(BLOCK), 0, st, P);
    return launched("mesh_bwd_gather");
}

int exa_mesh_vertex_normals(const ExaMeshGeometry* g, const int32_t* vert_offsets, const int32_t* vert_entries,
                            float* normals, void* stream) {
    if (!g) return fail(EXA_MESH_E_NULLPTR, "geometry is NULL");
    if (int rc = check_shape(g->N, g->V, g->F, 0, 0)) return rc;       // H, W, focal and princpt are not used
    if (g->N < 1) return fail(EXA_MESH_E_INVALID, "N must be at least 1");
    if (g->V == 0) return 0;
    if (!normals || !vert_offsets || !g->verts) return fail(EXA_MESH_E_NULLPTR, "normals / vert_offsets / verts is NULL");
    if (g->F > 0 && (!vert_entries || !g->faces)) return fail(EXA_MESH_E_NULLPTR, "vert_entries / faces is NULL");
    Params P;
    memset(&P, 0, sizeof(P));
    P.N = g->N; P.V = g->V; P.F = g->F;
    P.verts = g->verts; P.faces = g->faces;
    P.offsets = vert_offsets; P.entries = vert_entries; P.normals_out = normals;
    hipLaunchKernelGGL(mesh_vertex_normals, dim3(ceil_div((int64_t)P.N * P.V, BLOCK)), dim3(BLOCK), 0,
                       static_cast<hipStream_t>(stream), P);
    return launched("mesh_vertex_normals");
}

int exa_mesh_forward_shaded(const ExaMeshGeometry* g, const ExaMeshShading* shading, const float* normals, void* face_ws,
                            void* bin_ws, int64_t* pix_to_face, float* zbuf, float* image, void* stream) {
    Params P;
    if (int rc = fill(g, nullptr, P)) return rc;
    if (P.N < 1) return fail(EXA_MESH_E_INVALID, "N must be at least 1");
    if (!shading) return fail(EXA_MESH_E_NULLPTR, "shading is NULL");
    if (!(shading->shininess >= 0.f) || !isfinite(shading->shininess))
        return fail(EXA_MESH_E_INVALID, "shininess must be finite and >= 0");
    if (!image) return fail(EXA_MESH_E_NULLPTR, "image is NULL");
    if (P.F > 0 && (!normals || !face_ws || !bin_ws)) return fail(EXA_MESH_E_NULLPTR, "normals / workspace is NULL");
    if ((int64_t)P.H * P.W == 0) return 0;
    P.recs = static_cast<FaceRec*>(face_ws);
    P.bins = static_cast<uint32_t*>(bin_ws);
    P.pix_to_face = pix_to_face; P.zbuf = zbuf; P.image = image;
    P.normals = normals;
    P.sh = *shading;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = launch_prep_bin(P, st)) return rc;
    hipLaunchKernelGGL((mesh_raster_fwd<false, true>), raster_grid(P), dim3(BLOCK), 0, st, P);
    return launched("mesh_raster_fwd (shaded)");
}

}  // extern "C"
