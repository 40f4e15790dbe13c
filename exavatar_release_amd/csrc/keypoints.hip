// The keypoint path of the fitting (include/exa_mesh.h, "KEYPOINTS" and "COORD LOSS"; the reference's tail of the SMPL-X
// layer, smplx/body_models.py:1257-1283, the tail of get_smplx_coord / get_flame_coord, fitting/main/model.py:97-117, 140-157,
// and CoordLoss, fitting/common/nets/loss.py:9-71).  The semantics -- every operation in fp32 in a stated order -- are written
// out in the header; this file implements them.
//
//   kpt_fwd           one workgroup per item: the yaw bin (every thread forms it from the same loads, so it is uniform), the
//                     root row through LDS, then one keypoint per thread: raw row, camera coordinates, projection.
//   kpt_mesh          one thread per (b, vertex): mesh_cam from the root row that kpt_fwd stored.
//   kpt_bwd_sums      workgroup (g, b): the per-workgroup sums of g_mesh (block_sums, the house sum).
//   kpt_bwd_rows      one workgroup per item: the cotangent c_k and its projection share p_k per keypoint into the workspace,
//                     their sequential sums, the root's raw cotangent, d_trans, and one joint per thread over the inverse table.
//   kpt_bwd_vertices  one thread per (b, vertex): g_mesh, then the vertex's CSR entries in order.
//   coord_fwd         one wave per item: every lane walks both hands' 2 x n rows itself (the loads are uniform), so the sums,
//                     the boxes and the decision are sequential and the same in every lane; then lanes own keypoints.
//   coord_bwd         one thread per element.
// The rows are read with 4-byte loads: the arrays may start at any 4-byte boundary.  No atomics, no memsets, no
// allocation, no synchronisation: every output element is one thread's value in the header's order.  Compiled with
// -ffp-contract=off (build.py): no product is contracted into a fused multiply-add; the two fmaf() of a landmark row are
// written out, because that is the header's definition of the row (the order of the reference's einsum on the device).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/exa_mesh.h"
#include "abi_status.h"
#include "fixed_sum.h"

namespace exa_mesh_impl {

using exa::ceil_div;

EXA_ABI_STATUS_SHARED("exa_mesh")         // exa_mesh_last_error() and its buffer are mesh_raster.hip's

namespace {

constexpr int KPT_BLOCK = EXA_MESH_KPT_ROWS;
constexpr int KPT_BINS = EXA_MESH_KPT_BINS;
constexpr int64_t KPT_MAX_ELEMS = 1 << 30;    // elements of any one array
constexpr int KPT_MAX_BATCH = 65535;          // B is a grid dimension of the partial sums
static_assert(KPT_BLOCK == 256, "block_sums is written out for four waves");

__device__ __forceinline__ float kpt_qnan() { return __int_as_float(0x7fc00000); }

struct KptArgs {
    ExaMeshKeypoints t;
    int32_t B, root_rel, blocks;
    const float* vertices; const float* joints; const float* rot; const float* trans;
    const float* focal; const float* princpt;
    const int32_t* bin_in;                    // the forward's yaw_bin, for the backward
    const float* g_cam; const float* g_proj; const float* g_root; const float* g_mesh;
    float* kpt_cam; float* root_cam; float* kpt_proj; float* mesh_cam; int32_t* yaw_bin;
    float* rows;                              // [B, 2 K + 1, 3]: c_0 .. c_{K-1}, the root's raw cotangent, p_0 .. p_{K-1}
    float* partials;                          // [B, 3, blocks]
    float* d_vertices; float* d_joints; float* d_trans;
};

// the header's "yaw bin" of item b; the same in every thread that calls it
__device__ __forceinline__ int kpt_yaw_bin(const KptArgs& a, int b) {
    float rel[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    for (int i = 0; i < a.t.C; ++i) {
        const int j = a.t.chain[i];
        if ((unsigned)j >= (unsigned)a.t.J) return 0;          // the guard: nothing outside rot is read
        const float* R = a.rot + ((int64_t)b * a.t.J + j) * 9;
        float m[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                m[r * 3 + c] = (R[r * 3 + 0] * rel[c] + R[r * 3 + 1] * rel[3 + c]) + R[r * 3 + 2] * rel[6 + c];
#pragma unroll
        for (int q = 0; q < 9; ++q) rel[q] = m[q];
    }
    const float sy = sqrtf(rel[0] * rel[0] + rel[3] * rel[3]);
    const float ang = atan2f(-rel[6], sy);
    const float deg = ((-ang) * 180.0f) / 3.14159274101257324f;
    if (!(fabsf(deg) <= 3.0e38f)) return 0;                    // NaN or infinite
    const float y = rintf(deg < 39.0f ? deg : 39.0f);          // half to even
    int bin = y >= 0.0f ? (int)y : (y >= -39.0f ? 39 - (int)y : 78);
    bin = bin < 0 ? 0 : (bin > KPT_BINS - 1 ? KPT_BINS - 1 : bin);
    return bin;
}

__device__ __forceinline__ int kpt_clamp_bin(int bin) { return bin < 0 ? 0 : (bin > KPT_BINS - 1 ? KPT_BINS - 1 : bin); }

// the raw row of record k (record K is the root) of item b under yaw bin `bin`
__device__ __forceinline__ void kpt_raw_row(const KptArgs& a, int b, int k, int bin, float* out) {
    const int32_t* r = a.t.rec + (int64_t)k * 4;
    const int kind = r[0];
    out[0] = out[1] = out[2] = kpt_qnan();                     // the guard's value: an index outside its table reads nothing
    if (kind == EXA_MESH_KPT_JOINT) {
        if ((unsigned)r[1] >= (unsigned)a.t.J) return;
        const float* p = a.joints + ((int64_t)b * a.t.J + r[1]) * 3;
        out[0] = p[0]; out[1] = p[1]; out[2] = p[2];
        return;
    }
    const float* vb = a.vertices + (int64_t)b * a.t.V * 3;
    if (kind == EXA_MESH_KPT_VERTEX) {
        if ((unsigned)r[1] >= (unsigned)a.t.V) return;
        const float* p = vb + (int64_t)r[1] * 3;
        out[0] = p[0]; out[1] = p[1]; out[2] = p[2];
        return;
    }
    int v[3];
    float w[3];
    if (kind == EXA_MESH_KPT_STATIC) {
#pragma unroll
        for (int i = 0; i < 3; ++i) { v[i] = r[1 + i]; w[i] = a.t.rec_w[(int64_t)k * 3 + i]; }
    } else if (kind == EXA_MESH_KPT_DYNAMIC) {
        if ((unsigned)r[1] >= (unsigned)a.t.Ld) return;
        const int64_t base = ((int64_t)bin * a.t.Ld + r[1]) * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) { v[i] = a.t.dyn_vtx[base + i]; w[i] = a.t.dyn_w[base + i]; }
    } else {
        return;
    }
    if ((unsigned)v[0] >= (unsigned)a.t.V || (unsigned)v[1] >= (unsigned)a.t.V || (unsigned)v[2] >= (unsigned)a.t.V) return;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        out[c] = fmaf(vb[(int64_t)v[2] * 3 + c], w[2], fmaf(vb[(int64_t)v[1] * 3 + c], w[1], vb[(int64_t)v[0] * 3 + c] * w[0]));
}

// cam = (raw - root) + trans of keypoint k: what the projection is taken of
__device__ __forceinline__ void kpt_cam_row(const KptArgs& a, int b, int k, int bin, const float* root, float* cam) {
    float raw[3];
    kpt_raw_row(a, b, k, bin, raw);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        cam[c] = raw[c] - root[c];
        if (a.trans) cam[c] = cam[c] + a.trans[b * 3 + c];
    }
}

__global__ __launch_bounds__(KPT_BLOCK) void kpt_fwd(KptArgs a) {
    const int b = blockIdx.x, K = a.t.K;
    __shared__ float root_lds[3];
    const int bin = a.t.Ld > 0 ? kpt_yaw_bin(a, b) : 0;
    if (threadIdx.x == 0) {
        float r[3];
        kpt_raw_row(a, b, K, bin, r);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            root_lds[c] = r[c];
            a.root_cam[b * 3 + c] = r[c];
        }
        a.yaw_bin[b] = bin;
    }
    __syncthreads();
    const float root[3] = {root_lds[0], root_lds[1], root_lds[2]};
    for (int k = threadIdx.x; k < K; k += KPT_BLOCK) {
        const int64_t o = (int64_t)b * K + k;
        float cam[3];
        kpt_cam_row(a, b, k, bin, root, cam);
        if (a.kpt_proj) {
            a.kpt_proj[o * 2 + 0] = ((cam[0] / cam[2]) * a.focal[b * 2 + 0]) + a.princpt[b * 2 + 0];
            a.kpt_proj[o * 2 + 1] = ((cam[1] / cam[2]) * a.focal[b * 2 + 1]) + a.princpt[b * 2 + 1];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (a.root_rel && a.trans) cam[c] = cam[c] - a.trans[b * 3 + c];
            a.kpt_cam[o * 3 + c] = cam[c];
        }
    }
}

__global__ __launch_bounds__(KPT_BLOCK) void kpt_mesh(KptArgs a) {
    const int64_t i = (int64_t)blockIdx.x * KPT_BLOCK + threadIdx.x;
    if (i >= (int64_t)a.B * a.t.V) return;
    const int b = (int)(i / a.t.V);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float m = a.vertices[i * 3 + c] - a.root_cam[b * 3 + c];
        if (a.trans) {
            m = m + a.trans[b * 3 + c];
            if (a.root_rel) m = m - a.trans[b * 3 + c];
        }
        a.mesh_cam[i * 3 + c] = m;
    }
}

__global__ __launch_bounds__(KPT_BLOCK) void kpt_bwd_sums(KptArgs a) {
    const int b = blockIdx.y, v = blockIdx.x * KPT_BLOCK + threadIdx.x;
    float s[3] = {0.0f, 0.0f, 0.0f};
    if (v < a.t.V) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = a.g_mesh[((int64_t)b * a.t.V + v) * 3 + c];
    }
    exa::block_sums<KPT_BLOCK / 64>(s);       // the header's WG(values)
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.partials[((int64_t)b * 3 + c) * a.blocks + blockIdx.x] = s[c];
    }
}

__global__ __launch_bounds__(KPT_BLOCK) void kpt_bwd_rows(KptArgs a) {
    const int b = blockIdx.x, K = a.t.K;
    __shared__ float seq[6];                  // S_c, S_p
    const int bin = kpt_clamp_bin(a.bin_in[b]);
    float* rows = a.rows + (int64_t)b * (2 * K + 1) * 3;
    float Sm[3] = {0.0f, 0.0f, 0.0f};         // SUM2 of g_mesh: the second level
    if (a.g_mesh && a.t.V > 0) {
        exa::strided_sums<KPT_BLOCK, 3>(Sm, a.partials + (int64_t)b * 3 * a.blocks, a.blocks, a.blocks);
        exa::block_sums<KPT_BLOCK / 64>(Sm);  // the header's WG(s)
    }
    float root[3];
    kpt_raw_row(a, b, K, bin, root);
    for (int k = threadIdx.x; k < K; k += KPT_BLOCK) {
        const int64_t o = (int64_t)b * K + k;
        float p[3] = {0.0f, 0.0f, 0.0f}, ck[3];
        if (a.g_proj) {
            float cam[3];
            kpt_cam_row(a, b, k, bin, root, cam);
            const float tx = a.g_proj[o * 2 + 0] * a.focal[b * 2 + 0], ty = a.g_proj[o * 2 + 1] * a.focal[b * 2 + 1];
            const float qx = cam[0] / cam[2], qy = cam[1] / cam[2];
            p[0] = tx / cam[2];
            p[1] = ty / cam[2];
            p[2] = -((tx * qx + ty * qy) / cam[2]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            ck[c] = a.g_cam ? (a.g_proj ? a.g_cam[o * 3 + c] + p[c] : a.g_cam[o * 3 + c]) : p[c];
            rows[k * 3 + c] = ck[c];
            rows[(K + 1 + k) * 3 + c] = p[c];
        }
    }
    __syncthreads();                          // the rows of this workgroup are visible to it
    if (threadIdx.x < 6) {
        const int c = threadIdx.x % 3;
        const float* src = rows + (threadIdx.x < 3 ? 0 : (K + 1) * 3);
        float s = 0.0f;
        for (int k = 0; k < K; ++k) s = s + src[k * 3 + c];
        seq[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        const float g = a.g_root ? a.g_root[b * 3 + c] : 0.0f;
        rows[K * 3 + c] = (g - seq[c]) - Sm[c];
        if (a.d_trans) a.d_trans[b * 3 + c] = a.root_rel ? seq[3 + c] : seq[c] + Sm[c];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < a.t.J; j += KPT_BLOCK) {
        float acc[3] = {0.0f, 0.0f, 0.0f};
        for (int q = a.t.joff[j], end = a.t.joff[j + 1]; q < end; ++q) {
            const int k = a.t.jent[q];
            if ((unsigned)k > (unsigned)K) {                   // the guard: nothing outside the rows is read
                acc[0] = acc[1] = acc[2] = kpt_qnan();
                continue;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = acc[c] + rows[k * 3 + c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) a.d_joints[((int64_t)b * a.t.J + j) * 3 + c] = acc[c];
    }
}

__global__ __launch_bounds__(KPT_BLOCK) void kpt_bwd_vertices(KptArgs a) {
    const int64_t i = (int64_t)blockIdx.x * KPT_BLOCK + threadIdx.x;
    if (i >= (int64_t)a.B * a.t.V) return;
    const int b = (int)(i / a.t.V), v = (int)(i % a.t.V), K = a.t.K;
    const int bin = kpt_clamp_bin(a.bin_in[b]);
    const float* rows = a.rows + (int64_t)b * (2 * K + 1) * 3;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    if (a.g_mesh) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = a.g_mesh[i * 3 + c];
    }
    const int t = a.t.vrow[v];
    if (t >= 0) {
        if (t >= a.t.T) {
            acc[0] = acc[1] = acc[2] = kpt_qnan();
        } else {
            for (int q = a.t.voff[t], end = a.t.voff[t + 1]; q < end; ++q) {
                const int eb = a.t.vent_bin[q];
                if (eb != -1 && eb != bin) continue;
                const int k = a.t.vent_k[q];
                if ((unsigned)k > (unsigned)K) {               // the guard
                    acc[0] = acc[1] = acc[2] = kpt_qnan();
                    continue;
                }
                const float w = a.t.vent_w[q];
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] = acc[c] + w * rows[k * 3 + c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) a.d_vertices[i * 3 + c] = acc[c];
}

// ---- CoordLoss ----------------------------------------------------------------------------------------------------------
struct CoordArgs {
    int32_t B, K, nl, nr;
    const int32_t* lhand; const int32_t* rhand; const int32_t* part;
    const float* proj; const float* gt; const float* valid; const float* cam; const float* weight; const float* grad;
    float* hand_w; float* loss; float* d_proj;
};

struct HandBox { float sum, depth, x, y, w, h; int count; };

// torch.maximum / torch.minimum: NaN when either operand is
__device__ __forceinline__ float coord_max(float p, float q) { return (p != p || q != q) ? kpt_qnan() : (p > q ? p : q); }
__device__ __forceinline__ float coord_min(float p, float q) { return (p != p || q != q) ? kpt_qnan() : (p < q ? p : q); }

__device__ __forceinline__ void coord_extend(float lo_in, float hi_in, float* lo, float* w) {
    const float centre = (lo_in + hi_in) / 2.0f, width = hi_in - lo_in;
    const float half = (0.5f * width) * 1.2f;
    const float l = centre - half, h = centre + half;
    *lo = l;
    *w = h - l;
}

__device__ __forceinline__ HandBox coord_hand(const CoordArgs& a, int b, const int32_t* idx, int n) {
    HandBox h;
    h.sum = 0.0f; h.count = 0;
    float z = 0.0f, xmin = 0.0f, xmax = 0.0f, ymin = 0.0f, ymax = 0.0f;
    for (int i = 0; i < n; ++i) {
        const int k = idx[i];
        if ((unsigned)k >= (unsigned)a.K) continue;            // the guard: nothing outside the item's rows is read
        const int64_t o = (int64_t)b * a.K + k;
        const float v = a.valid[o];
        h.sum = h.sum + v;
        z = z + a.cam[o * 3 + 2];
        if (v > 0.0f) {
            const float x = a.proj[o * 2 + 0], y = a.proj[o * 2 + 1];
            if (h.count == 0) {
                xmin = xmax = x; ymin = ymax = y;
            } else {
                xmin = coord_min(xmin, x); xmax = coord_max(xmax, x);
                ymin = coord_min(ymin, y); ymax = coord_max(ymax, y);
            }
            ++h.count;
        }
    }
    h.depth = z / (float)n;
    coord_extend(xmin, xmax, &h.x, &h.w);
    coord_extend(ymin, ymax, &h.y, &h.h);
    return h;
}

__global__ __launch_bounds__(64) void coord_fwd(CoordArgs a) {
    const int b = blockIdx.x;
    const HandBox L = coord_hand(a, b, a.lhand, a.nl), R = coord_hand(a, b, a.rhand, a.nr);
    int lose = 0;                             // bit 1: the left hand and its wrist, bit 2: the right
    if (!(L.sum == 0.0f) && !(R.sum == 0.0f) && L.count > 0 && R.count > 0) {
        const float lx2 = L.w + L.x, ly2 = L.h + L.y, rx2 = R.w + R.x, ry2 = R.h + R.y;      // xywh -> xyxy
        const float xmin = coord_max(L.x, R.x), ymin = coord_max(L.y, R.y);
        const float xmax = coord_min(lx2, rx2), ymax = coord_min(ly2, ry2);
        const float inter = coord_max(0.0f, xmax - xmin) * coord_max(0.0f, ymax - ymin);
        const float area_l = (lx2 - L.x) * (ly2 - L.y), area_r = (rx2 - R.x) * (ry2 - R.y);
        const float uni = (area_l + area_r) - inter;
        const float iou = inter / (uni + 1e-5f);
        if (iou > 0.5f) lose = L.depth > R.depth ? 1 : 2;
    }
    for (int k = threadIdx.x; k < a.K; k += 64) {
        const int64_t o = (int64_t)b * a.K + k;
        const float hw = (a.part[k] & lose) ? 0.0f : 1.0f, v = a.valid[o];
        a.hand_w[o] = hw;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float l = (fabsf(a.proj[o * 2 + c] - a.gt[o * 2 + c]) * v) * hw;
            if (a.weight) l = l * a.weight[o * 2 + c];
            a.loss[o * 2 + c] = l;
        }
    }
}

__global__ __launch_bounds__(KPT_BLOCK) void coord_bwd(CoordArgs a) {
    const int64_t i = (int64_t)blockIdx.x * KPT_BLOCK + threadIdx.x;
    if (i >= (int64_t)a.B * a.K * 2) return;
    const float d = a.proj[i] - a.gt[i];
    const float sign = (d > 0.0f ? 1.0f : 0.0f) - (d < 0.0f ? 1.0f : 0.0f);
    float g = a.grad[i];
    if (a.weight) g = g * a.weight[i];
    a.d_proj[i] = ((g * a.hand_w[i / 2]) * a.valid[i / 2]) * sign;
}

int check_kpt(const ExaMeshKeypoints* t, int32_t B) {
    if (!t) return fail(EXA_MESH_E_NULLPTR, "tables is NULL");
    if (B < 0 || t->V < 0 || t->J < 0 || t->K < 0 || t->Ld < 0 || t->C < 0 || t->T < 0) return fail(EXA_MESH_E_INVALID, "negative size");
    if (B > KPT_MAX_BATCH) return fail(EXA_MESH_E_INVALID, "B exceeds 65535");
    if ((int64_t)B * t->V * 3 > KPT_MAX_ELEMS) return fail(EXA_MESH_E_INVALID, "B * V * 3 exceeds 2^30");
    if ((int64_t)B * t->J * 9 > KPT_MAX_ELEMS) return fail(EXA_MESH_E_INVALID, "B * J * 9 exceeds 2^30");
    if ((int64_t)B * (2 * (int64_t)t->K + 1) * 3 > KPT_MAX_ELEMS) return fail(EXA_MESH_E_INVALID, "B * (2 K + 1) * 3 exceeds 2^30");
    if (t->T > t->V) return fail(EXA_MESH_E_INVALID, "T exceeds V");
    if (!t->rec || !t->rec_w) return fail(EXA_MESH_E_NULLPTR, "rec / rec_w is NULL");
    if (t->Ld > 0 && (!t->dyn_vtx || !t->dyn_w)) return fail(EXA_MESH_E_NULLPTR, "dyn_vtx / dyn_w is NULL with Ld > 0");
    if (t->C > 0 && !t->chain) return fail(EXA_MESH_E_NULLPTR, "chain is NULL with C > 0");
    return 0;
}

int check_coord(int32_t B, int32_t K) {
    if (B < 0 || K < 0) return fail(EXA_MESH_E_INVALID, "negative size");
    if ((int64_t)B * K * 3 > KPT_MAX_ELEMS) return fail(EXA_MESH_E_INVALID, "B * K * 3 exceeds 2^30");
    return 0;
}

}  // namespace

}  // namespace exa_mesh_impl

using namespace exa_mesh_impl;

extern "C" {

int64_t exa_mesh_keypoints_blocks(int32_t V) { return V <= 0 ? 0 : ((int64_t)V + KPT_BLOCK - 1) / KPT_BLOCK; }

int exa_mesh_keypoints_workspace_size(int32_t B, int32_t V, int32_t K, uint64_t* out_bytes) {
    if (!out_bytes) return fail(EXA_MESH_E_NULLPTR, "out_bytes is NULL");
    if (B < 0 || V < 0 || K < 0) return fail(EXA_MESH_E_INVALID, "negative size");
    const uint64_t rows = (uint64_t)B * (2 * (uint64_t)K + 1) * 3, partials = (uint64_t)B * 3 * (uint64_t)exa_mesh_keypoints_blocks(V);
    *out_bytes = exa::align256(rows * 4) + exa::align256(partials * 4);
    return 0;
}

int exa_mesh_keypoints_forward(const ExaMeshKeypoints* tables, int32_t B, const float* vertices, const float* joints,
                               const float* rot, const float* trans, const float* focal, const float* princpt,
                               int32_t root_rel, float* kpt_cam, float* root_cam, float* kpt_proj, float* mesh_cam,
                               int32_t* yaw_bin, void* stream) {
    if (int rc = check_kpt(tables, B)) return rc;
    if (B == 0) return 0;
    if (tables->Ld > 0 && !rot) return fail(EXA_MESH_E_NULLPTR, "rot is NULL with Ld > 0");
    if ((tables->V > 0 && !vertices) || (tables->J > 0 && !joints)) return fail(EXA_MESH_E_NULLPTR, "vertices / joints is NULL");
    if (!root_cam || !yaw_bin || (tables->K > 0 && !kpt_cam)) return fail(EXA_MESH_E_NULLPTR, "kpt_cam / root_cam / yaw_bin is NULL");
    if (kpt_proj && (!focal || !princpt)) return fail(EXA_MESH_E_NULLPTR, "focal / princpt is NULL with kpt_proj");
    KptArgs a = {};
    a.t = *tables; a.B = B; a.root_rel = root_rel != 0;
    a.vertices = vertices; a.joints = joints; a.rot = rot; a.trans = trans; a.focal = focal; a.princpt = princpt;
    a.kpt_cam = kpt_cam; a.root_cam = root_cam; a.kpt_proj = kpt_proj; a.mesh_cam = mesh_cam; a.yaw_bin = yaw_bin;
    hipLaunchKernelGGL(kpt_fwd, dim3((unsigned)B), dim3(KPT_BLOCK), 0, (hipStream_t)stream, a);
    if (int rc = launched("kpt_fwd")) return rc;
    if (!mesh_cam || tables->V == 0) return 0;
    hipLaunchKernelGGL(kpt_mesh, dim3(ceil_div((int64_t)B * tables->V, KPT_BLOCK)), dim3(KPT_BLOCK), 0, (hipStream_t)stream, a);
    return launched("kpt_mesh");
}

int exa_mesh_keypoints_backward(const ExaMeshKeypoints* tables, int32_t B, const float* vertices, const float* joints,
                                const float* trans, const float* focal, const float* princpt, int32_t root_rel,
                                const int32_t* yaw_bin, const float* g_kpt_cam, const float* g_kpt_proj,
                                const float* g_root_cam, const float* g_mesh_cam, void* workspace, uint64_t workspace_bytes,
                                float* d_vertices, float* d_joints, float* d_trans, void* stream) {
    if (int rc = check_kpt(tables, B)) return rc;
    if (B == 0) return 0;
    if ((tables->V > 0 && !vertices) || (tables->J > 0 && !joints)) return fail(EXA_MESH_E_NULLPTR, "vertices / joints is NULL");
    if (!yaw_bin) return fail(EXA_MESH_E_NULLPTR, "yaw_bin is NULL");
    if (g_kpt_proj && (!focal || !princpt)) return fail(EXA_MESH_E_NULLPTR, "focal / princpt is NULL with g_kpt_proj");
    if ((tables->V > 0 && !d_vertices) || (tables->J > 0 && !d_joints)) return fail(EXA_MESH_E_NULLPTR, "d_vertices / d_joints is NULL");
    if (tables->J > 0 && (!tables->joff || !tables->jent)) return fail(EXA_MESH_E_NULLPTR, "joff / jent is NULL");
    if (tables->V > 0 && (!tables->vrow || !tables->voff || !tables->vent_k || !tables->vent_bin || !tables->vent_w))
        return fail(EXA_MESH_E_NULLPTR, "vrow / voff / vent_k / vent_bin / vent_w is NULL");
    uint64_t need = 0;
    if (int rc = exa_mesh_keypoints_workspace_size(B, tables->V, tables->K, &need)) return rc;
    if (!workspace) return fail(EXA_MESH_E_NULLPTR, "workspace is NULL");
    if (workspace_bytes < need) return fail(EXA_MESH_E_INVALID, "workspace is too small");
    KptArgs a = {};
    a.t = *tables; a.B = B; a.root_rel = root_rel != 0; a.blocks = (int32_t)exa_mesh_keypoints_blocks(tables->V);
    a.vertices = vertices; a.joints = joints; a.trans = trans; a.focal = focal; a.princpt = princpt; a.bin_in = yaw_bin;
    a.g_cam = g_kpt_cam; a.g_proj = g_kpt_proj; a.g_root = g_root_cam; a.g_mesh = g_mesh_cam;
    a.rows = (float*)workspace;
    a.partials = (float*)((char*)workspace + exa::align256((uint64_t)B * (2 * (uint64_t)tables->K + 1) * 3 * 4));
    a.d_vertices = d_vertices; a.d_joints = d_joints; a.d_trans = trans ? d_trans : nullptr;
    if (g_mesh_cam && tables->V > 0) {
        hipLaunchKernelGGL(kpt_bwd_sums, dim3((unsigned)a.blocks, (unsigned)B), dim3(KPT_BLOCK), 0, (hipStream_t)stream, a);
        if (int rc = launched("kpt_bwd_sums")) return rc;
    }
    hipLaunchKernelGGL(kpt_bwd_rows, dim3((unsigned)B), dim3(KPT_BLOCK), 0, (hipStream_t)stream, a);
    if (int rc = launched("kpt_bwd_rows")) return rc;
    if (tables->V == 0) return 0;
    hipLaunchKernelGGL(kpt_bwd_vertices, dim3(ceil_div((int64_t)B * tables->V, KPT_BLOCK)), dim3(KPT_BLOCK), 0, (hipStream_t)stream, a);
    return launched("kpt_bwd_vertices");
}

int exa_mesh_coord_loss_forward(int32_t B, int32_t K, int32_t n_lhand, int32_t n_rhand, const int32_t* lhand_idx,
                                const int32_t* rhand_idx, const int32_t* part, const float* kpt_proj,
                                const float* kpt_proj_gt, const float* kpt_valid, const float* kpt_cam, const float* weight,
                                float* hand_w, float* loss, void* stream) {
    if (int rc = check_coord(B, K)) return rc;
    if (n_lhand < 1 || n_rhand < 1) return fail(EXA_MESH_E_INVALID, "a hand needs at least one keypoint");
    if (B == 0 || K == 0) return 0;
    if (!lhand_idx || !rhand_idx || !part) return fail(EXA_MESH_E_NULLPTR, "lhand_idx / rhand_idx / part is NULL");
    if (!kpt_proj || !kpt_proj_gt || !kpt_valid || !kpt_cam) return fail(EXA_MESH_E_NULLPTR, "kpt_proj / kpt_proj_gt / kpt_valid / kpt_cam is NULL");
    if (!hand_w || !loss) return fail(EXA_MESH_E_NULLPTR, "hand_w / loss is NULL");
    CoordArgs a = {};
    a.B = B; a.K = K; a.nl = n_lhand; a.nr = n_rhand; a.lhand = lhand_idx; a.rhand = rhand_idx; a.part = part;
    a.proj = kpt_proj; a.gt = kpt_proj_gt; a.valid = kpt_valid; a.cam = kpt_cam; a.weight = weight;
    a.hand_w = hand_w; a.loss = loss;
    hipLaunchKernelGGL(coord_fwd, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, a);
    return launched("coord_fwd");
}

int exa_mesh_coord_loss_backward(int32_t B, int32_t K, const float* kpt_proj, const float* kpt_proj_gt,
                                 const float* kpt_valid, const float* weight, const float* hand_w, const float* grad_loss,
                                 float* dL_dkpt_proj, void* stream) {
    if (int rc = check_coord(B, K)) return rc;
    if (B == 0 || K == 0) return 0;
    if (!kpt_proj || !kpt_proj_gt || !kpt_valid || !hand_w || !grad_loss || !dL_dkpt_proj)
        return fail(EXA_MESH_E_NULLPTR, "kpt_proj / kpt_proj_gt / kpt_valid / hand_w / grad_loss / dL_dkpt_proj is NULL");
    CoordArgs a = {};
    a.B = B; a.K = K; a.proj = kpt_proj; a.gt = kpt_proj_gt; a.valid = kpt_valid; a.weight = weight; a.hand_w = (float*)hand_w;
    a.grad = grad_loss; a.d_proj = dL_dkpt_proj;
    hipLaunchKernelGGL(coord_bwd, dim3(ceil_div((int64_t)B * K * 2, KPT_BLOCK)), dim3(KPT_BLOCK), 0, (hipStream_t)stream, a);
    return launched("coord_bwd");
}

}  // extern "C"
