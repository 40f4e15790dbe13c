// Gaussian offset and joint offset regularisers (include/exa_mesh.h; the reference's gaussian_mean_reg,
// gaussian_scale_reg, joint_offset_reg and JointOffsetSymmetricReg, model.py:217-232, 253-257, loss.py:133-146).  The
// semantics -- every operation in fp32 in a stated order -- are written out in the header; this file implements them.
//
//   offset_vertex_fwd   one thread per row (b, v) of the B V rows, OFF_BLOCK = 256 rows per workgroup: the three
//                       elements of the row for both vertex terms.  Map mode writes them; mean mode adds the row up,
//                       (t0 + t1) + t2, and the workgroup writes one partial per term (block_sums, the house sum).
//   offset_joint_fwd    ONE workgroup.  Thread j takes joint elements j, j + 256, .. and pairs j, j + 256, ..; map mode
//                       writes them, mean mode also adds the vertex partials j, j + 256, .. and writes the four means.
//   offset_bwd          workgroups 0 .. blocks - 1: one thread per row, every requested vertex gradient; the last
//                       workgroup (only when dL_djoint_offset is requested): thread j takes joints j, j + 256, .. and
//                       finds a joint's pair through the inverse table, so nothing is scattered.
// The rows are read with 4-byte loads: a wave's 64 rows are 768 consecutive bytes of every array, and the arrays may start
// at any 4-byte boundary.  No atomics, no memsets, no allocation, no synchronisation: every output element is one thread's
// value in the header's order.  Compiled with -ffp-contract=off (build.py): no product is contracted into a fused
// multiply-add.
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

constexpr int OFF_BLOCK = EXA_MESH_OFFSET_ROWS;
constexpr int64_t OFF_MAX_ELEMS = 1 << 30;    // B * V * 3
constexpr int32_t OFF_MAX_JOINTS = 1 << 20;

__device__ __forceinline__ float off_qnan() { return __int_as_float(0x7fc00000); }

__device__ __forceinline__ float off_sign(float x) { return (x > 0.0f ? 1.0f : 0.0f) - (x < 0.0f ? 1.0f : 0.0f); }

struct OffsetArgs {
    int32_t V, C, J, n_pairs;                 // C: channels of scale_offset, 1 or 3
    int64_t rows;                             // B * V
    int64_t blocks;                           // vertex workgroups = partials per term
    const float* mo; const float* moo; const float* sc; const float* so;
    const float* w_mean; const float* w_scale;
    const float* jo; const float* jref; const float* w_joint;
    const int32_t* pair_r; const int32_t* pair_l; const int32_t* joint_pair;
    // forward
    float* mean_map; float* scale_map; float* joint_map; float* sym_map;
    float* partials;                          // vertex launch: written; joint launch: read
    float* means;
    float n[4];                               // (float)N_k
    // backward: per term a cotangent of the map or of the mean (or neither)
    const float* g_map[4]; const float* g_mean[4];
    float* d_mo; float* d_moo; float* d_sc; float* d_so; float* d_jo;
};

__global__ __launch_bounds__(OFF_BLOCK) void offset_vertex_fwd(OffsetArgs a) {
    const int64_t i = (int64_t)blockIdx.x * OFF_BLOCK + threadIdx.x;
    float s[2] = {0.0f, 0.0f};
    if (i < a.rows) {
        const int v = (int)(i % a.V);
        const float wm = a.w_mean[v], ws = a.w_scale[v];
        float tm[3], ts[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float x = a.mo[i * 3 + c], y = a.moo[i * 3 + c], z = a.sc[i * 3 + c];
            const float u = a.C == 1 ? a.so[i] : a.so[i * 3 + c];
            tm[c] = ((x * x) + (y * y)) * wm;
            ts[c] = ((z * z) + (u * u)) * ws;
        }
        if (a.mean_map) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                a.mean_map[i * 3 + c] = tm[c];
                a.scale_map[i * 3 + c] = ts[c];
            }
        }
        s[0] = (tm[0] + tm[1]) + tm[2];
        s[1] = (ts[0] + ts[1]) + ts[2];
    }
    if (a.partials) {                                          // (uniform: every thread of the workgroup gets here)
        exa::block_sums<OFF_BLOCK / 64>(s);      // the header's WG(s)
        if (threadIdx.x == 0) {
            a.partials[blockIdx.x] = s[0];
            a.partials[a.blocks + blockIdx.x] = s[1];
        }
    }
}

// the sym term of pair p; an index outside [0, J) reads nothing and gives NaN
__device__ __forceinline__ float sym_of(const OffsetArgs& a, int p) {
    const int r = a.pair_r[p], l = a.pair_l[p];
    if ((unsigned)r >= (unsigned)a.J || (unsigned)l >= (unsigned)a.J) return off_qnan();
    const float* R = a.jo + (int64_t)r * 3;
    const float* L = a.jo + (int64_t)l * 3;
    return (fabsf(R[0] + L[0]) + fabsf(R[1] - L[1])) + fabsf(R[2] - L[2]);
}

__global__ __launch_bounds__(OFF_BLOCK) void offset_joint_fwd(OffsetArgs a) {
    const int tid = threadIdx.x;
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (a.means) exa::strided_sums<OFF_BLOCK, 2>(s, a.partials, a.blocks, a.blocks);
    for (int e = tid; e < a.J * 3; e += OFF_BLOCK) {
        const float d = a.jo[e] - a.jref[e];
        const float t = (d * d) * a.w_joint[e];
        if (a.joint_map) a.joint_map[e] = t;
        s[2] = s[2] + t;
    }
    for (int p = tid; p < a.n_pairs; p += OFF_BLOCK) {
        const float t = sym_of(a, p);
        if (a.sym_map) a.sym_map[p] = t;
        s[3] = s[3] + t;
    }
    if (a.means) {                                             // (uniform)
        exa::block_sums<OFF_BLOCK / 64>(s);      // the header's WG(s)
        if (tid < 4) a.means[tid] = s[tid] / a.n[tid];         // N_k == 0: 0 / 0 = NaN, torch.mean of an empty tensor
    }
}

// the cotangent of element e of term k: the map's, or g_k * (1 / N_k) with the reciprocal rounded first
__device__ __forceinline__ bool has_g(const OffsetArgs& a, int k) { return a.g_map[k] || a.g_mean[k]; }

__device__ __forceinline__ float mean_g(const OffsetArgs& a, int k) {
    return a.g_mean[k] ? *a.g_mean[k] * (1.0f / a.n[k]) : 0.0f;
}

__device__ __forceinline__ void offset_bwd_rows(const OffsetArgs& a) {
    const int64_t i = (int64_t)blockIdx.x * OFF_BLOCK + threadIdx.x;
    if (i >= a.rows) return;
    const int v = (int)(i % a.V);
    if (a.d_mo || a.d_moo) {
        const bool on = has_g(a, 0);
        const float w = on ? a.w_mean[v] : 0.0f, km = mean_g(a, 0);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float gw = on ? (a.g_map[0] ? a.g_map[0][i * 3 + c] : km) * w : 0.0f;
            if (a.d_mo) a.d_mo[i * 3 + c] = on ? gw * (2.0f * a.mo[i * 3 + c]) : 0.0f;
            if (a.d_moo) a.d_moo[i * 3 + c] = on ? gw * (2.0f * a.moo[i * 3 + c]) : 0.0f;
        }
    }
    if (a.d_sc || a.d_so) {
        const bool on = has_g(a, 1);
        const float w = on ? a.w_scale[v] : 0.0f, km = mean_g(a, 1);
        float gw[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            gw[c] = on ? (a.g_map[1] ? a.g_map[1][i * 3 + c] : km) * w : 0.0f;
            if (a.d_sc) a.d_sc[i * 3 + c] = on ? gw[c] * (2.0f * a.sc[i * 3 + c]) : 0.0f;
        }
        if (a.d_so) {
            if (a.C == 1) {                                    // the broadcast is summed first, then the power rule
                const float r = (gw[0] + gw[1]) + gw[2];
                a.d_so[i] = on ? r * (2.0f * a.so[i]) : 0.0f;
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) a.d_so[i * 3 + c] = on ? gw[c] * (2.0f * a.so[i * 3 + c]) : 0.0f;
            }
        }
    }
}

__device__ __forceinline__ void offset_bwd_joints(const OffsetArgs& a) {
    const bool on_reg = has_g(a, 2), on_sym = has_g(a, 3);
    const float k_reg = mean_g(a, 2), k_sym = mean_g(a, 3);
    for (int j = threadIdx.x; j < a.J; j += OFF_BLOCK) {
        float sym[3] = {0.0f, 0.0f, 0.0f};
        bool paired = false;
        const int code = on_sym && a.n_pairs > 0 ? a.joint_pair[j] : -1;
        if (code >= 0) {
            const int p = code >> 1, left = code & 1;
            paired = true;
            int r = -1, l = -1;
            if (p < a.n_pairs) {
                r = a.pair_r[p];
                l = a.pair_l[p];
            }
            if ((unsigned)r >= (unsigned)a.J || (unsigned)l >= (unsigned)a.J) {      // the guard, as in the forward
                sym[0] = sym[1] = sym[2] = off_qnan();
            } else {
                const float g = a.g_map[3] ? a.g_map[3][p] : k_sym;
                const float* R = a.jo + (int64_t)r * 3;
                const float* L = a.jo + (int64_t)l * 3;
                sym[0] = off_sign(R[0] + L[0]) * g;
#pragma unroll
                for (int c = 1; c < 3; ++c) {
                    const float t = off_sign(R[c] - L[c]) * g;
                    sym[c] = left ? -t : t;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int e = j * 3 + c;
            float reg = 0.0f;
            if (on_reg) reg = ((a.g_map[2] ? a.g_map[2][e] : k_reg) * a.w_joint[e]) * (2.0f * (a.jo[e] - a.jref[e]));
            a.d_jo[e] = on_reg && paired ? reg + sym[c] : on_reg ? reg : paired ? sym[c] : 0.0f;
        }
    }
}

__global__ __launch_bounds__(OFF_BLOCK) void offset_bwd(OffsetArgs a, int vertex_blocks) {
    if ((int)blockIdx.x < vertex_blocks) offset_bwd_rows(a);
    else offset_bwd_joints(a);
}

int64_t offset_blocks(int32_t B, int32_t V) {
    if (B <= 0 || V <= 0) return 0;
    return ((int64_t)B * V + OFF_BLOCK - 1) / OFF_BLOCK;
}

int check_vertex_shape(int32_t B, int32_t V, int32_t C) {
    if (B < 0 || V < 0) return fail(EXA_MESH_E_INVALID, "negative size");
    if ((int64_t)B * V * 3 > OFF_MAX_ELEMS) return fail(EXA_MESH_E_INVALID, "B * V * 3 exceeds 2^30");
    if (C != 1 && C != 3) return fail(EXA_MESH_E_INVALID, "scale_offset must have 1 or 3 channels");
    return 0;
}

int check_joint_shape(int32_t J, int32_t n_pairs) {
    if (J < 0 || n_pairs < 0) return fail(EXA_MESH_E_INVALID, "negative size");
    if (J > OFF_MAX_JOINTS) return fail(EXA_MESH_E_INVALID, "J exceeds 2^20");
    if (n_pairs > J / 2) return fail(EXA_MESH_E_INVALID, "n_pairs exceeds J / 2 (a joint belongs to at most one pair)");
    return 0;
}

void set_counts(OffsetArgs& a, int32_t B, int32_t V, int32_t J, int32_t n_pairs) {
    a.n[0] = a.n[1] = (float)((int64_t)B * V * 3);
    a.n[2] = (float)((int64_t)J * 3);
    a.n[3] = (float)n_pairs;
}

}  // namespace

}  // namespace exa_mesh_impl

using namespace exa_mesh_impl;

extern "C" {

int64_t exa_mesh_offset_regs_blocks(int32_t B, int32_t V) {
    if ((int64_t)B * V * 3 > OFF_MAX_ELEMS) return 0;
    return offset_blocks(B, V);
}

int exa_mesh_offset_regs_pair_table(int32_t J, int32_t n_pairs, const int32_t* pair_r, const int32_t* pair_l,
                                    int32_t* joint_pair) {
    if (J < 0 || n_pairs < 0) return fail(EXA_MESH_E_INVALID, "negative size");
    if (J > OFF_MAX_JOINTS) return fail(EXA_MESH_E_INVALID, "J exceeds 2^20");
    if (J > 0 && !joint_pair) return fail(EXA_MESH_E_NULLPTR, "joint_pair is NULL");
    if (n_pairs > 0 && (!pair_r || !pair_l)) return fail(EXA_MESH_E_NULLPTR, "pair_r / pair_l is NULL");
    for (int32_t j = 0; j < J; ++j) joint_pair[j] = -1;
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int32_t side[2] = {pair_r[p], pair_l[p]};
        for (int s = 0; s < 2; ++s) {
            if (side[s] < 0 || side[s] >= J) return fail(EXA_MESH_E_INVALID, "a pair index is outside [0, J)");
            if (joint_pair[side[s]] != -1) return fail(EXA_MESH_E_INVALID, "a joint belongs to more than one pair");
            joint_pair[side[s]] = 2 * p + s;
        }
    }
    return 0;
}

int exa_mesh_offset_regs_vertex_forward(int32_t B, int32_t V, int32_t scale_offset_channels, const float* mean_offset,
                                        const float* mean_offset_offset, const float* scale, const float* scale_offset,
                                        const float* w_mean, const float* w_scale, float* mean_map, float* scale_map,
                                        float* partials, void* stream) {
    if (int rc = check_vertex_shape(B, V, scale_offset_channels)) return rc;
    if ((mean_map != nullptr) != (scale_map != nullptr))
        return fail(EXA_MESH_E_INVALID, "offset_regs forward: pass both maps or neither");
    if ((mean_map != nullptr) == (partials != nullptr))
        return fail(EXA_MESH_E_INVALID, "offset_regs forward: pass exactly one of the maps / partials");
    const int64_t blocks = offset_blocks(B, V);
    if (blocks == 0) return 0;
    if (!mean_offset || !mean_offset_offset || !scale || !scale_offset || !w_mean || !w_scale)
        return fail(EXA_MESH_E_NULLPTR, "mean_offset / mean_offset_offset / scale / scale_offset / w_mean / w_scale is NULL");
    OffsetArgs a = {};
    a.V = V; a.C = scale_offset_channels; a.rows = (int64_t)B * V; a.blocks = blocks;
    a.mo = mean_offset; a.moo = mean_offset_offset; a.sc = scale; a.so = scale_offset;
    a.w_mean = w_mean; a.w_scale = w_scale;
    a.mean_map = mean_map; a.scale_map = scale_map; a.partials = partials;
    hipLaunchKernelGGL(offset_vertex_fwd, dim3((unsigned)blocks), dim3(OFF_BLOCK), 0, (hipStream_t)stream, a);
    return launched("offset_vertex_fwd");
}

int exa_mesh_offset_regs_joint_forward(int32_t B, int32_t V, int32_t J, int32_t n_pairs, const float* joint_offset,
                                       const float* joint_ref, const float* w_joint, const int32_t* pair_r,
                                       const int32_t* pair_l, float* joint_map, float* sym_map, const float* partials,
                                       float* means, void* stream) {
    if (int rc = check_vertex_shape(B, V, 1)) return rc;
    if (int rc = check_joint_shape(J, n_pairs)) return rc;
    const bool maps = joint_map || sym_map;
    if (maps == (means != nullptr))
        return fail(EXA_MESH_E_INVALID, "offset_regs forward: pass exactly one of the maps / means");
    const int64_t blocks = offset_blocks(B, V);
    if (means && blocks > 0 && !partials) return fail(EXA_MESH_E_NULLPTR, "partials is NULL");
    if (maps && ((J > 0 && !joint_map) || (n_pairs > 0 && !sym_map))) return fail(EXA_MESH_E_NULLPTR, "joint_map / sym_map is NULL");
    if (J > 0 && (!joint_offset || !joint_ref || !w_joint)) return fail(EXA_MESH_E_NULLPTR, "joint_offset / joint_ref / w_joint is NULL");
    if (n_pairs > 0 && (!pair_r || !pair_l)) return fail(EXA_MESH_E_NULLPTR, "pair_r / pair_l is NULL");
    if (!means && J == 0) return 0;                             // (n_pairs <= J / 2: no map element is left to write)
    OffsetArgs a = {};
    a.V = V; a.J = J; a.n_pairs = n_pairs; a.rows = (int64_t)B * V; a.blocks = blocks;
    a.jo = joint_offset; a.jref = joint_ref; a.w_joint = w_joint; a.pair_r = pair_r; a.pair_l = pair_l;
    a.joint_map = joint_map; a.sym_map = sym_map; a.partials = (float*)partials; a.means = means;
    set_counts(a, B, V, J, n_pairs);
    hipLaunchKernelGGL(offset_joint_fwd, dim3(1), dim3(OFF_BLOCK), 0, (hipStream_t)stream, a);
    return launched("offset_joint_fwd");
}

int exa_mesh_offset_regs_backward(int32_t B, int32_t V, int32_t scale_offset_channels, int32_t J, int32_t n_pairs,
                                  const float* mean_offset, const float* mean_offset_offset, const float* scale,
                                  const float* scale_offset, const float* w_mean, const float* w_scale,
                                  const float* joint_offset, const float* joint_ref, const float* w_joint,
                                  const int32_t* pair_r, const int32_t* pair_l, const int32_t* joint_pair,
                                  const float* const* dL_dmaps, const float* const* dL_dmeans, float* dL_dmean_offset,
                                  float* dL_dmean_offset_offset, float* dL_dscale, float* dL_dscale_offset,
                                  float* dL_djoint_offset, void* stream) {
    if (int rc = check_vertex_shape(B, V, scale_offset_channels)) return rc;
    if (int rc = check_joint_shape(J, n_pairs)) return rc;
    bool any_map = false, any_mean = false;
    for (int k = 0; k < 4; ++k) {
        any_map = any_map || (dL_dmaps && dL_dmaps[k]);
        any_mean = any_mean || (dL_dmeans && dL_dmeans[k]);
    }
    if (any_map == any_mean)
        return fail(EXA_MESH_E_INVALID, "offset_regs backward: pass cotangents of the maps or of the means, not both or neither");
    OffsetArgs a = {};
    for (int k = 0; k < 4; ++k) {
        a.g_map[k] = any_map ? dL_dmaps[k] : nullptr;
        a.g_mean[k] = any_mean ? dL_dmeans[k] : nullptr;
    }
    const bool rows_out = dL_dmean_offset || dL_dmean_offset_offset || dL_dscale || dL_dscale_offset;
    const int64_t vblocks = rows_out ? offset_blocks(B, V) : 0;
    const int jblocks = dL_djoint_offset && J > 0 ? 1 : 0;
    if (vblocks + jblocks == 0) return 0;
    if (vblocks > 0) {
        if (((dL_dmean_offset || dL_dmean_offset_offset) && (a.g_map[0] || a.g_mean[0]) &&
             (!mean_offset || !mean_offset_offset || !w_mean)) ||
            ((dL_dscale || dL_dscale_offset) && (a.g_map[1] || a.g_mean[1]) && (!scale || !scale_offset || !w_scale)))
            return fail(EXA_MESH_E_NULLPTR, "mean_offset / mean_offset_offset / scale / scale_offset / w_mean / w_scale is NULL");
    }
    if (jblocks) {
        if ((a.g_map[2] || a.g_mean[2]) && (!joint_offset || !joint_ref || !w_joint))
            return fail(EXA_MESH_E_NULLPTR, "joint_offset / joint_ref / w_joint is NULL");
        if ((a.g_map[3] || a.g_mean[3]) && n_pairs > 0 && (!joint_offset || !pair_r || !pair_l || !joint_pair))
            return fail(EXA_MESH_E_NULLPTR, "joint_offset / pair_r / pair_l / joint_pair is NULL");
    }
    a.V = V; a.C = scale_offset_channels; a.J = J; a.n_pairs = n_pairs; a.rows = (int64_t)B * V; a.blocks = vblocks;
    a.mo = mean_offset; a.moo = mean_offset_offset; a.sc = scale; a.so = scale_offset;
    a.w_mean = w_mean; a.w_scale = w_scale;
    a.jo = joint_offset; a.jref = joint_ref; a.w_joint = w_joint;
    a.pair_r = pair_r; a.pair_l = pair_l; a.joint_pair = joint_pair;
    a.d_mo = dL_dmean_offset; a.d_moo = dL_dmean_offset_offset; a.d_sc = dL_dscale; a.d_so = dL_dscale_offset;
    a.d_jo = dL_djoint_offset;
    set_counts(a, B, V, J, n_pairs);
    hipLaunchKernelGGL(offset_bwd, dim3((unsigned)(vblocks + jblocks)), dim3(OFF_BLOCK), 0, (hipStream_t)stream, a,
                       (int)vblocks);
    return launched("offset_bwd");
}

}  // extern "C"
