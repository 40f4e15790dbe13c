// The launches of the SMPL-X template stage (body.hip) that the posed stage (posed_body.hip) runs as well: the parameter
// blocks of the kernels and one host function per kernel that enqueues it on a stream.  Both sources are part of the
// exa_mesh ABI and report through its message buffer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace exa_mesh_impl {

// most coefficients of one body_shape launch: the shape stage's L <= 512 and the 9 (J - 1) <= 567 pose features
constexpr int BD_STAGE = 576;

// out[m] = base[m] + sum_l coef[l] dirs[l][m], the sum from +0.0 in ascending l; coefficient l is coef[l] for l < La and
// coef_b[l - La] for the others (La == L: one array)
struct ShapeParams {
    int32_t L, M;                             // M = 3 V
    int32_t La;
    const float* coef;
    const float* coef_b;
    const float* dirs;
    const float* base;
    const float* pose_offsets;                // NULL: v_posed is not written
    float* v_shaped;
    float* v_posed;
    float* zero3;                             // three floats that receive +0.0, or NULL
};

struct JregParams {
    int32_t V, nnz, root;                     // root: the joint whose joint_offset row is ignored, -1 for none
    const int32_t* off;
    const int32_t* col;
    const float* val;
    const float* v_shaped;
    const float* joint_offset;                // [J, 3] or NULL (nothing is added)
    float* Jr;
};

struct JregBwdParams {
    int32_t V, J, nnz, root;
    const int32_t* off;                       // the transposed CSR
    const int32_t* row;
    const float* val;
    const float* gJA;                         // [J, 3] or NULL
    const float* gJC;                         // [J, 3] or NULL
    const float* g_vp;                        // [V, 3] or NULL
    float* d_joint_offset;                    // [J, 3] or NULL
    float* dvs;                               // [V, 3] or NULL
};

// dcoef[l] = sum_m dirs[l][m] dvs[m] as the header's two-level sum; row l goes to dcoef[l] for l < split and to
// dcoef_b[l - split] for the others (split == L: one array)
struct CoefParams {
    int32_t L, M, chunks;
    int32_t split;
    const float* dirs;
    const float* dvs;
    float* partial;                           // [chunks, L]
    float* dcoef;
    float* dcoef_b;
};

// each enqueues its kernel on `st` and returns 0 or the ABI's status of the launch
int launch_body_shape(const ShapeParams& P, hipStream_t st);
int launch_body_jreg(const JregParams& P, int32_t J, hipStream_t st);
int launch_body_jreg_bwd(const JregBwdParams& P, bool all_vertices, hipStream_t st);
int launch_body_coef(const CoefParams& P, hipStream_t st);      // both launches of the two-level sum

// "skinning: <exa_skin_last_error()>" as this ABI's message; returns rc
int skin_failed(int rc);

}  // namespace exa_mesh_impl
