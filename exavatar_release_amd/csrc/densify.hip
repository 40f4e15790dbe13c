// Densification for gfx950 (include/exa_raster.h, exa_raster_densify_plan / exa_raster_densify_move): the clone, split and
// prune passes of the reference's SceneGaussian.densify_and_prune (avatar/common/nets/module.py:159-245) decided per SOURCE
// row and carried out as one move of all rows.  The header writes out the decision table and the children's arithmetic;
// tests/densify_oracle.py restates them in numpy.  Compiled with -ffp-contract=off and no fast-math flag.
//
//   densify_classify   one thread per source row: the row's code (KEEP / CLONE / SPLIT / CAND bits, one byte) and, per
//                      workgroup of DENSIFY_BLOCK rows, the counts of the four bits (ballot + popcount per wave, the four
//                      waves summed through LDS, one 16-byte plain store).  In mask mode the code is KEEP or nothing.
//   densify_scan       ONE workgroup of DENSIFY_SCAN threads: the per-workgroup counts become exclusive offsets in place
//                      (wave_incl_scan of wave_scan.h, a carry between rounds of DENSIFY_SCAN records), the four totals go
//                      to the 16-byte record at the head of the workspace.
//   densify_move       a workgroup owns the same DENSIFY_BLOCK source rows as in the classification.  It rebuilds in LDS
//                      the compact lists of its kept, cloned and split rows from the codes (ballot + popcount again: the
//                      rank of a row inside its list is the count of earlier rows with the bit), then walks, segment by
//                      segment, its slice of every output range as a flat run of count * row_floats floats: consecutive
//                      lanes store consecutive floats, and load consecutive floats wherever consecutive source rows are in
//                      the list.  The segments travel BY VALUE in the argument block.  The children's means go row by row
//                      (one thread builds the rotation of its source once and emits split_factor rows of 3 floats).
//                      Before it writes anything a workgroup compares the totals it was given with the record the scan
//                      left: a caller that passes other totals gets no store at all instead of one out of bounds.
// All accesses are 4 bytes wide: none of the reference's row widths (1, 3, 6, 45) lets a 16-byte access stay inside a row.
// No global atomics, no memset, no allocation, no synchronisation: the same inputs give the same bits.
#include <float.h>
#include "common.h"
#include "rot6d.h"
#include "wave_scan.h"

namespace exa {

namespace {

constexpr int DB = EXA_RASTER_DENSIFY_BLOCK;
constexpr int DS = EXA_RASTER_DENSIFY_SCAN;
constexpr int DW = DB / 64;                              // waves of a workgroup
static_assert(DB == 256 && DS % 64 == 0, "four waves per block of rows");
static_assert(DENSIFY_MAX_SEGMENTS == EXA_RASTER_DENSIFY_MAX_SEGMENTS, "segments per launch");
static_assert(sizeof(DensifyMoveArgs) <= 4096, "the argument block of a HIP kernel holds 4 KiB");

constexpr uint32_t KEEP = EXA_RASTER_DENSIFY_KEEP, CLONE = EXA_RASTER_DENSIFY_CLONE, SPLIT = EXA_RASTER_DENSIFY_SPLIT,
                   CAND = EXA_RASTER_DENSIFY_CAND;

// torch.max over a row: a NaN wins
__device__ __forceinline__ float max_nan(float m, float a) { return (a > m || a != a) ? a : m; }

__device__ __forceinline__ uint32_t classify_row(const DensifyPlanArgs& A, int i, float extent) {
    float g = A.grad_accum[i] / A.track_cnt[i];
    if (g != g) g = 0.0f;                                  // nan_to_num
    else if (g == INFINITY) g = FLT_MAX;
    else if (g == -INFINITY) g = -FLT_MAX;
    const bool hot = g >= A.grad_thr;
    const float e0 = expf(A.scale[3 * (size_t)i]), e1 = expf(A.scale[3 * (size_t)i + 1]), e2 = expf(A.scale[3 * (size_t)i + 2]);
    const float m = max_nan(max_nan(e0, e1), e2);
    const bool big = m > A.dense_percent * extent;
    const float o = A.opacity[i];
    const bool low = 1.0f / (1.0f + expf(-o)) < A.opacity_min;
    bool wide = false, wide_child = false, screen = false;
    if (A.prune_big) {
        const float lim = 0.1f * extent;
        wide = m > lim;
        const float c0 = expf(logf(e0 / A.child_div)), c1 = expf(logf(e1 / A.child_div)), c2 = expf(logf(e2 / A.child_div));
        wide_child = max_nan(max_nan(c0, c1), c2) > lim;
        if (A.radius_max) screen = A.radius_max[i] > A.screen_size_max;
    }
    uint32_t code = 0;
    if (!(hot && big) && !low && !wide && !screen) code |= KEEP;
    if (hot && !big && !low && !wide) code |= CLONE;
    if (hot && big && !low && !wide_child) code |= SPLIT;
    if (hot && big) code |= CAND;
    return code;
}

__global__ __launch_bounds__(DB) void densify_classify(DensifyPlanArgs A) {
    __shared__ uint32_t s_cnt[DW][4];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int64_t i = (int64_t)blockIdx.x * DB + t;
    uint32_t code = 0;
    if (i < A.P0) {
        code = A.mask ? (A.mask[i] ? 0u : KEEP) : classify_row(A, (int)i, *A.extent);
        A.codes[i] = (uint8_t)code;
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const unsigned long long m = __ballot((code >> b) & 1u);
        if (lane == 0) s_cnt[wave][b] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (t == 0) {
        uint4 c;
        c.x = s_cnt[0][0] + s_cnt[1][0] + s_cnt[2][0] + s_cnt[3][0];
        c.y = s_cnt[0][1] + s_cnt[1][1] + s_cnt[2][1] + s_cnt[3][1];
        c.z = s_cnt[0][2] + s_cnt[1][2] + s_cnt[2][2] + s_cnt[3][2];
        c.w = s_cnt[0][3] + s_cnt[1][3] + s_cnt[2][3] + s_cnt[3][3];
        A.counts[blockIdx.x] = c;
    }
}

__global__ __launch_bounds__(DS) void densify_scan(uint4* __restrict__ counts, int nb, uint4* __restrict__ record) {
    __shared__ uint32_t s_w[DS / 64][4];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    uint32_t carry[4] = {0, 0, 0, 0};
    for (int base = 0; base < nb; base += DS) {            // uniform: every thread takes every round
        const int k = base + t;
        const uint4 c = k < nb ? counts[k] : make_uint4(0, 0, 0, 0);
        const uint32_t v[4] = {c.x, c.y, c.z, c.w};
        uint32_t incl[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            incl[b] = wave_incl_scan(v[b]);
            if (lane == 63) s_w[wave][b] = incl[b];
        }
        __syncthreads();
        uint32_t out[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            uint32_t before = 0, total = 0;
            for (int w = 0; w < DS / 64; ++w) {
                const uint32_t x = s_w[w][b];
                if (w < wave) before += x;
                total += x;
            }
            out[b] = carry[b] + before + incl[b] - v[b];
            carry[b] += total;
        }
        __syncthreads();
        if (k < nb) counts[k] = make_uint4(out[0], out[1], out[2], out[3]);
    }
    if (t == 0) *record = make_uint4(carry[0], carry[1], carry[2], carry[3]);
}

// the flat run of n_rows * w floats of one output range: float e of the run belongs to list row e / w
template <typename I, typename F>
__device__ __forceinline__ void walk(int n_rows, I w, F&& f) {
    const I n = (I)n_rows * w;
    for (I e = threadIdx.x; e < n; e += DB) {
        const I r = e / w;
        f(e, (int)r, e - r * w);
    }
}

template <typename I>
__device__ __forceinline__ void move_segment(const ExaRasterDensifySegment& S, const DensifyMoveArgs& A, int64_t row0,
                                             const uint16_t* keep, const uint16_t* clone, const uint16_t* split,
                                             const uint16_t* split_cand, int nk, int nc, int ns, const uint4 off) {
    const I w = (I)S.row_floats;
    const size_t W = (size_t)S.row_floats;
    const float* const src = S.src + (size_t)row0 * W;
    float* const d_keep = S.dst + (size_t)off.x * W;
    walk<I>(nk, w, [&](I e, int r, I c) { d_keep[e] = src[(size_t)keep[r] * W + c]; });
    const bool state = S.role == EXA_RASTER_DENSIFY_STATE;
    float* const d_clone = S.dst + ((size_t)A.n_keep + off.y) * W;
    if (state) walk<I>(nc, w, [&](I e, int, I) { d_clone[e] = 0.0f; });
    else walk<I>(nc, w, [&](I e, int r, I c) { d_clone[e] = src[(size_t)clone[r] * W + c]; });
    if (S.role == EXA_RASTER_DENSIFY_MEAN) {               // row_floats = 3: one thread per split row
        for (int j = threadIdx.x; j < ns; j += DB) {
            const size_t row = (size_t)row0 + split[j];
            float a[6], n[3], mu[3], sd[3];
#pragma unroll
            for (int k = 0; k < 6; ++k) a[k] = A.rotation[row * 6 + k];
#pragma unroll
            for (int k = 0; k < 3; ++k) { sd[k] = expf(A.scale[row * 3 + k]); mu[k] = S.src[row * 3 + k]; }
            rot6d::Frame f;
            rot6d::frame(a, f);
            const size_t cand = (size_t)off.w + split_cand[j];
            for (int c = 0; c < A.split_factor; ++c) {
                const float* const z = A.noise + ((size_t)c * A.n_cand + cand) * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) n[k] = z[k] * sd[k];
                float* const o = S.dst + ((size_t)A.n_keep + A.n_clone + (size_t)c * A.n_split + off.z + j) * 3;
                o[0] = ((f.b1[0] * n[0] + f.b1[1] * n[1]) + f.b1[2] * n[2]) + mu[0];
                o[1] = ((f.b2[0] * n[0] + f.b2[1] * n[1]) + f.b2[2] * n[2]) + mu[1];
                o[2] = ((f.b3[0] * n[0] + f.b3[1] * n[1]) + f.b3[2] * n[2]) + mu[2];
            }
        }
        return;
    }
    for (int c = 0; c < A.split_factor; ++c) {
        float* const d = S.dst + ((size_t)A.n_keep + A.n_clone + (size_t)c * A.n_split + off.z) * W;
        if (state) walk<I>(ns, w, [&](I e, int, I) { d[e] = 0.0f; });
        else if (S.role == EXA_RASTER_DENSIFY_SCALE)
            walk<I>(ns, w, [&](I e, int r, I k) { d[e] = logf(expf(src[(size_t)split[r] * W + k]) / A.child_div); });
        else walk<I>(ns, w, [&](I e, int r, I k) { d[e] = src[(size_t)split[r] * W + k]; });
    }
}

__global__ __launch_bounds__(DB) void densify_move(DensifyMoveArgs A) {
    __shared__ uint16_t s_keep[DB], s_clone[DB], s_split[DB], s_split_cand[DB];
    __shared__ uint32_t s_cnt[DW][4];
    const uint4 rec = *A.record;
    if ((int)rec.x != A.n_keep || (int)rec.y != A.n_clone || (int)rec.z != A.n_split || (int)rec.w != A.n_cand) return;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int64_t row0 = (int64_t)blockIdx.x * DB;
    const uint32_t code = row0 + t < A.P0 ? A.codes[row0 + t] : 0u;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t rank[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const unsigned long long m = __ballot((code >> b) & 1u);
        rank[b] = (uint32_t)__popcll(m & below);
        if (lane == 0) s_cnt[wave][b] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    uint32_t total[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        uint32_t before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < DW; ++w) {
            const uint32_t x = s_cnt[w][b];
            if (w < wave) before += x;
            tot += x;
        }
        rank[b] += before;
        total[b] = tot;
    }
    if (code & KEEP) s_keep[rank[0]] = (uint16_t)t;
    if (code & CLONE) s_clone[rank[1]] = (uint16_t)t;
    if (code & SPLIT) { s_split[rank[2]] = (uint16_t)t; s_split_cand[rank[2]] = (uint16_t)rank[3]; }
    __syncthreads();
    const uint4 off = A.offsets[blockIdx.x];
    for (int s = 0; s < A.n_seg; ++s) {
        const ExaRasterDensifySegment& S = A.seg[s];
        if (S.row_floats <= 65536)
            move_segment<uint32_t>(S, A, row0, s_keep, s_clone, s_split, s_split_cand, (int)total[0], (int)total[1],
                                   (int)total[2], off);
        else
            move_segment<uint64_t>(S, A, row0, s_keep, s_clone, s_split, s_split_cand, (int)total[0], (int)total[1],
                                   (int)total[2], off);
    }
}

}  // namespace

hipError_t launch_densify_plan(const DensifyPlanArgs& A, uint4* record, hipStream_t s) {
    const int nb = (int)(((int64_t)A.P0 + DB - 1) / DB);
    hipLaunchKernelGGL(densify_classify, dim3(nb), dim3(DB), 0, s, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(densify_scan, dim3(1), dim3(DS), 0, s, A.counts, nb, record);
    return hipGetLastError();
}

hipError_t launch_densify_move(const DensifyMoveArgs& A, hipStream_t s) {
    const int nb = (int)(((int64_t)A.P0 + DB - 1) / DB);
    hipLaunchKernelGGL(densify_move, dim3(nb), dim3(DB), 0, s, A);
    return hipGetLastError();
}

}  // namespace exa
