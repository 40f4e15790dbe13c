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

#include <algorithm>
#include <vector>

#include "../../include/exa_raster.h"
#include "abi_status.h"
#include "rot6d.h"
#include "wave_scan.h"

namespace exa {

// the kernels' argument blocks, as exa_raster_densify_plan / exa_raster_densify_move fill them: the classification with its
// scan, and the move of up to DENSIFY_MAX_SEGMENTS tensors
constexpr int DENSIFY_MAX_SEGMENTS = 64;
struct DensifyPlanArgs {
    int32_t P0;
    int32_t prune_big;
    const float *grad_accum, *track_cnt, *scale, *opacity;
    const float* radius_max;                   // NULL: no screen-space rule
    const float* extent;
    const uint8_t* mask;                       // not NULL: mask mode, the six pointers above are not looked at
    float grad_thr, dense_percent, opacity_min, child_div, screen_size_max;
    uint8_t* codes;                            // the sections of the workspace
    uint4* counts;
};
struct DensifyMoveArgs {
    int32_t P0, split_factor, n_keep, n_clone, n_split, n_cand, n_seg;
    float child_div;                           // (float)(0.8 * split_factor)
    const uint4* record;                       // the sections of the workspace
    const uint4* offsets;
    const uint8_t* codes;
    const float *rotation, *scale, *noise;     // the children's sources
    ExaRasterDensifySegment seg[DENSIFY_MAX_SEGMENTS];
};

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

}  // namespace exa

// ---- C entry points (include/exa_raster.h): checks, the argument blocks, the launches --------------------------------------
namespace exa_raster_impl {

using namespace exa;

EXA_ABI_STATUS_SHARED("exa_raster")       // exa_raster_last_error() and its buffer are api.hip's

// the workspace: the record of the four totals | 16 bytes per workgroup of rows | the codes, one byte per row
static uint64_t densify_blocks(int32_t P0) { return ((uint64_t)P0 + DB - 1) / DB; }
static uint64_t densify_bytes(int32_t P0) { return 16 + 16 * densify_blocks(P0) + 16 * (((uint64_t)P0 + 15) / 16); }

static int densify_check_workspace(int32_t P0, const void* workspace, uint64_t workspace_bytes) {
    if (!workspace) return fail(EXA_RASTER_E_NULLPTR, "densify: workspace is NULL");
    if (workspace_bytes < densify_bytes(P0))
        return fail(EXA_RASTER_E_WORKSPACE, "densify: workspace smaller than exa_raster_densify_workspace_size");
    if ((uintptr_t)workspace & 15) return fail(EXA_RASTER_E_WORKSPACE, "densify: workspace must be 16-byte aligned");
    return 0;
}

}  // namespace exa_raster_impl

using namespace exa_raster_impl;

extern "C" {

int exa_raster_densify_workspace_size(int32_t P0, uint64_t* bytes) {
    if (!bytes) return fail(EXA_RASTER_E_NULLPTR, "densify: bytes is NULL");
    if (P0 < 0) return fail(EXA_RASTER_E_INVALID, "densify: negative P0");
    *bytes = densify_bytes(P0);
    return 0;
}

int exa_raster_densify_plan(int32_t P0, const float* grad_accum, const float* track_cnt, const float* scale,
                            const float* opacity, const float* radius_max, const float* extent, const uint8_t* mask,
                            double grad_thr, double dense_percent, double opacity_min, int32_t prune_big,
                            int32_t split_factor, double screen_size_max, void* workspace, uint64_t workspace_bytes,
                            void* stream) {
    if (P0 < 0) return fail(EXA_RASTER_E_INVALID, "densify: negative P0");
    if (split_factor < 1 || split_factor > 8) return fail(EXA_RASTER_E_INVALID, "densify: split_factor must be in 1..8");
    if (P0 == 0) return 0;
    if (!mask && (!grad_accum || !track_cnt || !scale || !opacity || !extent))
        return fail(EXA_RASTER_E_NULLPTR, "densify: NULL argument");
    if (int rc = densify_check_workspace(P0, workspace, workspace_bytes)) return rc;
    char* const ws = static_cast<char*>(workspace);
    DensifyPlanArgs A;
    A.P0 = P0;
    A.prune_big = prune_big != 0;
    A.grad_accum = grad_accum; A.track_cnt = track_cnt; A.scale = scale; A.opacity = opacity; A.extent = extent;
    A.radius_max = (prune_big && screen_size_max > 0.0) ? radius_max : nullptr;
    A.mask = mask;
    A.grad_thr = (float)grad_thr; A.dense_percent = (float)dense_percent; A.opacity_min = (float)opacity_min;
    A.child_div = (float)(0.8 * split_factor);
    A.screen_size_max = (float)screen_size_max;
    A.counts = reinterpret_cast<uint4*>(ws + 16);
    A.codes = reinterpret_cast<uint8_t*>(ws + 16 + 16 * densify_blocks(P0));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nb = (int)densify_blocks(P0);
    hipLaunchKernelGGL(densify_classify, dim3(nb), dim3(DB), 0, s, A);
    if (int rc = launched("densify_plan")) return rc;
    hipLaunchKernelGGL(densify_scan, dim3(1), dim3(DS), 0, s, A.counts, nb, reinterpret_cast<uint4*>(ws));
    return launched("densify_plan");
}

int exa_raster_densify_move(int32_t P0, int32_t split_factor, const void* workspace, uint64_t workspace_bytes,
                            int32_t n_keep, int32_t n_clone, int32_t n_split, int32_t n_cand,
                            const ExaRasterDensifySegment* segs, int32_t n_seg, const float* rotation, const float* scale,
                            const float* noise, void* stream) {
    if (P0 < 0 || n_seg < 0) return fail(EXA_RASTER_E_INVALID, "densify: negative size");
    if (split_factor < 1 || split_factor > 8) return fail(EXA_RASTER_E_INVALID, "densify: split_factor must be in 1..8");
    if (n_keep < 0 || n_clone < 0 || n_split < 0 || n_cand < 0 || n_keep > P0 || n_clone > P0 || n_cand > P0 ||
        n_split > n_cand)
        return fail(EXA_RASTER_E_INVALID, "densify: the totals are not those of a plan over P0 rows");
    if (P0 == 0 || n_seg == 0) return 0;
    if (!segs) return fail(EXA_RASTER_E_NULLPTR, "densify: segs is NULL");
    if (int rc = densify_check_workspace(P0, workspace, workspace_bytes)) return rc;
    const int64_t n_out = (int64_t)n_keep + n_clone + (int64_t)split_factor * n_split;
    bool any_mean = false;
    for (int32_t s = 0; s < n_seg; ++s) {
        const ExaRasterDensifySegment& g = segs[s];
        if (g.row_floats < 1) return fail(EXA_RASTER_E_INVALID, "densify: row_floats must be >= 1");
        if (g.role < EXA_RASTER_DENSIFY_COPY || g.role > EXA_RASTER_DENSIFY_SCALE)
            return fail(EXA_RASTER_E_INVALID, "densify: unknown role");
        if (g.role == EXA_RASTER_DENSIFY_MEAN && g.row_floats != 3)
            return fail(EXA_RASTER_E_INVALID, "densify: a MEAN segment has row_floats = 3");
        if (g.dst_rows < n_out) return fail(EXA_RASTER_E_INVALID, "densify: the totals do not fit dst (dst_rows < n_out)");
        if (g.row_floats > (INT64_C(1) << 40) / ((int64_t)P0 + n_out + 1))
            return fail(EXA_RASTER_E_INVALID, "densify: a segment of more than 2^40 floats");
        if (!g.src || (n_out > 0 && !g.dst)) return fail(EXA_RASTER_E_NULLPTR, "densify: a segment holds a NULL pointer");
        any_mean |= g.role == EXA_RASTER_DENSIFY_MEAN;
    }
    if (any_mean && (!rotation || !scale || (n_cand > 0 && !noise)))
        return fail(EXA_RASTER_E_NULLPTR, "densify: a MEAN segment needs rotation, scale and noise");
    // every written range against every range of the call: sorted by start, one sweep
    struct Span { uintptr_t lo, hi; bool written; };
    std::vector<Span> spans;
    auto add = [&spans](const void* p, uint64_t bytes, bool written) {
        if (p && bytes) spans.push_back({(uintptr_t)p, (uintptr_t)p + bytes, written});
    };
    add(workspace, densify_bytes(P0), false);
    if (any_mean) {
        add(rotation, (uint64_t)P0 * 24, false);
        add(scale, (uint64_t)P0 * 12, false);
        add(noise, (uint64_t)split_factor * n_cand * 12, false);
    }
    for (int32_t s = 0; s < n_seg; ++s) {
        add(segs[s].src, (uint64_t)P0 * segs[s].row_floats * 4, false);
        add(segs[s].dst, (uint64_t)n_out * segs[s].row_floats * 4, true);
    }
    std::sort(spans.begin(), spans.end(), [](const Span& a, const Span& b) { return a.lo < b.lo || (a.lo == b.lo && a.hi < b.hi); });
    uintptr_t w_end = 0, r_end = 0;
    for (const Span& sp : spans) {
        if (sp.lo < w_end || (sp.written && sp.lo < r_end))
            return fail(EXA_RASTER_E_ALIAS, "densify: a dst range overlaps another range of the call");
        if (sp.written) w_end = std::max(w_end, sp.hi); else r_end = std::max(r_end, sp.hi);
    }
    const char* const ws = static_cast<const char*>(workspace);
    DensifyMoveArgs A;
    A.P0 = P0; A.split_factor = split_factor;
    A.n_keep = n_keep; A.n_clone = n_clone; A.n_split = n_split; A.n_cand = n_cand;
    A.child_div = (float)(0.8 * split_factor);
    A.record = reinterpret_cast<const uint4*>(ws);
    A.offsets = reinterpret_cast<const uint4*>(ws + 16);
    A.codes = reinterpret_cast<const uint8_t*>(ws + 16 + 16 * densify_blocks(P0));
    A.rotation = rotation; A.scale = scale; A.noise = noise;
    for (int32_t s0 = 0; s0 < n_seg; s0 += DENSIFY_MAX_SEGMENTS) {
        A.n_seg = std::min<int32_t>(DENSIFY_MAX_SEGMENTS, n_seg - s0);
        for (int k = 0; k < DENSIFY_MAX_SEGMENTS; ++k) A.seg[k] = k < A.n_seg ? segs[s0 + k] : ExaRasterDensifySegment{};
        hipLaunchKernelGGL(densify_move, dim3((int)densify_blocks(P0)), dim3(DB), 0, static_cast<hipStream_t>(stream), A);
        if (int rc = launched("densify_move")) return rc;
    }
    return 0;
}

}  // extern "C"
