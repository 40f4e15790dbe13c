// K-nearest-neighbour search, squared L2, D = 3 (include/exa_knn.h): pytorch3d knn_points as ExAvatar calls it for the
// per-frame nearest template vertex (reference module.py:543, K = 1) and the init-time scene scale (module.py:86, K = 4).
// The semantics -- lexicographic (d, j), d rounded operation by operation -- are written out in the header; this file
// implements them.
//
// Search (one wave of 64 queries per workgroup, one query per lane):
//   every lane keeps its K best (d, j) pairs sorted in registers (KK >= K slots, KK a power of two); refs are streamed
//   through LDS in chunks of 64 and every lane compares its query against each of them.  A candidate enters only when it
//   is lexicographically smaller than the last slot, so the visiting order does not change the result.
//
// Culling (the default; EXA_KNN_NO_CULL visits every chunk in index order instead):
//   knn_bbox_part   64 workgroups per batch element: partial bounding boxes of p1 and p2 together.
//   knn_sort_pass   <false> one workgroup per 1024 points of one set: the Morton code of the point's cell of a 16^3 grid
//                   over that box, the point's stable rank among the chunk's points of its cell (ballots inside a wave,
//                   the 16 waves in order through an LDS histogram), the chunk's histogram as a row of the (chunk, cell)
//                   count matrix.
//   knn_col_scan    per cell: exclusive prefix of the count matrix's column over the chunks (in place), cell totals.
//   knn_cell_scan   per set: exclusive prefix of the totals over the cells = where each cell starts in sorted order.
//   knn_sort_pass   <true> the same ranks again, and every point scattered to start[cell] + prefix[chunk][cell] + rank
//                   as (x, y, z, original index): a stable counting sort by cell, no atomics.
//   knn_boxes       one wave per 64 sorted refs: the chunk's axis-aligned box.
//   knn_search      each wave takes 64 consecutive sorted queries and their box, visits the ref chunk where its cell
//                   starts, then tests the boxes of all chunks 64 at a time against the wave's box and its largest K-th
//                   distance (one chunk per lane, a ballot, the set bits walked in order); a chunk that passes is
//                   tested against every lane's own query and K-th distance and visited unless, for every lane, its
//                   lower bound is strictly greater.  Results go to the query's original position.
//
// The lower bound of a chunk is the fp32 squared distance between the two boxes (or the query and the box), evaluated
// like d.  Rounding is
// monotone and a.x - b.x rounds to exactly -(b.x - a.x), so for every pair of the two boxes the computed d is already >=
// the computed bound; the bound is still shrunk by 2^-20 relative before the test, so that no ref with d <= the K-th
// distance can be skipped, ties included, even if an evaluation rounds differently.
//
// Compiled with -ffp-contract=off (build.py): d must not be contracted into fused multiply-adds.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/exa_knn.h"
#include "abi_status.h"

namespace exa_knn_impl {

using exa::align256;
using exa::ceil_div;

constexpr int WAVE = 64;
constexpr int NPART = 64;                    // partial boxes per batch element (= one wave reduces them)
constexpr int GRID_BITS = 4;                 // 16 cells per axis
constexpr int GRID = 1 << GRID_BITS;
constexpr int CELLS = GRID * GRID * GRID;    // 4096
constexpr int SORT_CHUNK = 1024;             // points per workgroup of the counting sort (one per thread)
constexpr int SORT_WAVES = SORT_CHUNK / WAVE;
constexpr int REF_CHUNK = 64;                // refs per LDS chunk and per culling box
constexpr int BLOCK = 256;
constexpr float CULL_MARGIN = 1.0f - 0x1p-20f;

struct Params {
    int N, P1, P2, K;
    const float* p1;                         // [N, P1, 3]
    const float* p2;                         // [N, P2, 3]
    float* dists;                            // [N, P1, K]
    int64_t* idx;                            // [N, P1, K]
    uint32_t* wave_refs;                     // [N, ceil(P1 / 64)] or NULL
    // culling workspace
    float4* part;                            // [N, NPART, 2]: lo, hi
    uint32_t* cnt1;                          // [N, chunks(P1), CELLS]
    uint32_t* cnt2;                          // [N, chunks(P2), CELLS]
    uint32_t* tot;                           // [N, 2, CELLS]
    uint32_t* start;                         // [N, 2, CELLS + 1]
    float4* s1;                              // [N, P1]: sorted queries, w = original index
    float4* s2;                              // [N, P2]: sorted refs, w = original index
    float4* boxes;                           // [N, chunks64(P2), 2]: lo, hi
};

__host__ __device__ inline int sort_chunks(int P) { return (P + SORT_CHUNK - 1) / SORT_CHUNK; }
__host__ __device__ inline int ref_chunks(int P) { return (P + REF_CHUNK - 1) / REF_CHUNK; }

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) v = fminf(v, __shfl_xor(v, o, WAVE));
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, WAVE));
    return v;
}

__device__ __forceinline__ uint64_t lanes_below(int lane) { return lane ? (~0ull >> (WAVE - lane)) : 0ull; }

__device__ __forceinline__ float uniform(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// ---- the grid of the culling sort -----------------------------------------------------------------------------------

struct Grid {
    float lx, ly, lz;                        // box corner
    float sx, sy, sz;                        // cells per unit length (0 on a flat or unbounded axis)
};

// The batch element's box from the NPART partials, reduced by one wave (every lane gets the same result; every wave
// that asks computes the same bits, min and max being exact).
__device__ Grid grid_of(const Params& P, int b) {
    const int lane = threadIdx.x & (WAVE - 1);
    const float4 lo = P.part[((size_t)b * NPART + lane) * 2];
    const float4 hi = P.part[((size_t)b * NPART + lane) * 2 + 1];
    Grid g;
    g.lx = wave_min(lo.x); g.ly = wave_min(lo.y); g.lz = wave_min(lo.z);
    const float ex = wave_max(hi.x) - g.lx, ey = wave_max(hi.y) - g.ly, ez = wave_max(hi.z) - g.lz;
    g.sx = ex > 0.f ? (float)GRID / ex : 0.f;
    g.sy = ey > 0.f ? (float)GRID / ey : 0.f;
    g.sz = ez > 0.f ? (float)GRID / ez : 0.f;
    return g;
}

__device__ __forceinline__ int axis_cell(float v, float lo, float s) {
    const float t = (v - lo) * s;
    return t > 0.f ? (int)fminf(t, (float)(GRID - 1)) : 0;     // NaN (an infinite extent) lands in cell 0
}

__device__ __forceinline__ uint32_t spread3(uint32_t v) {      // bit k -> bit 3k, GRID_BITS bits
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < GRID_BITS; ++k) r |= ((v >> k) & 1u) << (3 * k);
    return r;
}

__device__ __forceinline__ int cell_of(float x, float y, float z, const Grid& g) {
    return (int)(spread3(axis_cell(x, g.lx, g.sx)) | (spread3(axis_cell(y, g.ly, g.sy)) << 1) |
                 (spread3(axis_cell(z, g.lz, g.sz)) << 2));
}

// ---- culling sort ---------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(BLOCK) knn_bbox_part(Params P) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t total = (int64_t)P.P1 + P.P2;
    float lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
    for (int64_t s = (int64_t)blockIdx.x * BLOCK + tid; s < total; s += (int64_t)NPART * BLOCK) {
        const float* p = s < P.P1 ? P.p1 + ((int64_t)b * P.P1 + s) * 3 : P.p2 + ((int64_t)b * P.P2 + (s - P.P1)) * 3;
        const float x = p[0], y = p[1], z = p[2];
        lx = fminf(lx, x); ly = fminf(ly, y); lz = fminf(lz, z);
        hx = fmaxf(hx, x); hy = fmaxf(hy, y); hz = fmaxf(hz, z);
    }
    lx = wave_min(lx); ly = wave_min(ly); lz = wave_min(lz);
    hx = wave_max(hx); hy = wave_max(hy); hz = wave_max(hz);
    __shared__ float4 s_lo[BLOCK / WAVE], s_hi[BLOCK / WAVE];
    const int wave = tid / WAVE;
    if ((tid & (WAVE - 1)) == 0) {
        s_lo[wave] = make_float4(lx, ly, lz, 0.f);
        s_hi[wave] = make_float4(hx, hy, hz, 0.f);
    }
    __syncthreads();
    if (tid == 0) {
        float4 lo = s_lo[0], hi = s_hi[0];
        for (int w = 1; w < BLOCK / WAVE; ++w) {
            lo.x = fminf(lo.x, s_lo[w].x); lo.y = fminf(lo.y, s_lo[w].y); lo.z = fminf(lo.z, s_lo[w].z);
            hi.x = fmaxf(hi.x, s_hi[w].x); hi.y = fmaxf(hi.y, s_hi[w].y); hi.z = fmaxf(hi.z, s_hi[w].z);
        }
        P.part[((size_t)b * NPART + blockIdx.x) * 2] = lo;
        P.part[((size_t)b * NPART + blockIdx.x) * 2 + 1] = hi;
    }
}

// blockIdx = (chunk, batch element, set): set 0 = queries (p1), 1 = refs (p2).  SCATTER = false writes the chunk's row
// of the count matrix; SCATTER = true (after the scans) writes the points to their sorted positions.
template <bool SCATTER>
__global__ void __launch_bounds__(SORT_CHUNK) knn_sort_pass(Params P) {
    const int set = blockIdx.z, b = blockIdx.y, ch = blockIdx.x;
    const int Pn = set ? P.P2 : P.P1;
    if (ch >= sort_chunks(Pn)) return;                         // whole workgroup
    __shared__ uint32_t hist[CELLS];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const Grid g = grid_of(P, b);
    const int i = ch * SORT_CHUNK + tid;
    const bool valid = i < Pn;
    const float* src = (set ? P.p2 + (int64_t)b * P.P2 * 3 : P.p1 + (int64_t)b * P.P1 * 3) + (int64_t)i * 3;
    float x = 0.f, y = 0.f, z = 0.f;
    if (valid) { x = src[0]; y = src[1]; z = src[2]; }
    const int cell = valid ? cell_of(x, y, z, g) : -1;

    // rank among the lower lanes of this wave in the same cell; the group's lowest lane ("lead") holds the group size
    uint64_t active = __ballot(valid);
    int rank = 0, gsize = 0, lead = 0;
    while (active) {
        const int l = __ffsll((unsigned long long)active) - 1;
        const int c = __builtin_amdgcn_readlane(cell, l);
        const uint64_t m = __ballot(cell == c);
        if (cell == c) {
            rank = __popcll(m & lanes_below(lane));
            gsize = __popcll(m);
            lead = l;
        }
        active &= ~m;
    }
    for (int c = tid; c < CELLS; c += SORT_CHUNK) hist[c] = 0;
    __syncthreads();
    // the waves in order: each group's lead takes the cell's running count as its base and adds its group
    int base = 0;
    for (int w = 0; w < SORT_WAVES; ++w) {
        if (wave == w && valid && lane == lead) {
            base = hist[cell];
            hist[cell] = base + gsize;
        }
        __syncthreads();
    }
    base = __shfl(base, lead, WAVE);
    uint32_t* cnt = set ? P.cnt2 + ((size_t)b * sort_chunks(P.P2) + ch) * CELLS
                        : P.cnt1 + ((size_t)b * sort_chunks(P.P1) + ch) * CELLS;
    if (!SCATTER) {
        for (int c = tid; c < CELLS; c += SORT_CHUNK) cnt[c] = hist[c];
    } else if (valid) {
        const uint32_t dest = P.start[((size_t)b * 2 + set) * (CELLS + 1) + cell] + cnt[cell] + base + rank;
        float4* dst = set ? P.s2 + (size_t)b * P.P2 : P.s1 + (size_t)b * P.P1;
        if (dest < (uint32_t)Pn) dst[dest] = make_float4(x, y, z, __int_as_float(i));     // always, by construction
    }
}

// blockIdx = (64 cells, set, batch element); wave r of the 16 takes a contiguous range of the chunks.
__global__ void __launch_bounds__(SORT_CHUNK) knn_col_scan(Params P) {
    const int set = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & (WAVE - 1), r = threadIdx.x / WAVE;
    const int cell = blockIdx.x * WAVE + lane;
    const int nch = sort_chunks(set ? P.P2 : P.P1);
    uint32_t* col = (set ? P.cnt2 + (size_t)b * sort_chunks(P.P2) * CELLS : P.cnt1 + (size_t)b * sort_chunks(P.P1) * CELLS)
                    + cell;
    const int L = (nch + SORT_WAVES - 1) / SORT_WAVES;
    const int c0 = min(nch, r * L), c1 = min(nch, c0 + L);
    uint32_t sum = 0;
    for (int c = c0; c < c1; ++c) sum += col[(size_t)c * CELLS];
    __shared__ uint32_t s[SORT_WAVES][WAVE];
    s[r][lane] = sum;
    __syncthreads();
    uint32_t run = 0;
    for (int q = 0; q < r; ++q) run += s[q][lane];
    if (r == SORT_WAVES - 1) P.tot[((size_t)b * 2 + set) * CELLS + cell] = run + sum;
    for (int c = c0; c < c1; ++c) {
        const uint32_t v = col[(size_t)c * CELLS];
        col[(size_t)c * CELLS] = run;
        run += v;
    }
}

// blockIdx = (set, batch element): exclusive prefix of the cell totals, 4 cells per thread.
__global__ void __launch_bounds__(1024) knn_cell_scan(Params P) {
    const int set = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int lane = tid & (WAVE - 1), wave = tid / WAVE;
    const uint32_t* t = P.tot + ((size_t)b * 2 + set) * CELLS + tid * 4;
    uint32_t* st = P.start + ((size_t)b * 2 + set) * (CELLS + 1);
    const uint32_t v0 = t[0], v1 = t[1], v2 = t[2], v3 = t[3];
    const uint32_t mine = v0 + v1 + v2 + v3;
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint32_t n = __shfl_up(incl, d, WAVE);
        if (lane >= d) incl += n;
    }
    __shared__ uint32_t s_w[1024 / WAVE];
    if (lane == WAVE - 1) s_w[wave] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wave; ++w) base += s_w[w];
    base += incl - mine;
    st[tid * 4] = base;
    st[tid * 4 + 1] = base + v0;
    st[tid * 4 + 2] = base + v0 + v1;
    st[tid * 4 + 3] = base + v0 + v1 + v2;
    if (tid == 1023) st[CELLS] = base + mine;
}

// one wave per chunk of 64 sorted refs: its box
__global__ void __launch_bounds__(BLOCK) knn_boxes(Params P) {
    const int b = blockIdx.y, lane = threadIdx.x & (WAVE - 1);
    const int c = blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
    const int nch = ref_chunks(P.P2);
    if (c >= nch) return;                                      // whole wave
    const int j = c * REF_CHUNK + lane;
    float lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
    if (j < P.P2) {
        const float4 r = P.s2[(size_t)b * P.P2 + j];
        lx = hx = r.x; ly = hy = r.y; lz = hz = r.z;
    }
    lx = wave_min(lx); ly = wave_min(ly); lz = wave_min(lz);
    hx = wave_max(hx); hy = wave_max(hy); hz = wave_max(hz);
    if (lane == 0) {
        P.boxes[((size_t)b * nch + c) * 2] = make_float4(lx, ly, lz, 0.f);
        P.boxes[((size_t)b * nch + c) * 2 + 1] = make_float4(hx, hy, hz, 0.f);
    }
}

// ---- search ---------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool lex_less(float d, int j, float e, int k) { return d < e || (d == e && j < k); }

template <int KK>
__device__ __forceinline__ void insert(float (&dk)[KK], int (&jk)[KK], float d, int j) {
    float cd = d;
    int cj = j;
#pragma unroll
    for (int t = 0; t < KK; ++t) {
        const bool lt = lex_less(cd, cj, dk[t], jk[t]);
        const float td = dk[t];
        const int tj = jk[t];
        dk[t] = lt ? cd : td;
        jk[t] = lt ? cj : tj;
        cd = lt ? td : cd;
        cj = lt ? tj : cj;
    }
}

// blockIdx = (64 queries, batch element), one wave per workgroup.
template <int KK, bool CULL>
__global__ void __launch_bounds__(WAVE) knn_search(Params P) {
    const int b = blockIdx.y, lane = threadIdx.x;
    const int q = blockIdx.x * WAVE + lane;
    const bool valid = q < P.P1;
    const int nch = ref_chunks(P.P2);
    float qx = 0.f, qy = 0.f, qz = 0.f;
    int qi = q;
    if (valid) {
        if (CULL) {
            const float4 v = P.s1[(size_t)b * P.P1 + q];
            qx = v.x; qy = v.y; qz = v.z;
            qi = __float_as_int(v.w);
        } else {
            const float* a = P.p1 + ((int64_t)b * P.P1 + q) * 3;
            qx = a[0]; qy = a[1]; qz = a[2];
        }
    }
    float dk[KK];
    int jk[KK];
#pragma unroll
    for (int t = 0; t < KK; ++t) { dk[t] = INFINITY; jk[t] = INT32_MAX; }

    __shared__ float4 s_ref[REF_CHUNK];
    uint32_t visited = 0;
    auto visit = [&](int c) {                                  // c is wave-uniform
        const int base = c * REF_CHUNK;
        const int n = min(REF_CHUNK, P.P2 - base);
        __syncthreads();                                       // the previous chunk's readers are done
        if (lane < n) {
            if (CULL) {
                s_ref[lane] = P.s2[(size_t)b * P.P2 + base + lane];
            } else {
                const float* r = P.p2 + ((int64_t)b * P.P2 + base + lane) * 3;
                s_ref[lane] = make_float4(r[0], r[1], r[2], __int_as_float(base + lane));
            }
        }
        __syncthreads();
        for (int t = 0; t < n; ++t) {
            const float4 r = s_ref[t];
            const float dx = qx - r.x, dy = qy - r.y, dz = qz - r.z;
            const float d = (dx * dx + dy * dy) + dz * dz;
            const int j = __float_as_int(r.w);
            if (lex_less(d, j, dk[KK - 1], jk[KK - 1])) insert<KK>(dk, jk, d, j);
        }
        visited += n;
    };

    if (!CULL) {
        for (int c = 0; c < nch; ++c) visit(c);
    } else {
        // the wave's queries' box
        const float qlx = wave_min(valid ? qx : INFINITY), qly = wave_min(valid ? qy : INFINITY),
                    qlz = wave_min(valid ? qz : INFINITY);
        const float qhx = wave_max(valid ? qx : -INFINITY), qhy = wave_max(valid ? qy : -INFINITY),
                    qhz = wave_max(valid ? qz : -INFINITY);
        // the largest K-th distance over the wave's queries (+inf until every lane holds K candidates)
        // this lane's K-th distance (+inf until it holds K candidates; -inf for a lane without a query)
        auto kth = [&]() {
            float w = dk[0];
#pragma unroll
            for (int t = 1; t < KK; ++t) w = (t == P.K - 1) ? dk[t] : w;
            return valid ? w : -INFINITY;
        };
        // home chunk: where the cell of a query in the middle of the wave starts among the sorted refs
        const Grid g = grid_of(P, b);
        const int nq = min(WAVE, P.P1 - (int)blockIdx.x * WAVE);
        const int cell = cell_of(qx, qy, qz, g);
        const int hcell = __builtin_amdgcn_readlane(cell, min(WAVE / 2, nq - 1));
        const uint32_t hstart = P.start[((size_t)b * 2 + 1) * (CELLS + 1) + hcell];
        const int h = min((int)(hstart / REF_CHUNK), nch - 1);
        visit(h);
        float w = uniform(wave_max(kth()));
        const float4* boxes = P.boxes + (size_t)b * nch * 2;
        const int ng = (nch + WAVE - 1) / WAVE;
        for (int gi = 0, g0 = h / WAVE; gi < ng; ++gi) {
            // 64 chunks at a time, one per lane: bound against the wave's box, a ballot of the chunks under the wave's
            // largest K-th distance
            const int grp = (g0 + gi) % ng;
            const int c = grp * WAVE + lane;
            float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
            float lb = INFINITY;
            const bool cand = c < nch && c != h;
            if (cand) {
                lo = boxes[(size_t)c * 2];
                hi = boxes[(size_t)c * 2 + 1];
                const float gx = fmaxf(fmaxf(lo.x - qhx, qlx - hi.x), 0.f);
                const float gy = fmaxf(fmaxf(lo.y - qhy, qly - hi.y), 0.f);
                const float gz = fmaxf(fmaxf(lo.z - qhz, qlz - hi.z), 0.f);
                lb = ((gx * gx + gy * gy) + gz * gz) * CULL_MARGIN;
            }
            uint64_t m = __ballot(cand && lb <= w);
            while (m) {
                const int l = __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                // then every lane's own query against the chunk's box and its own K-th distance: a wave whose queries
                // lie far apart (its 64 sorted queries straddle a jump of the Morton order) visits what its lanes need,
                // not everything between them
                auto rd = [&](float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); };
                const float gx = fmaxf(fmaxf(rd(lo.x) - qx, qx - rd(hi.x)), 0.f);
                const float gy = fmaxf(fmaxf(rd(lo.y) - qy, qy - rd(hi.y)), 0.f);
                const float gz = fmaxf(fmaxf(rd(lo.z) - qz, qz - rd(hi.z)), 0.f);
                const float lbq = ((gx * gx + gy * gy) + gz * gz) * CULL_MARGIN;
                if (!__ballot(valid && lbq <= kth())) continue;
                visit(grp * WAVE + l);
                w = uniform(wave_max(kth()));
            }
        }
    }

    if (P.wave_refs && lane == 0) P.wave_refs[(size_t)b * gridDim.x + blockIdx.x] = visited;
    if (valid && (uint32_t)qi < (uint32_t)P.P1) {            // qi from the sorted queries: in range by construction
        float* od = P.dists + ((int64_t)b * P.P1 + qi) * P.K;
        int64_t* oi = P.idx + ((int64_t)b * P.P1 + qi) * P.K;
#pragma unroll
        for (int t = 0; t < KK; ++t) {
            if (t < P.K) {
                od[t] = dk[t];
                oi[t] = jk[t];
            }
        }
    }
}

// ---- backward -------------------------------------------------------------------------------------------------------

struct BwdParams {
    int N, P1, P2, K;
    const float* p1;
    const float* p2;
    const int64_t* idx;
    const float* gd;                         // [N, P1, K] or NULL
    const float* gk;                         // [N, P1, K, 3] or NULL
    const int64_t* sorted_idx;               // [N, P1 * K]
    const int64_t* order;                    // [N, P1 * K]
    float* g1;                               // [N, P1, 3]
    float* g2;                               // [N, P2, 3]
};

__global__ void __launch_bounds__(BLOCK) knn_grad_p1(BwdParams P) {
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= (int64_t)P.N * P.P1) return;
    const int64_t b = t / P.P1;
    const float ax = P.p1[t * 3], ay = P.p1[t * 3 + 1], az = P.p1[t * 3 + 2];
    float sx = 0.f, sy = 0.f, sz = 0.f;
    if (P.gd) {
        for (int k = 0; k < P.K; ++k) {
            const int64_t j = P.idx[t * P.K + k];
            if (j < 0 || j >= P.P2) continue;
            const float* r = P.p2 + (b * P.P2 + j) * 3;
            const float g2 = 2.f * P.gd[t * P.K + k];
            sx += g2 * (ax - r[0]);
            sy += g2 * (ay - r[1]);
            sz += g2 * (az - r[2]);
        }
    }
    P.g1[t * 3] = sx;
    P.g1[t * 3 + 1] = sy;
    P.g1[t * 3 + 2] = sz;
}

// one thread per ref: its entries are the run [lo, hi) of its index in sorted_idx, summed in that (stable) order
__global__ void __launch_bounds__(BLOCK) knn_grad_p2(BwdParams P) {
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= (int64_t)P.N * P.P2) return;
    const int64_t b = t / P.P2, j = t % P.P2;
    const int64_t M = (int64_t)P.P1 * P.K;
    const int64_t* si = P.sorted_idx + b * M;
    int64_t lo = 0, hi = M;                                    // first position with si >= j
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (si[mid] < j) lo = mid + 1; else hi = mid;
    }
    const float bx = P.p2[t * 3], by = P.p2[t * 3 + 1], bz = P.p2[t * 3 + 2];
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int64_t s = lo; s < M && si[s] == j; ++s) {
        const int64_t e = P.order[b * M + s];
        if (e < 0 || e >= M) continue;
        if (P.gd) {
            const float* a = P.p1 + (b * P.P1 + e / P.K) * 3;
            const float g2 = -2.f * P.gd[b * M + e];
            sx += g2 * (a[0] - bx);
            sy += g2 * (a[1] - by);
            sz += g2 * (a[2] - bz);
        }
        if (P.gk) {
            const float* gk = P.gk + (b * M + e) * 3;
            sx += gk[0];
            sy += gk[1];
            sz += gk[2];
        }
    }
    P.g2[t * 3] = sx;
    P.g2[t * 3 + 1] = sy;
    P.g2[t * 3 + 2] = sz;
}

// ---- host side ------------------------------------------------------------------------------------------------------

EXA_ABI_STATUS("exa_knn")

int check_shape(int32_t N, int32_t P1, int32_t P2, int32_t K) {
    if (N < 0 || P1 < 0 || P2 < 0) return fail(EXA_KNN_E_INVALID, "negative size");
    if (N > 65535) return fail(EXA_KNN_E_INVALID, "more than 65535 batch elements");
    if (P1 > EXA_KNN_MAX_POINTS || P2 > EXA_KNN_MAX_POINTS) return fail(EXA_KNN_E_INVALID, "more than 2^28 points");
    if (K < 1 || K > EXA_KNN_MAX_K) return fail(EXA_KNN_E_INVALID, "K must be 1 .. 32");
    return 0;
}

// byte offsets of the workspace sections; total 0 when there is nothing to search
struct Layout {
    uint64_t part, cnt1, cnt2, tot, start, s1, s2, boxes, total;
};

Layout layout(int32_t N, int32_t P1, int32_t P2) {
    Layout L;
    memset(&L, 0, sizeof(L));
    if (N == 0 || P1 == 0 || P2 == 0) return L;
    uint64_t o = 0;
    L.part = o;  o += align256((uint64_t)N * NPART * 2 * sizeof(float4));
    L.cnt1 = o;  o += align256((uint64_t)N * sort_chunks(P1) * CELLS * 4);
    L.cnt2 = o;  o += align256((uint64_t)N * sort_chunks(P2) * CELLS * 4);
    L.tot = o;   o += align256((uint64_t)N * 2 * CELLS * 4);
    L.start = o; o += align256((uint64_t)N * 2 * (CELLS + 1) * 4);
    L.s1 = o;    o += align256((uint64_t)N * P1 * sizeof(float4));
    L.s2 = o;    o += align256((uint64_t)N * P2 * sizeof(float4));
    L.boxes = o; o += align256((uint64_t)N * ref_chunks(P2) * 2 * sizeof(float4));
    L.total = o;
    return L;
}

template <int KK>
int launch_search(const Params& P, bool cull, hipStream_t st) {
    const dim3 grid(ceil_div(P.P1, WAVE), P.N);
    if (cull)
        hipLaunchKernelGGL((knn_search<KK, true>), grid, dim3(WAVE), 0, st, P);
    else
        hipLaunchKernelGGL((knn_search<KK, false>), grid, dim3(WAVE), 0, st, P);
    return launched("knn_search");
}

int launch_cull_prep(const Params& P, hipStream_t st) {
    const int maxch = sort_chunks(P.P1 > P.P2 ? P.P1 : P.P2);
    hipLaunchKernelGGL(knn_bbox_part, dim3(NPART, P.N), dim3(BLOCK), 0, st, P);
    if (int rc = launched("knn_bbox_part")) return rc;
    hipLaunchKernelGGL(knn_sort_pass<false>, dim3(maxch, P.N, 2), dim3(SORT_CHUNK), 0, st, P);
    if (int rc = launched("knn_sort_pass (count)")) return rc;
    hipLaunchKernelGGL(knn_col_scan, dim3(CELLS / WAVE, 2, P.N), dim3(SORT_CHUNK), 0, st, P);
    if (int rc = launched("knn_col_scan")) return rc;
    hipLaunchKernelGGL(knn_cell_scan, dim3(2, P.N), dim3(1024), 0, st, P);
    if (int rc = launched("knn_cell_scan")) return rc;
    hipLaunchKernelGGL(knn_sort_pass<true>, dim3(maxch, P.N, 2), dim3(SORT_CHUNK), 0, st, P);
    if (int rc = launched("knn_sort_pass (scatter)")) return rc;
    hipLaunchKernelGGL(knn_boxes, dim3(ceil_div(ref_chunks(P.P2), BLOCK / WAVE), P.N), dim3(BLOCK), 0, st, P);
    return launched("knn_boxes");
}

}  // namespace exa_knn_impl

using namespace exa_knn_impl;

extern "C" {

int exa_knn_version(void) { return EXA_KNN_VERSION; }

const char* exa_knn_last_error(void) { return g_err; }

int exa_knn_workspace_size(int32_t N, int32_t P1, int32_t P2, int32_t K, uint64_t* out_bytes) {
    if (!out_bytes) return fail(EXA_KNN_E_NULLPTR, "out_bytes is NULL");
    if (int rc = check_shape(N, P1, P2, K)) return rc;
    *out_bytes = layout(N, P1, P2).total;
    return 0;
}

int exa_knn_forward(int32_t N, int32_t P1, int32_t P2, int32_t K, const float* p1, const float* p2, uint32_t flags,
                    void* workspace, uint64_t workspace_bytes, float* dists, int64_t* idx, uint32_t* wave_refs,
                    void* stream) {
    if (int rc = check_shape(N, P1, P2, K)) return rc;
    if (flags & ~EXA_KNN_NO_CULL) return fail(EXA_KNN_E_INVALID, "unknown flag bits");
    if (N == 0 || P1 == 0) return 0;
    if (K > P2) return fail(EXA_KNN_E_INVALID, "K is larger than P2");
    if (!p1 || !p2) return fail(EXA_KNN_E_NULLPTR, "p1 / p2 is NULL");
    if (!dists || !idx) return fail(EXA_KNN_E_NULLPTR, "dists / idx is NULL");
    const bool cull = !(flags & EXA_KNN_NO_CULL);
    const Layout L = layout(N, P1, P2);
    if (cull) {
        if (!workspace) return fail(EXA_KNN_E_NULLPTR, "workspace is NULL");
        if (workspace_bytes < L.total) return fail(EXA_KNN_E_INVALID, "workspace is smaller than exa_knn_workspace_size");
    }
    Params P;
    memset(&P, 0, sizeof(P));
    P.N = N; P.P1 = P1; P.P2 = P2; P.K = K;
    P.p1 = p1; P.p2 = p2; P.dists = dists; P.idx = idx; P.wave_refs = wave_refs;
    hipStream_t st = (hipStream_t)stream;
    if (cull) {
        char* ws = (char*)workspace;
        P.part = (float4*)(ws + L.part);
        P.cnt1 = (uint32_t*)(ws + L.cnt1);
        P.cnt2 = (uint32_t*)(ws + L.cnt2);
        P.tot = (uint32_t*)(ws + L.tot);
        P.start = (uint32_t*)(ws + L.start);
        P.s1 = (float4*)(ws + L.s1);
        P.s2 = (float4*)(ws + L.s2);
        P.boxes = (float4*)(ws + L.boxes);
        if (int rc = launch_cull_prep(P, st)) return rc;
    }
    if (K <= 1) return launch_search<1>(P, cull, st);
    if (K <= 2) return launch_search<2>(P, cull, st);
    if (K <= 4) return launch_search<4>(P, cull, st);
    if (K <= 8) return launch_search<8>(P, cull, st);
    if (K <= 16) return launch_search<16>(P, cull, st);
    return launch_search<32>(P, cull, st);
}

int exa_knn_backward(int32_t N, int32_t P1, int32_t P2, int32_t K, const float* p1, const float* p2, const int64_t* idx,
                     const float* grad_dists, const float* grad_knn, const int64_t* sorted_idx, const int64_t* order,
                     float* grad_p1, float* grad_p2, void* stream) {
    if (int rc = check_shape(N, P1, P2, K)) return rc;
    const int64_t n1 = (int64_t)N * P1, n2 = (int64_t)N * P2;
    if (n1 > 0 && P2 == 0) return fail(EXA_KNN_E_INVALID, "queries without refs have no neighbours");
    if ((n1 > 0 && (!p1 || !grad_p1)) || (n2 > 0 && (!p2 || !grad_p2)))
        return fail(EXA_KNN_E_NULLPTR, "p1 / p2 / grad_p1 / grad_p2 is NULL");
    if (n1 > 0 && (!idx || !sorted_idx || !order)) return fail(EXA_KNN_E_NULLPTR, "idx / sorted_idx / order is NULL");
    BwdParams P;
    P.N = N; P.P1 = P1; P.P2 = P2; P.K = K;
    P.p1 = p1; P.p2 = p2; P.idx = idx; P.gd = grad_dists; P.gk = grad_knn;
    P.sorted_idx = sorted_idx; P.order = order; P.g1 = grad_p1; P.g2 = grad_p2;
    hipStream_t st = (hipStream_t)stream;
    if (n1 > 0) {
        hipLaunchKernelGGL(knn_grad_p1, dim3(ceil_div(n1, BLOCK)), dim3(BLOCK), 0, st, P);
        if (int rc = launched("knn_grad_p1")) return rc;
    }
    if (n2 > 0) {
        hipLaunchKernelGGL(knn_grad_p2, dim3(ceil_div(n2, BLOCK)), dim3(BLOCK), 0, st, P);
        if (int rc = launched("knn_grad_p2")) return rc;
    }
    return 0;
}

}  // extern "C"
