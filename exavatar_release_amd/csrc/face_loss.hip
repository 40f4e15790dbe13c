// The face composite of the loss block and the test branch (reference avatar/main/model.py:200-201, 207-208, 268-276):
// the face-composited L1 term forward, its mean and its backward, and the three full-image composites.  The operations and
// every summation order are written out in include/exa_raster.h; this file is compiled with -ffp-contract=off.
//
// All kernels are memory-bound and elementwise.  One thread owns one RUN: the FACE_RUN = 4 consecutive pixels
// x = 4 q .. 4 q + 3 of one image row (q counts from the image's left edge, so a run starts on a 16-byte boundary of its row
// whenever W is a multiple of 4 and the arrays are 16-byte aligned).  It reads the coverage plane once and then walks the C
// colour planes.  A run that lies wholly inside the window is moved with 16-byte loads and stores; the head and the tail of a
// window whose x0 or width is not a multiple of 4, and every run of an image that does not allow 16-byte access, go pixel
// by pixel.  Workgroups are BLOCK = 256 threads (4 waves) on a one-dimensional grid over (image, row, run).
// No atomics; LDS only for the four wave sums of a workgroup sum.
#include "common.h"
#include "fixed_sum.h"
#include "image_checks.h"

namespace exa {

namespace {

constexpr int FACE_RUN = 4;

// Pixels lo <= x + k < hi of the run at x of the row that starts at p; 0 elsewhere.  `full`: the whole run, one 16-byte load.
__device__ __forceinline__ void load_run(const float* p, int x, bool full, int lo, int hi, float (&v)[FACE_RUN]) {
    if (full) {
        const float4 q = *reinterpret_cast<const float4*>(p + x);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < FACE_RUN; ++k) v[k] = (x + k >= lo && x + k < hi) ? p[x + k] : 0.0f;
    }
}

__device__ __forceinline__ void store_run(float* p, int x, bool full, int lo, int hi, const float (&v)[FACE_RUN]) {
    if (full) {
        *reinterpret_cast<float4*>(p + x) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < FACE_RUN; ++k)
            if (x + k >= lo && x + k < hi) p[x + k] = v[k];
    }
}

struct FaceL1Args {
    int C, H, W, cx0, cy0, cw, ch;
    int runs;                 // forward: runs per window row, (cw + 6) / 4; backward: runs per image row, (W + 3) / 4
    unsigned total;           // threads that have a run: B * ch * runs (forward), B * H * runs (backward)
    int vec, map_vec;         // 16-byte access to the [.., H, W] arrays / to the window-shaped array
    const float* img; const float* face; const float* tgt;
    float* map; float* partials;                             // forward
    const float* g_map; const float* g_mean; float n;        // backward: one of the two cotangents; n = (float)n_elements
    float* d_img; float* d_face;
};

__global__ __launch_bounds__(BLOCK) void face_l1_fwd_kernel(FaceL1Args a) {
    const unsigned i = blockIdx.x * BLOCK + threadIdx.x;
    float s = 0.0f;
    const int lo = a.cx0, hi = a.cx0 + a.cw;
    const int x = FACE_RUN * (a.cx0 / FACE_RUN + (int)(i % (unsigned)a.runs));
    if (i < a.total && x < hi) {                             // (the last run of a row may lie behind the window)
        const unsigned r = i / (unsigned)a.runs;
        const int ly = (int)(r % (unsigned)a.ch), b = (int)(r / (unsigned)a.ch);
        const bool full = a.vec && x >= lo && x + FACE_RUN <= hi;
        const size_t plane = (size_t)a.H * a.W, row = (size_t)(a.cy0 + ly) * a.W;
        const float* face = a.face + (size_t)b * (a.C + 1) * plane + row;
        float cov[FACE_RUN];
        load_run(face + a.C * plane, x, full, lo, hi, cov);
        for (int c = 0; c < a.C; ++c) {
            const size_t o = ((size_t)b * a.C + c) * plane + row;
            float fc[FACE_RUN], im[FACE_RUN], tg[FACE_RUN], t[FACE_RUN];
            load_run(face + c * plane, x, full, lo, hi, fc);
            load_run(a.img + o, x, full, lo, hi, im);
            load_run(a.tgt + o, x, full, lo, hi, tg);
#pragma unroll
            for (int k = 0; k < FACE_RUN; ++k) {
                const bool f = fc[k] != -1.0f && cov[k] == 1.0f;
                t[k] = fabsf((f ? fc[k] : im[k]) - tg[k]);
            }
            if (a.map)          // the window's row starts lo pixels into the image's: the same x indexes both
                store_run(a.map + (((size_t)b * a.C + c) * a.ch + ly) * a.cw - lo, x, full && a.map_vec, lo, hi, t);
#pragma unroll
            for (int k = 0; k < FACE_RUN; ++k)
                if (full || (x + k >= lo && x + k < hi)) s = s + t[k];
        }
    }
    if (a.partials) {                                        // (uniform: every thread of the workgroup gets here)
        s = block_sum<BLOCK / 64>(s);
        if (threadIdx.x == 0) a.partials[blockIdx.x] = s;
    }
}

// One workgroup: thread t adds partials t, t + 256, t + 512, .. in that order, then the workgroup sum.
__global__ __launch_bounds__(BLOCK) void face_l1_reduce_kernel(long long n_partials, float n, const float* partials,
                                                               float* out) {
    const float s = block_sum<BLOCK / 64>(strided_sum<BLOCK>(partials, n_partials));
    if (threadIdx.x == 0) *out = s / n;
}

// L1: the backward of the face-composited L1 map.  !L1: the backward of the hard composite, whose window is the image
// (g_map = dL_dout, no target, no sign).  Walks every run of the image; only window pixels read the inputs.
template <bool L1>
__global__ __launch_bounds__(BLOCK) void face_bwd_kernel(FaceL1Args a) {
    const unsigned i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.total) return;
    const int x = FACE_RUN * (int)(i % (unsigned)a.runs);
    const unsigned r = i / (unsigned)a.runs;
    const int y = (int)(r % (unsigned)a.H), b = (int)(r / (unsigned)a.H);
    const bool in_rows = y >= a.cy0 && y < a.cy0 + a.ch;
    const int lo = in_rows ? a.cx0 : 0, hi = in_rows ? a.cx0 + a.cw : 0;      // the window's pixels of this row
    const bool any = x < hi && x + FACE_RUN > lo;
    const bool full = a.vec && x >= lo && x + FACE_RUN <= hi;
    const size_t plane = (size_t)a.H * a.W, row = (size_t)y * a.W;
    const float* face = a.face + (size_t)b * (a.C + 1) * plane + row;
    float k_mean = 0.0f;
    if (L1 && a.g_mean) k_mean = *a.g_mean * (1.0f / a.n);      // torch's `grad / numel` on the device (exa_raster.h)
    float cov[FACE_RUN] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (any) load_run(face + a.C * plane, x, full, lo, hi, cov);
    for (int c = 0; c < a.C; ++c) {
        const size_t o = ((size_t)b * a.C + c) * plane + row;
        float gi[FACE_RUN] = {0.0f, 0.0f, 0.0f, 0.0f}, gf[FACE_RUN] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (any) {
            float fc[FACE_RUN], g[FACE_RUN], im[FACE_RUN], tg[FACE_RUN];
            load_run(face + c * plane, x, full, lo, hi, fc);
            if (L1) {
                load_run(a.img + o, x, full, lo, hi, im);
                load_run(a.tgt + o, x, full, lo, hi, tg);
            }
            if (a.g_map)
                load_run(a.g_map + (((size_t)b * a.C + c) * a.ch + (y - a.cy0)) * a.cw - lo, x, full && a.map_vec, lo, hi, g);
            else
                g[0] = g[1] = g[2] = g[3] = k_mean;
#pragma unroll
            for (int k = 0; k < FACE_RUN; ++k) {
                if (!(full || (x + k >= lo && x + k < hi))) continue;
                const bool f = fc[k] != -1.0f && cov[k] == 1.0f;
                float sg = g[k];
                if (L1) {
                    const float d = (f ? fc[k] : im[k]) - tg[k];
                    sg = ((d > 0.0f ? 1.0f : 0.0f) - (d < 0.0f ? 1.0f : 0.0f)) * g[k];
                }
                gi[k] = f ? 0.0f : sg;
                gf[k] = f ? sg : 0.0f;
            }
        }
        if (a.d_img) store_run(a.d_img + o, x, a.vec, 0, a.W, gi);
        if (a.d_face) store_run(a.d_face + (size_t)b * (a.C + 1) * plane + c * plane + row, x, a.vec, 0, a.W, gf);
    }
    if (a.d_face) {                                          // the coverage plane: `== 1` cuts its gradient
        const float zero[FACE_RUN] = {0.0f, 0.0f, 0.0f, 0.0f};
        store_run(a.d_face + (size_t)b * (a.C + 1) * plane + a.C * plane + row, x, a.vec, 0, a.W, zero);
    }
}

struct CompositeArgs {
    int C, H, W, runs, vec;
    unsigned total;
    const float* a; const float* sel; const float* b; float* out;
    float thr;
};

template <int MODE>
__global__ __launch_bounds__(BLOCK) void composite_fwd_kernel(CompositeArgs p) {
    const unsigned i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= p.total) return;
    const int x = FACE_RUN * (int)(i % (unsigned)p.runs);
    const unsigned r = i / (unsigned)p.runs;
    const int y = (int)(r % (unsigned)p.H), b = (int)(r / (unsigned)p.H);
    const bool full = p.vec != 0;
    const size_t plane = (size_t)p.H * p.W, row = (size_t)y * p.W;
    const int sel_planes = MODE == EXA_COMPOSITE_FOREGROUND ? 1 : p.C + 1;
    const float* sel = p.sel + (size_t)b * sel_planes * plane + row;
    float w[FACE_RUN];                                       // the coverage plane / the mask
    load_run(sel + (sel_planes - 1) * plane, x, full, 0, p.W, w);
    for (int c = 0; c < p.C; ++c) {
        const size_t o = ((size_t)b * p.C + c) * plane + row;
        float u[FACE_RUN], v[FACE_RUN], out[FACE_RUN];
        load_run(p.b + o, x, full, 0, p.W, v);
        if (MODE == EXA_COMPOSITE_FOREGROUND) load_run(p.a + o, x, full, 0, p.W, u);
        else load_run(sel + c * plane, x, full, 0, p.W, u);
#pragma unroll
        for (int k = 0; k < FACE_RUN; ++k) {
            if (MODE == EXA_COMPOSITE_FACE_HARD) {
                out[k] = (u[k] != -1.0f && w[k] == 1.0f) ? u[k] : v[k];
            } else if (MODE == EXA_COMPOSITE_FACE_SOFT) {
                const float wk = (u[k] != -1.0f ? 1.0f : 0.0f) * w[k];
                out[k] = v[k] * (1.0f - wk) + u[k] * wk;
            } else {
                out[k] = w[k] > p.thr ? u[k] : v[k];
            }
        }
        store_run(p.out + o, x, full, 0, p.W, out);
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

}  // namespace exa

// ---- C entry points (include/exa_raster.h): checks, then the launch --------------------------------------------------------
namespace exa_raster_impl {

using namespace exa;

EXA_ABI_STATUS_SHARED("exa_raster")       // exa_raster_last_error() and its buffer are api.hip's

// the runs of a window row: a window of cw > 0 pixels touches at most (cw + 6) / 4 runs of 4 pixels, wherever it starts
static int window_runs(int cw) { return (cw + 6) / FACE_RUN; }

// the workgroups (= partial sums) of the L1 term's forward, and those of a full-image walk
static int64_t face_l1_blocks(int B, int cw, int ch) {
    if (B <= 0 || cw <= 0 || ch <= 0) return 0;
    return ((int64_t)B * ch * window_runs(cw) + BLOCK - 1) / BLOCK;
}

static int64_t face_image_blocks(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return ((int64_t)B * H * ((W + FACE_RUN - 1) / FACE_RUN) + BLOCK - 1) / BLOCK;
}

// the one-dimensional grids index their runs of 4 pixels with 32 bits
static int check_face_runs(int32_t B, int32_t H, int32_t W) {
    if ((int64_t)B * H * ((W + 3) / 4 + 1) > 0x7fffffffLL)
        return fail(EXA_RASTER_E_INVALID, "face loss: more than 2^31 - 1 runs of 4 pixels");
    return 0;
}

// l1 != 0: the L1 term's backward (one of g_map / g_mean); l1 == 0: the hard composite's (g_map = dL_dout, crop = the image)
static int launch_face_bwd(int l1, int B, int C, int H, int W, const int* crop, const float* img, const float* face,
                           const float* tgt, const float* g_map, const float* g_mean, int64_t n_elements, float* d_img,
                           float* d_face, void* stream, const char* where) {
    const int64_t blocks = face_image_blocks(B, H, W);
    if (blocks == 0 || (!d_img && !d_face)) return 0;
    FaceL1Args a = {};
    a.C = C; a.H = H; a.W = W; a.cx0 = crop[0]; a.cy0 = crop[1]; a.cw = crop[2]; a.ch = crop[3];
    a.runs = (W + FACE_RUN - 1) / FACE_RUN;
    a.total = (unsigned)((int64_t)B * H * a.runs);
    a.vec = W % FACE_RUN == 0 && aligned16(face) && aligned16(d_img) && aligned16(d_face) &&
            (!l1 || (aligned16(img) && aligned16(tgt)));
    a.map_vec = a.cw % FACE_RUN == 0 && a.cx0 % FACE_RUN == 0 && aligned16(g_map);
    a.img = img; a.face = face; a.tgt = tgt; a.g_map = g_map; a.g_mean = g_mean; a.n = (float)n_elements;
    a.d_img = d_img; a.d_face = d_face;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (l1) face_bwd_kernel<true><<<(unsigned)blocks, BLOCK, 0, s>>>(a);
    else face_bwd_kernel<false><<<(unsigned)blocks, BLOCK, 0, s>>>(a);
    return launched(where);
}

}  // namespace exa_raster_impl

using namespace exa_raster_impl;

extern "C" {

int64_t exa_face_l1_blocks(int32_t B, int32_t C, int32_t crop_w, int32_t crop_h) {
    if (B < 0 || C <= 0 || crop_w < 0 || crop_h < 0) return 0;
    return face_l1_blocks(B, crop_w, crop_h);
}

int exa_face_l1_forward(int32_t B, int32_t C, int32_t H, int32_t W, const int32_t* crop, const float* img_out,
                        const float* face, const float* img_target, float* l1_map, float* partials, void* stream) {
    int rc = check_crop(B, C, H, W, crop);
    if (rc) return rc;
    if ((rc = check_face_runs(B, H, W))) return rc;
    if ((int64_t)B * C * crop[2] * crop[3] > 0 && (!img_out || !face || !img_target))
        return fail(EXA_RASTER_E_NULLPTR, "face_l1: NULL argument");
    const int64_t blocks = face_l1_blocks(B, crop[2], crop[3]);
    if (blocks == 0 || C == 0 || (!l1_map && !partials)) return 0;
    FaceL1Args a = {};
    a.C = C; a.H = H; a.W = W; a.cx0 = crop[0]; a.cy0 = crop[1]; a.cw = crop[2]; a.ch = crop[3];
    a.runs = window_runs(a.cw);
    a.total = (unsigned)((int64_t)B * a.ch * a.runs);
    a.vec = W % FACE_RUN == 0 && aligned16(img_out) && aligned16(face) && aligned16(img_target);
    a.map_vec = a.cw % FACE_RUN == 0 && a.cx0 % FACE_RUN == 0 && aligned16(l1_map);
    a.img = img_out; a.face = face; a.tgt = img_target; a.map = l1_map; a.partials = partials;
    face_l1_fwd_kernel<<<(unsigned)blocks, BLOCK, 0, static_cast<hipStream_t>(stream)>>>(a);
    return launched("face_l1_fwd");
}

int exa_face_l1_reduce(int64_t n_partials, int64_t n_elements, const float* partials, float* out_mean, void* stream) {
    if (n_partials < 0 || n_elements < 0) return fail(EXA_RASTER_E_INVALID, "negative size");
    if (!out_mean || (n_partials > 0 && !partials)) return fail(EXA_RASTER_E_NULLPTR, "face_l1 reduce: NULL argument");
    face_l1_reduce_kernel<<<1, BLOCK, 0, static_cast<hipStream_t>(stream)>>>((long long)n_partials, (float)n_elements, partials,
                                                                             out_mean);
    return launched("face_l1_reduce");
}

int exa_face_l1_backward(int32_t B, int32_t C, int32_t H, int32_t W, const int32_t* crop, const float* img_out,
                         const float* face, const float* img_target, const float* dL_dmap, const float* dL_dmean,
                         int64_t n_elements, float* dL_dimg, float* dL_dface, void* stream) {
    int rc = check_crop(B, C, H, W, crop);
    if (rc) return rc;
    if ((rc = check_face_runs(B, H, W))) return rc;
    if ((dL_dmap != nullptr) == (dL_dmean != nullptr))
        return fail(EXA_RASTER_E_INVALID, "face_l1 backward: pass exactly one of dL_dmap / dL_dmean");
    if (dL_dmean && n_elements < 0) return fail(EXA_RASTER_E_INVALID, "negative size");
    if ((int64_t)B * crop[2] * crop[3] > 0 && (dL_dimg || dL_dface) && (!img_out || !face || !img_target))
        return fail(EXA_RASTER_E_NULLPTR, "face_l1: NULL argument");
    return launch_face_bwd(1, B, C, H, W, crop, img_out, face, img_target, dL_dmap, dL_dmean, n_elements, dL_dimg, dL_dface,
                           stream, "face_l1_bwd");
}

int exa_composite_forward(int32_t mode, int32_t B, int32_t C, int32_t H, int32_t W, const float* a, const float* sel,
                          const float* b, float* out, float thr, void* stream) {
    if (mode != EXA_COMPOSITE_FACE_HARD && mode != EXA_COMPOSITE_FACE_SOFT && mode != EXA_COMPOSITE_FOREGROUND)
        return fail(EXA_RASTER_E_INVALID, "composite: unknown mode");
    if (B < 0 || C < 0 || H < 0 || W < 0) return fail(EXA_RASTER_E_INVALID, "negative size");
    if (int rc = check_face_runs(B, H, W)) return rc;
    if ((int64_t)B * C * H * W > 0 && (!sel || !b || !out || (mode == EXA_COMPOSITE_FOREGROUND && !a)))
        return fail(EXA_RASTER_E_NULLPTR, "composite: NULL argument");
    const int64_t blocks = face_image_blocks(B, H, W);
    if (blocks == 0 || C == 0) return 0;
    CompositeArgs p = {};
    p.C = C; p.H = H; p.W = W; p.runs = (W + FACE_RUN - 1) / FACE_RUN;
    p.total = (unsigned)((int64_t)B * H * p.runs);
    p.vec = W % FACE_RUN == 0 && aligned16(a) && aligned16(sel) && aligned16(b) && aligned16(out);
    p.a = a; p.sel = sel; p.b = b; p.out = out; p.thr = thr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (mode == EXA_COMPOSITE_FACE_HARD) composite_fwd_kernel<EXA_COMPOSITE_FACE_HARD><<<(unsigned)blocks, BLOCK, 0, s>>>(p);
    else if (mode == EXA_COMPOSITE_FACE_SOFT) composite_fwd_kernel<EXA_COMPOSITE_FACE_SOFT><<<(unsigned)blocks, BLOCK, 0, s>>>(p);
    else composite_fwd_kernel<EXA_COMPOSITE_FOREGROUND><<<(unsigned)blocks, BLOCK, 0, s>>>(p);
    return launched("composite_fwd");
}

int exa_composite_backward(int32_t B, int32_t C, int32_t H, int32_t W, const float* img, const float* face,
                           const float* dL_dout, float* dL_dimg, float* dL_dface, void* stream) {
    (void)img;                                             // the selection is decided by the face render alone
    if (B < 0 || C < 0 || H < 0 || W < 0) return fail(EXA_RASTER_E_INVALID, "negative size");
    if (int rc = check_face_runs(B, H, W)) return rc;
    if ((int64_t)B * H * W > 0 && (dL_dimg || dL_dface) && (!face || !dL_dout))
        return fail(EXA_RASTER_E_NULLPTR, "composite: NULL argument");
    const int32_t crop[4] = {0, 0, W, H};
    return launch_face_bwd(0, B, C, H, W, crop, nullptr, face, nullptr, dL_dout, nullptr, 0, dL_dimg, dL_dface, stream,
                           "composite_bwd");
}

}  // extern "C"
