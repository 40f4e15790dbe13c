/*
 * exa_raster.h -- C ABI of the MI355X-native differentiable 3D-Gaussian rasterizer.
 *
 * This is the drop-in boundary for the one native component on ExAvatar's render path: the
 * third-party CUDA extension `diff_gaussian_rasterization_depth` that the reference imports at
 * avatar/common/nets/module.py:11 and calls at module.py:623-640 (forward) and through autograd
 * from avatar/main/train.py:46 (backward).  Upstream binds three C++ entry points through pybind
 * (`rasterize_gaussians`, `rasterize_gaussians_backward`, `mark_visible`); the functions below are
 * what a ctypes / cffi / pybind stub binds instead.
 *
 * Conventions
 *   - plain C types only: device pointers, sizes, a `hipStream_t` passed as `void*`.
 *   - every pointer marked [dev] is a device pointer owned by the caller (PyTorch's caching
 *     allocator in the Python binding); the library allocates nothing and keeps no state between
 *     calls, so any number of forward contexts may be live before their backward runs
 *     (ExAvatar keeps five, avatar/main/model.py:130-162).
 *   - all floating point is fp32, indices int32/uint32, contiguous row-major tensors with the
 *     shapes the reference passes (module.py:632-640): means3D[P,3], opacities[P,1], scales[P,3],
 *     rotations[P,4] (w,x,y,z), colors_precomp[P,3], shs[P,M,3], cov3D_precomp[P,6].
 *   - work is enqueued on `stream`; no call synchronises the device unless `settings->debug != 0`.
 *   - return value: 0 = ok; < 0 = invalid argument (EXA_RASTER_E_*); > 0 = HIP error code (hipError_t).
 *     Instance-buffer overflow is latched in the device-side header (see exa_raster_forward_render): the launch
 *     calls never synchronise, so they cannot return it; exa_raster_header_status() turns a header that the
 *     caller copied to the host (exa_raster_read_header_async) into EXA_RASTER_E_OVERFLOW.
 *   - `settings->prefiltered` is accepted and IGNORED: upstream uses it only to assert that the caller already
 *     removed the Gaussians behind the near plane; this library culls them itself in every call (the reference
 *     always passes False, module.py:620).
 *   - `settings->scale_modifier`: dL_dscales is the derivative with respect to `scales` itself (chain rule through
 *     mod * scale).  Upstream returns the derivative with respect to (mod * scale), i.e. it omits the factor mod;
 *     the two agree for the reference, which passes 1.0 (module.py:615).  A caller that needs upstream's quirk
 *     divides dL_dscales by scale_modifier.
 */
#ifndef EXA_RASTER_H
#define EXA_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EXA_RASTER_VERSION 139          /* 0.1.3.9: exa_raster_densify_workspace_size / _plan / _move and ExaRasterDensifySegment were added under this number, as exa_raster_adam_step was (new functions only: nothing that existed changed, and tests/test_abi.py pins 139), and so was the host-only query exa_raster_launch_paths; tile_bytes of exa_raster_workspace_sizes grew (launch-order cursors per XCD region, one class code per sub-tile); no signature changed; 0.1.3.8: grad_bytes of exa_raster_workspace_sizes includes the 92 B x P group scratch of summed batches of more than four views; 0.1.3.7: ExaRasterComposeJob.radii_out / is_vis_out; 0.1.3.6: exa_raster_select_row; 0.1.3.5: EXA_RASTER_STAGE_* bits of store_ctx; 0.1.3.4: ExaRasterBackwardJob.used_slots; 0.1.3.3: ExaRasterForwardJob.is_vis, ExaRasterBackwardJob.accumulate; 0.1.3.2: ExaRasterBackwardJob.dL_dcolor_indirect, exa_raster_store_pointers, ExaRasterComposeJob.a_color .. a_bg; 0.1.3.1: composite renders (exa_raster_forward_compose_batch); 0.1.3: header.num_tile_instances, EXA_RASTER_E_OVERFLOW / _E_ALIAS, exa_raster_camera_block,
                                           exa_raster_header_status; 0.1.2: ExaRasterBackwardJob.grad_first; .1: exa_raster_read_header_async */
#define EXA_RASTER_TILE 16              /* 16x16 pixel tiles (upstream BLOCK_X/BLOCK_Y) */

#define EXA_RASTER_E_INVALID (-1)
#define EXA_RASTER_E_NULLPTR (-2)
#define EXA_RASTER_E_WORKSPACE (-3)
#define EXA_RASTER_E_OVERFLOW (-4)      /* instance-buffer overflow: only ever returned by exa_raster_header_status(), which
                                           interprets a header that was copied to the host; the launch calls themselves
                                           never return it (they do not synchronise) */
#define EXA_RASTER_E_ALIAS (-5)         /* two jobs of one batched backward call update the same densification-statistics
                                           arrays (the update is a plain read-modify-write per job) */

/* Mirrors the 12-field `GaussianRasterizationSettings` NamedTuple built at module.py:609-622.
 * The four tensor-valued fields stay on the device (the reference builds them with torch ops on
 * the GPU, module.py:604-608), so no host read-back is needed to fill this struct. */
typedef struct ExaRasterSettings {
    int32_t image_height;
    int32_t image_width;
    float tanfovx;
    float tanfovy;
    const float* bg;          /* [dev] float[3] */
    float scale_modifier;
    const float* viewmatrix;  /* [dev] float[16], row-major of the [4,4] tensor (= world->camera, transposed) */
    const float* projmatrix;  /* [dev] float[16], row-major of view^T @ proj^T */
    int32_t sh_degree;
    const float* campos;      /* [dev] float[3] */
    int32_t prefiltered;
    int32_t debug;            /* != 0: hipStreamSynchronize + error check after every kernel */
} ExaRasterSettings;

/* Byte sizes of the caller-allocated workspaces. */
typedef struct ExaRasterWorkspaceSizes {
    uint64_t geom_bytes;   /* per-Gaussian splat records, 64 B * P                         */
    uint64_t tile_bytes;   /* header, (chunk, cell) count matrix, prefixes, per-sub-tile ranges   */
    uint64_t bin_bytes;    /* keys, sorted ids, cell buckets, batch owners / masks, checkpoints: ~50 B * capacity */
    uint64_t grad_bytes;   /* backward scratch: per-instance partial sums, 40 B * capacity, + 92 B * P (sum of the second
                              group of views of exa_raster_backward_batch(sum_shared = 1) with more than four views) */
} ExaRasterWorkspaceSizes;

/* Device-side header at the start of the tile workspace (readable with a 28-byte D2H copy). */
typedef struct ExaRasterHeader {
    uint32_t num_rendered;   /* instance capacity this call needs: 64 * batch slots (role of upstream's
                                num_rendered: what the caller sizes the bin workspace with)   */
    uint32_t overflow;       /* != 0: num_rendered exceeded the capacity, outputs of this call invalid */
    uint32_t max_tile_list;  /* number of (Gaussian, 64x64 cell) entries                     */
    uint32_t num_visible;    /* V = Gaussians with radius > 0                                */
    uint32_t num_instances;  /* D = (Gaussian, 8x8 sub-tile) instances actually emitted      */
    uint32_t active_cells;   /* 64x64-pixel cells that hold at least one instance            */
    uint32_t num_tile_instances; /* sum over visible Gaussians of the 16x16 tiles of their rect: upstream's
                                num_rendered, the D of the byte model in SURVEY.md 8(d)          */
} ExaRasterHeader;

/* 0 if the header copy `h` (host memory) reports a complete render, EXA_RASTER_E_OVERFLOW if the call needed
 * h->num_rendered instances but was given fewer (its outputs are invalid; re-run it with that capacity). */
int exa_raster_header_status(const ExaRasterHeader* h);

int exa_raster_version(void);

/* Thread-local description of the last non-zero status returned on this thread. */
const char* exa_raster_last_error(void);

/* Sizes for P Gaussians, a W x H image and room for `capacity` tile instances. */
int exa_raster_workspace_sizes(int32_t P, int32_t W, int32_t H, uint64_t capacity,
                               ExaRasterWorkspaceSizes* out);

/*
 * Forward, stage 1 (replaces upstream preprocessCUDA + InclusiveSum): per-Gaussian cull, EWA
 * projection, radius, tile rect, optional SH colour; per-cell instance counts and their prefix.
 * After it completes, the header in `tile_ws` holds num_rendered so the caller can size `bin_ws`
 * (upstream reads the same number back to the host at this point).
 * Exactly one of shs / colors_precomp and one of (scales+rotations) / cov3D_precomp is non-NULL.
 */
int exa_raster_forward_bin(const ExaRasterSettings* settings, int32_t P, int32_t sh_M,
                           const float* means3D, const float* shs, const float* colors_precomp,
                           const float* opacities, const float* scales, const float* rotations,
                           const float* cov3D_precomp,
                           int32_t* radii,          /* [dev] out int32[P] */
                           void* geom_ws, void* tile_ws, void* stream);

/*
 * Forward, stage 2 (replaces duplicateWithKeys + SortPairs + identifyTileRanges + renderCUDA):
 * scatter Gaussians into cell buckets and then sub-tile buckets, depth-sort every bucket in LDS,
 * blend front to back.  (geom_ws is logically const; the call fills one reserved field per record.)
 * If the header's num_rendered > capacity nothing is rendered and header.overflow is set.
 * `store_ctx` != 0 additionally writes what the backward pass needs (per-batch pixel checkpoints,
 * batches entered per sub-tile); pass 0 for inference.
 */
int exa_raster_forward_render(const ExaRasterSettings* settings, int32_t P,
                              const void* geom_ws, void* tile_ws, void* bin_ws, uint64_t capacity,
                              float* out_color,   /* [dev] float[3,H,W] */
                              float* out_depth,   /* [dev] float[1,H,W] */
                              float* out_alpha,   /* [dev] float[1,H,W] */
                              int32_t store_ctx, void* stream);

/* Stage 1 + stage 2 back to back with a fixed capacity: no host round trip, hipGraph-capturable. */
int exa_raster_forward(const ExaRasterSettings* settings, int32_t P, int32_t sh_M,
                       const float* means3D, const float* shs, const float* colors_precomp,
                       const float* opacities, const float* scales, const float* rotations,
                       const float* cov3D_precomp, int32_t* radii,
                       void* geom_ws, void* tile_ws, void* bin_ws, uint64_t capacity,
                       float* out_color, float* out_depth, float* out_alpha,
                       int32_t store_ctx, void* stream);

/*
 * Backward (replaces upstream BACKWARD::render + BACKWARD::preprocess).  Consumes the workspaces
 * a forward call with store_ctx != 0 filled.  dL_ddepth / dL_dalpha may be NULL (= zeros; the
 * ExAvatar training case).  Gradient outputs that do not apply
 * (dL_dsh without shs, dL_dcov3D without cov3D_precomp, ...) may be NULL.  All non-NULL outputs
 * are fully written (zeros for culled Gaussians).  If the forward call overflowed its instance capacity
 * (header.overflow != 0) every gradient of that render is written as zero.
 * dL_dmeans2D[P,3]: (x, y) = dL/dpix * (W/2, H/2), z = 0 -- the densification signal the reference
 * reads at avatar/main/train.py:51.
 */
int exa_raster_backward(const ExaRasterSettings* settings, int32_t P, int32_t sh_M,
                        const float* means3D, const float* shs, const float* colors_precomp,
                        const float* opacities, const float* scales, const float* rotations,
                        const float* cov3D_precomp, const int32_t* radii,
                        const void* geom_ws, const void* tile_ws, const void* bin_ws,
                        uint64_t capacity,        /* the capacity bin_ws was carved with in forward */
                        const float* dL_dcolor,   /* [dev] float[3,H,W] */
                        const float* dL_ddepth,   /* [dev] float[1,H,W] or NULL */
                        const float* dL_dalpha,   /* [dev] float[1,H,W] or NULL */
                        void* grad_ws,
                        float* dL_dmeans2D, float* dL_dmeans3D, float* dL_dcolors, float* dL_dopacity,
                        float* dL_dscales, float* dL_drotations, float* dL_dsh, float* dL_dcov3D,
                        void* stream);

/*
 * Batched entry points: K independent renders ("jobs") per call, ONE kernel launch per pipeline stage for up to
 * eight jobs (larger K is processed in groups of eight).  Two uses on ExAvatar's path:
 *   - the K training views one GPU holds of a view-sharded step (same Gaussian tensors, K cameras; the reference's
 *     per-sample loop avatar/main/model.py:81): exa_raster_backward_batch(..., sum_shared = 1) then returns the SUM
 *     of the K views' gradients in job 0's outputs (dL_dmeans2D stays per view);
 *   - the five same-camera renders of one iteration (scene, human, scene+human, human refined, scene+human refined;
 *     avatar/main/model.py:119-167): five jobs with their own Gaussian tensors, sum_shared = 0.
 * A single 1024x1024 render leaves most of the chip idle in every stage but the blend, so a batch costs far less
 * than K calls.  Results are bit-identical to K single calls (sum_shared: up to the order of the K-term sum).
 * All jobs of one call share `store_ctx`.  Same workspace / ownership / error rules as the single-render calls,
 * which are implemented as a batch of one.
 */
typedef struct ExaRasterForwardJob {
    const ExaRasterSettings* settings;
    int32_t P, sh_M;
    const float* means3D; const float* shs; const float* colors_precomp; const float* opacities;
    const float* scales; const float* rotations; const float* cov3D_precomp;
    int32_t* radii;                 /* [dev] out int32[P]                                              */
    void* geom_ws; void* tile_ws;   /* sized by exa_raster_workspace_sizes(P, W, H, capacity)          */
    void* bin_ws; uint64_t capacity;                     /* ignored by exa_raster_forward_bin_batch    */
    float* out_color; float* out_depth; float* out_alpha; /* ignored by exa_raster_forward_bin_batch   */
    int32_t keep_sorted_keys;       /* != 0: this render will be a SOURCE of a composite (exa_raster_forward_compose_batch):
                                       the sort keeps the sorted 64-bit keys (in place, no extra memory)      */
    /* Optional zero-copy header report (NULL = off): a DEVICE-VISIBLE address of 16 bytes of pinned host memory
     * (exa_raster_host_device_pointer).  As soon as the instance count of this job is known -- in the scatter stage,
     * long before the blend finishes -- ONE thread stores {num_rendered, overflow, num_visible, header_tag} there
     * (system-scope, the tag last).  A caller that polls the tag learns whether the capacity was enough without any
     * runtime call, copy or synchronisation; it works inside a captured hipGraph too (a plain store).  Use a fresh tag
     * (or reset the slot) per call to tell a new report from an old one. */
    void* host_header; uint32_t header_tag;
    /* Optional (NULL = off): [dev] out uint8[P], is_vis[i] = radii[i] > 0, written by the per-Gaussian kernel next to radii --
     * the `is_vis` of the reference's renderer (avatar/common/nets/layer.py: `radius > 0`) without a kernel of its own. */
    uint8_t* is_vis;
} ExaRasterForwardJob;

typedef struct ExaRasterBackwardJob {
    const ExaRasterSettings* settings;
    int32_t P, sh_M;
    const float* means3D; const float* shs; const float* colors_precomp; const float* opacities;
    const float* scales; const float* rotations; const float* cov3D_precomp;
    const int32_t* radii;
    const void* geom_ws; const void* tile_ws; const void* bin_ws; uint64_t capacity;
    const float* dL_dcolor; const float* dL_ddepth; const float* dL_dalpha;
    void* grad_ws;
    float* dL_dmeans2D; float* dL_dmeans3D; float* dL_dcolors; float* dL_dopacity;
    float* dL_dscales; float* dL_drotations; float* dL_dsh; float* dL_dcov3D;
    /* optional fused densification statistics (all three NULL = off): updated in place by the per-Gaussian backward
     * kernel exactly as exa_raster_densify_stats would do it with this job's dL_dmeans2D and radii -- no extra pass.
     * The update is a plain read-modify-write: two jobs of one batched call must not name the same array
     * (EXA_RASTER_E_ALIAS), with one exception -- sum_shared = 1 and the SAME three arrays in all K jobs: the K views'
     * statistics are then summed inside the kernel and written once per Gaussian. */
    float* densify_grad_accum; float* densify_track_cnt; float* densify_radius_max;
    /* Constant prefix: Gaussians 0 .. grad_first - 1 are inputs only, they get no gradient.  This is the scene under
     * the human in ExAvatar's composite renders (torch.cat((scene.detach(), human)), avatar/main/model.py:119-126): the
     * backward skips every 64-entry batch that blended no trainable Gaussian, writes no partial record for a constant one
     * and runs no per-Gaussian chain rule for it.  With grad_first > 0 EVERY gradient array above (dL_dmeans2D ...
     * dL_dcov3D, densify_*) holds P - grad_first rows: row r belongs to Gaussian grad_first + r.  0 = all trainable.
     * Not combinable with sum_shared. */
    int32_t grad_first;
    /* Composite render (exa_raster_forward_compose_batch): compose_geom_a != NULL makes this the backward of a composite.
     * Then P, the input tensors, radii and every gradient array describe source B (the trainable Gaussians), geom_ws is B's
     * splat workspace, tile_ws / bin_ws / capacity are the COMPOSITE's workspaces, grad_ws holds exa_raster_compose_sizes().grad_bytes (40 B x compose_capacity_b),
     * compose_geom_a / compose_P_a name source A's records (constants: no gradient) and grad_first must be 0. */
    const void* compose_geom_a; int32_t compose_P_a; uint64_t compose_capacity_b;
    /* Optional (NULL = off): DEVICE address of one pointer that the kernels load at EXECUTION time and read dL/dcolor from,
     * instead of `dL_dcolor` (which must still be non-NULL: it says that a colour gradient exists).  For callers that
     * replay this call from a captured hipGraph while the gradient arrives in a different tensor every time (autograd
     * hands `backward` a fresh one per iteration): exa_raster_store_pointers, enqueued on the same stream ahead of the
     * replay, points the call at it -- no 12-byte-per-pixel copy into a static buffer (GraphedIteration). */
    const float* const* dL_dcolor_indirect;
    /* != 0: dL_dmeans3D, dL_dcolors, dL_dsh, dL_dopacity, dL_dscales, dL_drotations and dL_dcov3D already HOLD gradients
     * (of another render of the same Gaussians, e.g. the composite that shows them over the scene) and this call ADDS its
     * own to them: out = held + this render's, one read more per value and no separate summation pass.  dL_dmeans2D is
     * per render and always overwritten.  Not combinable with sum_shared. */
    int32_t accumulate;
    /* Optional (0 = capacity / 64): how many 64-instance batch slots of the instance buffer the forward call actually used =
     * ceil(header.num_rendered / 64), which a caller that has seen the header (or its zero-copy report) knows by now.  The
     * backward blend launches one wave per batch slot; with a buffer sized generously (capacity = 1.5 x an earlier need, or
     * capacity_a + capacity_b for a composite, whose packed lists typically fill a fifth of that) most of those waves only
     * find out that their slot is past the end -- tens of thousands of dispatches (~0.24 ns each chip-wide, 24 us per
     * five-render iteration for the two composites).  A value below the true count would skip batches: pass only what the
     * header of THIS forward call said. */
    uint32_t used_slots;
} ExaRasterBackwardJob;

/* A schedule of per-frame parameter blocks that is RESIDENT on the device -- the ring of cameras of a turntable animation
 * (avatar/main/animate_view_rot.py:104 computes all of them up front), the views of a benchmark -- stepped through without any
 * host-side work per frame: one 64-lane launch copies row (*counter mod n_rows) of `table` [n_rows x row_floats] to `dst` and
 * advances the counter (device int32).  Capturable: as the first node of a hipGraph every replay renders the next row
 * (a camera block as exa_raster_camera_block writes it: viewmatrix 16 | projmatrix 16 | campos 3 floats), where an eager copy
 * kernel in front of the replay costs ~4.5 us of GPU time per frame (system-scope fences around a launch outside the graph). */
int exa_raster_select_row(const float* table, int32_t n_rows, int32_t row_floats, int32_t* counter, float* dst, void* stream);

/* Stores `n` (<= 16) pointers into `table` (device memory) with one tiny kernel, in stream order. */
int exa_raster_store_pointers(void* table, const void* const* ptrs, int32_t n, void* stream);

/*
 * Composite renders: "A and B rendered together" from two renders of the SAME camera and image size that already exist,
 * without preprocessing, binning or sorting anything again -- the sorted list of every sub-tile is the merge of the two
 * sources' sorted lists (order of the concatenation cat(A, B): ascending depth, ties by index, so A wins ties).
 * This is what ExAvatar's scene + human renders are (torch.cat((scene.detach(), human)), avatar/main/model.py:119-126,
 * next to plain renders of `scene` and `human` in the same iteration).  A is a constant of the backward
 * pass (the detached scene), B is trainable.  Results are bit-identical to rendering the concatenation.
 * Both sources must be finished forward calls on the same stream with keep_sorted_keys != 0 whose workspaces are still
 * alive; the composite owns tile_ws / bin_ws (exa_raster_compose_sizes) and its output images.  radii of the composite =
 * the sources' radii, A's first.
 */
typedef struct ExaRasterComposeJob {
    const ExaRasterSettings* settings;          /* image size as the sources'; bg of the composite                      */
    int32_t P_a, P_b;
    const void* geom_a; const void* tile_a; const void* bin_a; uint64_t capacity_a;
    const void* geom_b; const void* tile_b; const void* bin_b; uint64_t capacity_b;
    void* tile_ws; void* bin_ws; uint64_t capacity;      /* capacity_a + capacity_b always suffices                     */
    float* out_color; float* out_depth; float* out_alpha;
    void* host_header; uint32_t header_tag;             /* as in ExaRasterForwardJob                                    */
    /* Optional (all four NULL = off): source A's OWN finished output images and the background pointer it was rendered with.
     * Where B has no entry in a sub-tile, the composite's pixels ARE A's pixels -- same list, same arithmetic -- provided
     * the two backgrounds hold equal values (compared on the device): such sub-tiles then get an EMPTY list in the
     * composite (no merge, no batch slots, no backward waves) and their 64 pixels are copied from A's images instead of
     * being blended again.  In ExAvatar's scene + human composites (avatar/main/model.py:129,146: both on the default white
     * background) that is every sub-tile outside the person: ~3/4 of the image.  Bit-identical either way. */
    const float* a_color; const float* a_depth; const float* a_alpha; const float* a_bg;
    /* Optional (radii_out / is_vis_out NULL = off): the composite's radii [P_a + P_b] and is_vis [P_a + P_b] = the sources'
     * arrays one behind the other -- what a render of cat(A, B) returns (reference module.py:641-647) -- copied by the
     * workgroups of the ranges launch that zero-fill the workspace anyway: no launch of their own. */
    const int32_t* radii_a; const int32_t* radii_b; int32_t* radii_out;
    const uint8_t* is_vis_a; const uint8_t* is_vis_b; uint8_t* is_vis_out;
} ExaRasterComposeJob;
/* tile_bytes / bin_bytes of a composite's workspaces, grad_bytes of its backward scratch (geom_bytes = 0) */
int exa_raster_compose_sizes(int32_t W, int32_t H, uint64_t capacity, uint64_t capacity_b, ExaRasterWorkspaceSizes* out);
int exa_raster_forward_compose_batch(const ExaRasterComposeJob* jobs, int32_t K, int32_t store_ctx, void* stream);

/*
 * Which launches a render of `width` x `height` pixels and P Gaussians takes -- host-only: it launches nothing, needs no
 * device and reads the developer knobs (EXA_FOOTPRINT, EXA_BIN_SINGLE_CELLS, EXA_SORT_SPLIT_SUBTILES) exactly as the launchers
 * do, because it asks the very predicates they ask.  `fused` != 0: one call does stage 1 + 2 (exa_raster_forward /
 * exa_raster_forward_batch); 0: the two-stage protocol (exa_raster_forward_bin, then _render), which never merges the scans.
 * For a batch every job's size has to allow the merge, and the binning / sort paths follow the largest job.
 *   SCANS_MERGED    cell_scatter_kernel scans the (chunk, cell) count matrix itself; otherwise col_scan + cell_scan launches
 *   WALK_TWO_CELLS  that merged scan walks two cells per thread (even cell counts); only ever set with SCANS_MERGED
 *   MASK_READY      cell_scatter_kernel hands its entries over with their footprint masks; otherwise subtile_count_kernel
 *                   (or the one-workgroup-per-cell kernel) computes them
 *   MULTI_PART      sub-tile binning in two launches of several workgroups per cell; otherwise one workgroup per cell
 *   SPLIT_SORT      the short sub-tile lists are sorted by a launch of their own
 *   bits 16 .. 31   trips of the composite's range scan over the cells = ceil(cells / 256) (0 for an empty image)
 * Sizes the render calls refuse (more than 4096 cells, a side above 32768, P above 2^26 - 4) are refused here too.
 */
#define EXA_RASTER_PATH_SCANS_MERGED   1u
#define EXA_RASTER_PATH_WALK_TWO_CELLS 2u
#define EXA_RASTER_PATH_MASK_READY     4u
#define EXA_RASTER_PATH_MULTI_PART     8u
#define EXA_RASTER_PATH_SPLIT_SORT     16u
#define EXA_RASTER_PATH_COMPOSE_TRIPS_SHIFT 16
int exa_raster_launch_paths(int32_t width, int32_t height, int32_t P, int32_t fused, uint32_t* bits_out);

/* `store_ctx` of exa_raster_forward_batch / exa_raster_forward_render_batch / exa_raster_forward_compose_batch: bit 0 = keep the
 * backward context (any caller that passes 0 / 1 is unaffected); the two stage bits split one call into two calls with the
 * SAME job array, so that the caller can put other work between the sorted lists and the blend -- e.g. run the list merges of
 * composite renders (which need their sources' sorted lists, not their images) on a second stream while the sources blend:
 *   ..._STAGE_NO_BLEND    everything up to the sorted per-sub-tile lists (composite: ranges + merged lists), no blend
 *   ..._STAGE_BLEND_ONLY  only the blend, on the lists an earlier NO_BLEND call with these jobs left in the workspaces
 * exa_raster_backward_batch takes the same two bits in its `sum_shared` argument (bit 0 = sum_shared): BLEND_ONLY = the blend's
 * backward (per-instance partial sums) without the per-Gaussian chain rule, NO_BLEND = only the chain rule, on the partial sums
 * an earlier BLEND_ONLY call with these jobs left in grad_ws -- e.g. to let the blend's backward of one batch overlap another
 * batch's on a second stream before a chain rule that adds to that batch's outputs (`accumulate`). */
#define EXA_RASTER_STORE_CTX        1
#define EXA_RASTER_STAGE_NO_BLEND   2
#define EXA_RASTER_STAGE_BLEND_ONLY 4
/* one more cut, in front of the sort (composite: in front of the list merges, which need the sources' sorted lists -- the
 * ranges before them only need the sources' binning): NO_SORT = everything before it, SORT_ONLY = only the sort / the merges */
#define EXA_RASTER_STAGE_NO_SORT    8
#define EXA_RASTER_STAGE_SORT_ONLY  16

int exa_raster_forward_bin_batch(const ExaRasterForwardJob* jobs, int32_t K, void* stream);
int exa_raster_forward_render_batch(const ExaRasterForwardJob* jobs, int32_t K, int32_t store_ctx, void* stream);
int exa_raster_forward_batch(const ExaRasterForwardJob* jobs, int32_t K, int32_t store_ctx, void* stream);
int exa_raster_backward_batch(const ExaRasterBackwardJob* jobs, int32_t K, int32_t sum_shared, void* stream);

/*
 * Asynchronous read-back of the first 16 bytes of the header (num_rendered, overflow, max_tile_list, num_visible) of a
 * tile workspace into caller-provided PINNED host memory (exa_raster_read_header_full_async: all sizeof(ExaRasterHeader)
 * = 28 bytes, dst needs 32), enqueued on `stream` behind the forward call: what a binding
 * does after a fused exa_raster_forward to learn -- later, without a host synchronisation now -- whether the capacity
 * was enough.  One runtime call instead of a slice + view + copy through the tensor library (~20 us of host time per
 * render in an eager training loop).  Not capturable in a hipGraph (a memcpy node): callers skip it under capture.
 */
int exa_raster_read_header_async(const void* tile_ws, void* host_dst16, void* stream);
int exa_raster_read_header_full_async(const void* tile_ws, void* host_dst32, void* stream);
/* Device-visible address of pinned (page-locked, host-coherent) memory at `host_ptr`, for ExaRasterForwardJob.host_header. */
int exa_raster_host_device_pointer(void* host_ptr, void** device_ptr_out);

/*
 * Camera block of GaussianRenderer.forward (module.py:604-608) from DEVICE-resident extrinsics: for R [dev float[9],
 * row-major 3x3] and t [dev float[3]] writes viewmatrix = [[R, t], [0, 0, 0, 1]]^T (row-major [4,4]), projmatrix =
 * viewmatrix @ proj^T and campos = -R^T t, the three device tensors ExaRasterSettings points at.  proj16_host = the
 * [4,4] of get_proj_matrix (transforms.py:43-64; a function of focal length and image size only) in HOST memory,
 * row-major, read during the call.  One tiny launch: a new camera per animation frame costs no read-back, no host
 * matrix code and no upload (hipGraph-capturable).
 * Optional focal-length check (both NULL = off): proj16_host and the tan(fov) of ExaRasterSettings were derived from a
 * focal length the caller remembers (fx_expected, fy_expected); `focal` = this frame's [dev float[2]].  The kernel
 * compares them and stores {equal ? 1 : 0, 0, 0, flag_tag} into the 16 bytes at `host_flag` (a device-visible address of
 * pinned host memory, exa_raster_host_device_pointer) -- a caller that is handed a fresh focal tensor with every frame
 * (a data loader) learns about a zoom without ever reading the tensor back.
 */
int exa_raster_camera_block(const float* R, const float* t, const float* proj16_host, float* viewmatrix_out,
                            float* projmatrix_out, float* campos_out, const float* focal, float fx_expected,
                            float fy_expected, void* host_flag, uint32_t flag_tag, void* stream);

/* upstream markVisible: present[i] = (view-space z of means3D[i] > 0.2). */
int exa_raster_mark_visible(const ExaRasterSettings* settings, int32_t P, const float* means3D,
                            uint8_t* present, void* stream);

/*
 * Fused densification statistics.  Replaces the PyTorch bookkeeping the reference runs after
 * every backward on the scene Gaussians -- avatar/main/train.py:49-54 (stack mean_2d.grad),
 * avatar/main/model.py:279-285 (radius_max), avatar/common/nets/module.py:155-157 (track_stats) -- whose
 * boolean-mask indexing costs a host synchronisation per statement.  For every Gaussian i with radii[i] > 0:
 *     xyz_grad_accum[i] += sqrt(g.x^2 + g.y^2)   with g = dL_dmeans2D[i] (the NDC-scaled screen gradient)
 *     track_cnt[i]      += 1
 *     radius_max[i]      = max(radius_max[i], (float)radii[i])
 * All arrays are device pointers of P elements ([P,3] for dL_dmeans2D); any of the three outputs may be NULL.
 * The same update can ride along in the backward pass itself (ExaRasterBackwardJob.densify_*): the screen-space gradient
 * is in registers there, so the statistics cost no extra P-sized pass.
 */
int exa_raster_densify_stats(int32_t P, const float* dL_dmeans2D, const int32_t* radii,
                             float* xyz_grad_accum, float* track_cnt, float* radius_max, void* stream);

/*
 * The scene-Gaussian stage: SceneGaussian.forward (reference avatar/common/nets/module.py:253-272) in one launch each
 * way -- what turns the scene's parameters into the asset dict the rasterizer takes, per sample.  All arrays [dev],
 * fp32, contiguous: mean [P,3], opacity [P,1] (logits), scale [P,3] (logs), rotation [P,6], feature_dc [P,1,3],
 * feature_rest [P,Mr,3] with Mr in {0, 3, 8, 15} (NULL when Mr = 0), cam_R [3,3], cam_t [3].  sh_degree is 0 .. 3 with
 * (sh_degree + 1)^2 <= 1 + Mr.  `mean` passes through untouched (the asset's mean_3d is the caller's own array).
 * Every line is one rounded fp32 operation, never fused, sums in the order written; only + - * / sqrt occur outside the
 * two activations, so a float32 restatement on a CPU gives the same bits.  With eps = 1e-12:
 *   opacity_out [P,1] = 1 / (1 + expf(-opacity));  scale_out [P,3] = expf(scale).
 *   rotation_out [P,4], quaternion (w, x, y, z), with a1 = rotation[0:3], a2 = rotation[3:6]:
 *     n1 = sqrt((a1x a1x + a1y a1y) + a1z a1z), b1 = a1 / max(n1, eps);  dot = (b1x a2x + b1y a2y) + b1z a2z;
 *     c = a2 - dot b1;  n2 = |c| likewise, b2 = c / max(n2, eps);
 *     b3 = (b1y b2z - b1z b2y, b1z b2x - b1x b2z, b1x b2y - b1y b2x);  m = rows (b1, b2, b3).
 *     x0 = ((1 + m00) + m11) + m22, x1 = ((1 + m00) - m11) - m22, x2 = ((1 - m00) + m11) - m22,
 *     x3 = ((1 - m00) - m11) + m22;  i = the first index of their maximum;  q = sqrt(x_i), D = 2 q.
 *     With A = m21 - m12, B = m02 - m20, C = m10 - m01, E = m10 + m01, F = m02 + m20, G = m12 + m21:
 *       row_0 = (q q, A, B, C), row_1 = (A, q q, E, F), row_2 = (B, E, q q, G), row_3 = (C, F, G, q q);
 *     out = row_i / D, negated when out[0] < 0.
 *     The four x sum to 4, so the selected one is >= 1: the 0.1 floor under q and the positive-part branch of the
 *     square root in pytorch3d's matrix_to_quaternion can never bind for the selected candidate and are not carried.
 *     A zero row gives (0.5, 0, 0, 0); (0, 1, 0, 0, 0, 1) is a four-way tie and gives (0.5, -0.5, -0.5, -0.5).
 *   rgb [P,3]:
 *     cam_pos = inverse(cam_R) (-cam_t) by cofactors, on the device (one lane per workgroup): c_ij the cofactors of
 *     cam_R, each `p q - r s`, det = (R00 c00 + R01 c01) + R02 c02,
 *     cam_pos_i = ((c_0i / det) (-t0) + (c_1i / det) (-t1)) + (c_2i / det) (-t2).
 *     v = mean - cam_pos, n = sqrt((vx vx + vy vy) + vz vz), (x, y, z) = v / max(n, eps).
 *     Per channel, with sh_0 = feature_dc and sh_k = feature_rest[k - 1]: the polynomial of the reference's eval_sh
 *     (avatar/common/utils/transforms.py:112-155) in its term order and association,
 *       res = C0 sh_0;  res = res - b1 sh_1;  res = res + b2 sh_2;  res = res - b3 sh_3;  res = res + b_k sh_k, k = 4 ..
 *     with b1 = C1 y, b2 = C1 z, b3 = C1 x, b4 = C2[0] (x y), b5 = C2[1] (y z), b6 = C2[2] ((2 zz - xx) - yy),
 *     b7 = C2[3] (x z), b8 = C2[4] (xx - yy), b9 = (C3[0] y) (3 xx - yy), b10 = (C3[1] (x y)) z,
 *     b11 = (C3[2] y) ((4 zz - xx) - yy), b12 = (C3[3] z) ((2 zz - 3 xx) - 3 yy), b13 = (C3[4] x) ((4 zz - xx) - yy),
 *     b14 = (C3[5] z) (xx - yy), b15 = (C3[6] x) (xx - 3 yy);  u = res + 0.5;  rgb = u < 0 ? 0 : u.
 * exa_raster_scene_assets_backward: one launch, no atomics (nothing is summed across Gaussians), the same bits for the
 * same inputs.  A NULL cotangent (grad_*_out, grad_rgb) counts as zero; a NULL gradient is not computed; every
 * element of every requested gradient is written, zeros included (the rows of grad_feature_rest above the active
 * degree get exactly +0), so the arrays may arrive uninitialised.
 *   grad_opacity = (g (1 - y)) y and grad_scale = g y from the saved outputs y.
 *   out = v / max(n, eps) backward, used three times (a1, c, the view direction), for a cotangent g:
 *     s = (g0 v0 + g1 v1) + g2 v2;  gd = -(s / (d d)), d = max(n, eps);  gn = n >= eps ? gd : 0;
 *     k = n > 0 ? gn / n : 0;  gv_j = g_j / d + v_j k        (torch's clamp_min and norm conventions).
 *   grad_rotation: no gradient through i or the sign.  gs = the cotangent, negated where out was;  gr_j = gs_j / D;
 *     S = ((gs0 row0 + gs1 row1) + gs2 row2) + gs3 row3;  gD = -(S / (D D));  gq = 2 gD + (gr_i 2) q;  gx = gq / D;
 *     dL/dm00, dL/dm11, dL/dm22 = +-gx by x_i's signs; dL/dm21 = gA + gG, dL/dm12 = gG - gA, dL/dm02 = gB + gF,
 *     dL/dm20 = gF - gB, dL/dm10 = gC + gE, dL/dm01 = gE - gC with gA .. gG the gr_j of row_i's entries (0 if absent);
 *     gb1 = gb1 + b2 x gb3, gb2 = gb2 + gb3 x b1 (each component `cur + (p q - r s)`);  gc = backward of b2 at gb2;
 *     gdot = -((gc0 b1x + gc1 b1y) + gc2 b1z);  gb1_j = (gb1_j - dot gc_j) + gdot a2_j;  grad a2_j = gc_j + gdot b1_j;
 *     grad a1 = backward of b1 at gb1.  A zero row gets finite values (of order 1 / eps), as torch gives.
 *   The colour: gm = grad_rgb where u >= 0, else 0 (clamp_min passes the gradient at equality).
 *     grad_feature_dc = C0 gm;  grad sh_k = b_k gm, negated for k = 1, 3;
 *     w_k = (gm_r sh_k,r + gm_g sh_k,g) + gm_b sh_k,b, negated for k = 1, 3;  dL/d(x, y, z) = the sum over k of
 *     w_k d b_k / d(x, y, z) in ascending k (csrc/scene_assets.hip writes the derivative terms out);
 *     grad_mean = backward of the view direction at that -- the view-direction term only: what reaches mean_3d itself
 *     is the caller's (autograd's) to add.
 * A negative P, an Mr or sh_degree outside the above: EXA_RASTER_E_INVALID before any device call.
 */
int exa_raster_scene_assets_forward(int32_t P, int32_t Mr, int32_t sh_degree, const float* mean, const float* opacity,
                                    const float* scale, const float* rotation, const float* feature_dc,
                                    const float* feature_rest, const float* cam_R, const float* cam_t,
                                    float* opacity_out, float* scale_out, float* rotation_out, float* rgb,
                                    void* stream);
int exa_raster_scene_assets_backward(int32_t P, int32_t Mr, int32_t sh_degree, const float* mean, const float* rotation,
                                     const float* feature_dc, const float* feature_rest, const float* cam_R,
                                     const float* cam_t, const float* opacity_out, const float* scale_out,
                                     const float* grad_opacity_out, const float* grad_scale_out,
                                     const float* grad_rotation_out, const float* grad_rgb, float* grad_mean,
                                     float* grad_opacity, float* grad_scale, float* grad_rotation,
                                     float* grad_feature_dc, float* grad_feature_rest, void* stream);

/*
 * Fused SSIM map (the image-loss gradient producer in front of the rasterizer's backward).
 * Replaces class SSIM of reference avatar/common/nets/loss.py:31-74 -- five grouped 11x11 conv2d (Gaussian window,
 * sigma 1.5, zero padding 5) + elementwise ops + their autograd graph -- for N = batch * channels planes of H x W
 * floats.  forward writes ssim_map and, when the three dm_* pointers are non-NULL, the partial derivatives of
 * the map w.r.t. (mu1, E[x^2], E[x y]) that backward consumes; backward writes dL/d(img1) (the rendered image;
 * the target gets no gradient).  The mask / bbox options of the reference are plain tensor ops in the Python mirror
 * (exavatar_release_amd/losses.py).
 */
int exa_ssim_forward(int32_t N, int32_t H, int32_t W, const float* img1, const float* img2, float* ssim_map,
                     float* dm_dmu1, float* dm_dE11, float* dm_dE12, void* stream);
int exa_ssim_backward(int32_t N, int32_t H, int32_t W, const float* img1, const float* img2, const float* dL_dmap,
                      const float* dm_dmu1, const float* dm_dE11, const float* dm_dE12, float* dL_dimg1,
                      void* stream);

/*
 * Fused photometric loss of one render: the weighted L1 + (1 - SSIM) objective the reference builds from
 * class RGBLoss and class SSIM (avatar/common/nets/loss.py:11-74) at avatar/main/model.py:197-198, 204-205, 214-215
 *     loss = w_l1 * mean(l1_weight * |x - y|) + w_ssim * mean(1 - ssim(x * ssim_mask, y * ssim_mask))
 * over the crop window `crop` = {x0, y0, w, h} (the clamped bbox; the SSIM convolutions zero-pad at ITS border, as the
 * reference crops first, loss.py:50-58).  img_out / img_target: [B, C, H, W]; l1_weight, ssim_mask: [B, 1, H, W] or NULL.
 *   exa_photo_loss_forward  one kernel: SSIM statistics, the three partial-derivative maps (maps_ws: 3 * B * C * w * h
 *       floats) and per-workgroup partial sums (partials: 2 floats x exa_photo_loss_blocks(): sum of the SSIM map, sum
 *       of l1_weight |x - y|; the caller adds them up and forms the loss value).
 *   exa_photo_loss_grad     one kernel: dL/d(img_out) inside the crop window (the caller zero-fills dL_dimg outside it),
 *       ready to be handed to exa_raster_backward as dL_dcolor.
 * exa_l1_forward / exa_l1_backward: the L1 map of RGBLoss alone -- |x - t| over the crop with t = y * mask + (1 - mask) * bg
 * when mask [B,1,H,W] and bg [B,C] are given (loss.py:15-17) -- and sign(x - t) * dL_dmap.
 */
int64_t exa_photo_loss_blocks(int32_t B, int32_t C, int32_t crop_w, int32_t crop_h);
int exa_photo_loss_forward(int32_t B, int32_t C, int32_t H, int32_t W, const int32_t* crop, const float* img_out,
                           const float* img_target, const float* l1_weight, const float* ssim_mask, float* maps_ws,
                           float* partials, void* stream);
int exa_photo_loss_grad(int32_t B, int32_t C, int32_t H, int32_t W, const int32_t* crop, const float* img_out,
                        const float* img_target, const float* l1_weight, const float* ssim_mask, float w_l1, float w_ssim,
                        const float* maps_ws, float* dL_dimg, void* stream);
int exa_l1_forward(int32_t B, int32_t C, int32_t H, int32_t W, const int32_t* crop, const float* img_out,
                   const float* img_target, const float* mask, const float* bg, float* l1_map, void* stream);
int exa_l1_backward(int32_t B, int32_t C, int32_t H, int32_t W, const int32_t* crop, const float* img_out,
                    const float* img_target, const float* mask, const float* bg, const float* dL_dmap, float* dL_dimg,
                    void* stream);

/*
 * The face composite in front of the L1 term and the composites of the test branch (csrc/face_loss.hip): reference
 * avatar/main/model.py:200-201, 207-208 (`is_face = ((face[:, :3] != -1) * (face[:, 3:] == 1)).float()`,
 * `rgb_loss(img * (1 - is_face) + face[:, :3] * is_face, target, bbox)`) and model.py:268-276.
 * img_out, img_target: [B, C, H, W]; face: [B, C + 1, H, W], C colour planes and one coverage plane (the face render of
 * exa_mesh_forward: -1 in every channel of a background pixel); crop = {x0, y0, w, h}, the clamped bbox, as for
 * exa_l1_forward.  All arithmetic is fp32, one rounding per operation written, no fused multiply-adds.
 *
 * Work split of every kernel: one thread owns one RUN, the 4 consecutive pixels x = 4 q .. 4 q + 3 of one image row (q counts
 * from the image's left edge), reads the coverage plane once and walks the C colour planes.  A run wholly inside the
 * window moves with 16-byte loads and stores when W is a multiple of 4 and the arrays are 16-byte aligned (the window-shaped
 * arrays l1_map / dL_dmap: when x0 and w are multiples of 4 as well); every other pixel moves by itself.  Workgroups of
 * 256 threads on a one-dimensional grid; thread index i = (b * rows + row) * runs + run.  No atomics anywhere.
 *
 * exa_face_l1_forward: rows = h, runs = (w + 6) / 4 (the runs a window of w pixels can touch, wherever it starts; run r of
 *   a window row is q = x0 / 4 + r, and a last run behind the window holds nothing), grid = exa_face_l1_blocks().
 *   Per window pixel and channel c:  f = (face_c != -1) && (coverage == 1);  v = f ? face_c : img_out_c;
 *   t = |v - img_target_c|.  l1_map ([B, C, h, w], or NULL) receives t.  partials (or NULL) receives one float per
 *   workgroup, the sum of the workgroup's t in this order:
 *     thread:     s = 0; for c = 0 .. C - 1: for k = 0 .. 3: if pixel 4 q + k is in the window: s = s + t   (4 C additions)
 *     wave:       for distance = 32, 16, 8, 4, 2, 1: s = s + s[lane ^ distance]                              (6 additions)
 *     workgroup:  ((wave 0 + wave 1) + wave 2) + wave 3                                                      (3 additions)
 *   Threads without a run or a window pixel enter with s = 0.
 * exa_face_l1_blocks: the number of partials, ceil(B * h * ((w + 6) / 4) / 256); 0 for an empty window, B or C.
 * exa_face_l1_reduce: ONE workgroup of 256 threads.  Thread j adds partials j, j + 256, j + 512, .. in that order to
 *   s = 0 (ceil(n_partials / 256) additions), then the wave and workgroup sums above (9 additions), and thread 0 writes
 *   out_mean = sum / (float)n_elements (n_elements = 0: NaN, as torch.mean of an empty map).  The mean is therefore two
 *   launches and the same bits on every call; an element passes through at most
 *   4 C + 9 + ceil(n_partials / 256) + 9 additions.
 * exa_face_l1_backward: rows = H, runs = ceil(W / 4): the launch walks the whole image.  Exactly one of dL_dmap
 *   ([B, C, h, w]) and dL_dmean is non-NULL; dL_dmean is a DEVICE pointer to one float, read on the device as
 *   g = *dL_dmean * (1 / (float)n_elements), the quotient rounded and then the product (no host read-back).  That is what
 *   torch's backward of .mean() leaves on the device -- its division of a device tensor by a host scalar multiplies by the
 *   rounded reciprocal -- and can differ from *dL_dmean / (float)n_elements, which torch forms on the CPU, in the last bit.
 *   Per window pixel and channel, with g the cotangent,
 *   d = v - img_target_c and s = (d > 0 ? 1 : 0) - (d < 0 ? 1 : 0):
 *     dL_dimg_c = f ? 0 : s * g;    dL_dface_c = f ? s * g : 0.
 *   dL_dimg [B, C, H, W] and dL_dface [B, C + 1, H, W] may each be NULL; each one given is written WHOLE: zeros outside
 *   the window and in the coverage plane of dL_dface (the reference's `== 1` cuts that gradient).  The caller clears
 *   nothing.  Only window pixels read img_out, face, img_target and dL_dmap.
 * exa_composite_forward: the full image, rows = H, runs = ceil(W / 4); out [B, C, H, W]:
 *   EXA_COMPOSITE_FACE_HARD   sel = face [B, C + 1, H, W]:  out_c = f ? face_c : b_c  (a is not read and may be NULL)
 *   EXA_COMPOSITE_FACE_SOFT   sel = face:  w = (face_c != -1 ? 1 : 0) * coverage;  out_c = b_c * (1 - w) + face_c * w, the two
 *                             products rounded before the sum (model.py:268-271; a is not read)
 *   EXA_COMPOSITE_FOREGROUND  sel = mask [B, 1, H, W]:  out_c = mask > thr ? a_c : b_c  (model.py:273-276; the reference's
 *                             is_fg * a + (1 - is_fg) * b with a 0 / 1 weight is this selection for finite inputs)
 * exa_composite_backward: EXA_COMPOSITE_FACE_HARD only: dL_dimg_c = f ? 0 : dL_dout_c, dL_dface_c = f ? dL_dout_c : 0, the
 *   coverage plane of dL_dface zero; either output may be NULL; img is not read (the selection is the face render's alone)
 *   and may be NULL.
 * Negative sizes, a window outside the image, both or neither cotangent, an unknown mode: EXA_RASTER_E_INVALID; a missing
 * array: EXA_RASTER_E_NULLPTR; both before any device call.  The calls neither allocate nor synchronise.
 */
#define EXA_COMPOSITE_FACE_HARD 0
#define EXA_COMPOSITE_FACE_SOFT 1
#define EXA_COMPOSITE_FOREGROUND 2
int64_t exa_face_l1_blocks(int32_t B, int32_t C, int32_t crop_w, int32_t crop_h);
int exa_face_l1_forward(int32_t B, int32_t C, int32_t H, int32_t W, const int32_t* crop, const float* img_out,
                        const float* face, const float* img_target, float* l1_map, float* partials, void* stream);
int exa_face_l1_reduce(int64_t n_partials, int64_t n_elements, const float* partials, float* out_mean, void* stream);
int exa_face_l1_backward(int32_t B, int32_t C, int32_t H, int32_t W, const int32_t* crop, const float* img_out,
                         const float* face, const float* img_target, const float* dL_dmap, const float* dL_dmean,
                         int64_t n_elements, float* dL_dimg, float* dL_dface, void* stream);
int exa_composite_forward(int32_t mode, int32_t B, int32_t C, int32_t H, int32_t W, const float* a, const float* sel,
                          const float* b, float* out, float thr, void* stream);
int exa_composite_backward(int32_t B, int32_t C, int32_t H, int32_t W, const float* img, const float* face,
                           const float* dL_dout, float* dL_dimg, float* dL_dface, void* stream);

/*
 * LPIPS with the VGG-16 trunk (csrc/lpips.hip): lpips.LPIPS(net='vgg') 0.1.4 in eval mode behind the reference's wrapper
 * (avatar/common/nets/loss.py:77-95), forward and the gradient w.r.t. the first image.  fp32 throughout; fused multiply-adds
 * only where written (fmaf, or the MFMA, which is bit-equal to an fmaf chain).
 *
 * Arrays.  img, dL_dimg: [B, 3, H, W].  crop = {x0, y0, w, h}, the clamped bbox, w >= 16 and h >= 16.  Every activation,
 * tap, head gradient and feature array is CHANNEL-INNERMOST: [B, rows, columns, C].  Block b = 0 .. 4 of the trunk works at
 * (h >> b) x (w >> b); the 13 layers have Cin 3, 64 | 64, 128 | 128, 256, 256 | 256, 512, 512 | 512, 512, 512 and
 * Cout 64, 64 | 128, 128 | 256, 256, 256 | 512, 512, 512 | 512, 512, 512; tap t is the output of layer 1, 3, 6, 9, 12
 * (counting from 0) with C = 64, 128, 256, 512, 512.
 * shift_scale: HOST array {shift_r, shift_g, shift_b, scale_r, scale_g, scale_b}.
 * weights, biases, weights_t, head_grads, partials (of the reduce): HOST arrays of device pointers.
 *   weights[0] = weights_t[0]: the first layer as [tap = 3 ky + kx][ci][co] (27 x 64 floats).
 *   weights[l], l >= 1: layer l's [Cout, Cin, 3, 3] as [Cout / 64][Cin / 16][tap][g = 0, 1][co = 0 .. 63][p = 0 .. 7], the
 *     element at p being input channel 16 chunk + 8 g + 2 (p & 3) + (p >> 2).
 *   weights_t[l], l >= 1: the same image of the TRANSPOSED and 180-degree ROTATED weights wt[ci, co, ky, kx] =
 *     w[co, ci, 2 - ky, 2 - kx] (so its Cout is the layer's Cin).
 * Workspace: exa_lpips_workspace_size() bytes ([dev], 256-byte aligned), carved by the library: the 13 activations, the
 * mapped input and two gradient buffers of B h w 64 floats; (270 + 3 + 128) B h w floats but for rounding.  The forward
 * writes every section before it is read; the backward reads the activations its forward left there.
 * exa_lpips_tap_layout() gives tap t's byte offset in it and shape = {rows, columns, C}.
 *
 * exa_lpips_trunk_forward.  Input map per crop pixel and channel: x = ((img * 2 - 1) - shift) / scale, one rounding per
 *   operation.  Convolution (3 x 3, stride 1, zero padding 1 at the border of the CROP) per output element: per chunk of
 *   16 input channels a chain c = 0; c = fma(in, w, c) over the chunk's 144 terms, the taps (ky, kx) row-major and inside a
 *   tap the chunk's channels ascending; s = 0, then s = s + c over the chunks ascending (the first layer: one chain, taps
 *   row-major, its 3 channels ascending, taps in the padding skipped).  The order is a property of the shape alone; a
 *   single K-term chain would carry the rounding of K = 4608 additions at the deep layers.  Then out = max(s + bias, 0).  The 2 x 2 stride-2 max-pool (floor) in front of
 *   blocks 1 .. 4 is taken when the next layer reads its input; pooled arrays are never stored.
 * exa_lpips_normalize: out = f / (sqrt(S) + 1e-10) per pixel of f [N, C], C % 4 == 0, with S = sum_c f_c^2 as four running
 *   sums s_k over the channels c = k (mod 4) ascending, s_k = s_k + f_c * f_c, then (s_0 + s_1) + (s_2 + s_3).
 * exa_lpips_head_forward (one tap; grid of exa_lpips_head_blocks(npix) = ceil(npix / 256) workgroups per image): per pixel
 *   e_c = f_out_c / (sqrt(S) + 1e-10) - n_target_c; d = sum_c lin_c * (e_c * e_c) in S's order; d_map [B, npix] (or NULL)
 *   receives d; partials [B, blocks] receives the workgroup's sum of d: the wave butterfly over lane distances 32 .. 1, then
 *   ((wave 0 + wave 1) + wave 2) + wave 3, as exa_face_l1_forward.
 * exa_lpips_head_reduce: one workgroup per image.  Per tap l = 0 .. n_taps - 1 (n_taps <= EXA_LPIPS_MAX_TAPS): thread j adds
 *   the image's partials j, j + 256, .. in that order, then the workgroup sum, D_l = sum / (float)npix[l]; out[b] =
 *   (((D_0 + D_1) + D_2) + ..).  No atomics: the same bits on every call.
 * exa_lpips_head_backward (one tap): with g = dL_dout[b] * (1 / (float)npix), r = sqrt(S), u_c = ((2 lin_c) e_c) g and
 *   dot = sum_c u_c * f_out_c (S's order): dL_df_c = u_c / (r + 1e-10) - f_out_c * (dot / (r * (r + 1e-10)^2)); where r = 0 the
 *   second term is 0 (torch's sqrt backward gives NaN there: the library's "finite gradient at zero rows" rule).
 * exa_lpips_trunk_backward: head_grads[t] = dL/d(tap t) as exa_lpips_head_backward leaves it.  The gradient of an
 *   activation a of layer l - 1 is the convolution of layer l's (masked) gradient with weights_t[l] in the order above
 *   (Cin and Cout swapped); through a pool it goes to the first maximum of the 2 x 2 window in row-major order and the
 *   row / column an odd size drops gets 0; the head's gradient is added at a tap; then it is multiplied by [a > 0].  The
 *   first layer: per crop pixel and input channel s = 0; taps row-major, the 64 output channels ascending,
 *   s = fma(g[y - ky + 1][x - kx + 1][co], w[tap][ci][co], s); dL_dimg = (s / scale) * 2.  dL_dimg is written WHOLE by that
 *   kernel, zeros outside the crop: the caller clears nothing.
 * Errors before any device call: negative sizes, a window outside the image or below 16 x 16, a short workspace, C not a
 * multiple of 4, a zero scale: EXA_RASTER_E_INVALID; a missing array: EXA_RASTER_E_NULLPTR.  The calls neither allocate nor
 * synchronise; B = 0 is a no-op.
 */
#define EXA_LPIPS_LAYERS 13
#define EXA_LPIPS_TAPS 5
#define EXA_LPIPS_MAX_TAPS 8
#define EXA_LPIPS_MIN_CROP 16
int exa_lpips_workspace_size(int32_t B, int32_t h, int32_t w, uint64_t* bytes);
int exa_lpips_tap_layout(int32_t B, int32_t h, int32_t w, int32_t tap, uint64_t* byte_offset, int32_t* shape);
int exa_lpips_trunk_forward(int32_t B, int32_t H, int32_t W, const int32_t* crop, const float* img,
                            const float* shift_scale, const float* const* weights, const float* const* biases, void* ws,
                            uint64_t ws_bytes, void* stream);
int exa_lpips_trunk_backward(int32_t B, int32_t H, int32_t W, const int32_t* crop, const float* shift_scale,
                             const float* const* weights_t, const float* const* head_grads, void* ws, uint64_t ws_bytes,
                             float* dL_dimg, void* stream);
int exa_lpips_normalize(int64_t N, int32_t C, const float* f, float* out, void* stream);
int64_t exa_lpips_head_blocks(int64_t npix);
int exa_lpips_head_forward(int32_t B, int64_t npix, int32_t C, const float* f_out, const float* n_target, const float* lin,
                           float* d_map, float* partials, void* stream);
int exa_lpips_head_reduce(int32_t B, int32_t n_taps, const float* const* partials, const int64_t* npix, float* out,
                          void* stream);
int exa_lpips_head_backward(int32_t B, int64_t npix, int32_t C, const float* f_out, const float* n_target, const float* lin,
                            const float* dL_dout, float* dL_df, void* stream);

/*
 * The Adam step (csrc/adam.hip): `trainer.optimizer.step()` of the reference (avatar/main/train.py:57, base.py:83-85:
 * torch.optim.Adam without weight decay or amsgrad) for any number of separately allocated tensors, one launch per
 * EXA_RASTER_ADAM_MAX_SEGMENTS of them.  A native host applies the gradients of exa_raster_backward with it.
 *
 * One ExaRasterAdamSegment describes one tensor: four [dev] arrays of n contiguous floats -- param, exp_avg and
 * exp_avg_sq are updated in place, grad is only read -- and the two scalars of the tensor's own step count t and
 * learning rate, which the HOST forms in double and rounds once to float:
 *     step_size = lr / (1 - beta1^t)        bc2_sqrt = sqrt(1 - beta2^t)
 * beta1, beta2 and eps hold for the whole call; the call rounds w1 = (float)(1 - beta1), b2 = (float)beta2,
 * w2 = (float)(1 - beta2) and e = (float)eps once.  Per element, every line one rounded fp32 operation, never fused:
 *     m' = m + w1 * (g - m)                       when w1 < 0.5;  m' = g - (g - m) * (1 - w1) otherwise (torch's lerp)
 *     v' = v * b2 + (w2 * g) * g
 *     d  = sqrtf(v') / bc2_sqrt + e
 *     p' = p + (-step_size) * (m' / d)
 * sqrtf and / are the correctly rounded ones and subnormals are kept, so a float32 restatement on a CPU gives the same
 * bits (tests/adam_oracle.py).  What guarantees it: the file is built without any fast-math flag and with
 * -ffp-contract=off; hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt expands `/` to the v_div_scale / v_div_fmas
 * / v_div_fixup sequence and sqrtf to v_sqrt_f32 plus its fused correction steps, and -fgpu-flush-denormals-to-zero is
 * off for gfx950.  With step_size = 0 (the reference constructs its optimizer with lr = 0.0) p' = p + (-0 * x) = p bit for
 * bit for every finite x (only a p of -0 can become +0), and the moments still advance.  g = 0 over m = v = 0 gives m' = 0, d = e and p' = p.
 *
 * Work split: a workgroup of 256 threads owns one chunk of EXA_RASTER_ADAM_CHUNK consecutive elements of one segment; the
 * chunk counts of the segments lie end to end on a one-dimensional grid and a workgroup finds its segment by a binary
 * search over the prefix counts in its kernel arguments.  The segments travel BY VALUE in the kernel arguments: no device
 * pointer table, no workspace, no atomics, no memset, no allocation, no synchronisation, no state; the same inputs give
 * the same bits.  A thread moves 4 consecutive floats with 16-byte loads and stores when all four arrays of its segment
 * are 16-byte aligned; the elements of any other segment, and the last n % 4 of an aligned one, move one by one.
 * Segments with n = 0 are skipped (their pointers are not looked at); n_seg = 0 or nothing but empty segments: no launch,
 * returns 0.  More than EXA_RASTER_ADAM_MAX_SEGMENTS non-empty segments are issued as several launches on `stream`, in
 * the order given.  Two segments of one call must not overlap (the caller's to ensure).
 *
 * Checked on the host before any launch: segs NULL with n_seg > 0, a NULL array in a segment with n > 0:
 * EXA_RASTER_E_NULLPTR; n_seg < 0, n < 0 or n > EXA_RASTER_ADAM_MAX_N, beta1 or beta2 outside [0, 1), eps < 0, a
 * non-finite beta1 / beta2 / eps / step_size / bc2_sqrt, bc2_sqrt <= 0 (t >= 1 makes it positive): EXA_RASTER_E_INVALID.
 */
#define EXA_RASTER_ADAM_MAX_SEGMENTS 64
#define EXA_RASTER_ADAM_CHUNK 4096
#define EXA_RASTER_ADAM_MAX_N (INT64_C(1) << 36)      /* 64 segments of it are 2^30 chunks: the grid stays below 2^31 */
typedef struct ExaRasterAdamSegment {
    float* param;                           /* [dev] n floats, updated in place */
    const float* grad;                      /* [dev] n floats */
    float* exp_avg;                         /* [dev] n floats, updated in place */
    float* exp_avg_sq;                      /* [dev] n floats, updated in place */
    int64_t n;
    float step_size;                        /* (float)(lr / (1 - beta1^t)) */
    float bc2_sqrt;                         /* (float)sqrt(1 - beta2^t) */
} ExaRasterAdamSegment;
int exa_raster_adam_step(const ExaRasterAdamSegment* segs, int32_t n_seg, double beta1, double beta2, double eps,
                         void* stream);

/*
 * Densification (csrc/densify.hip): the clone, split and prune passes of the reference's SceneGaussian.densify_and_prune
 * (avatar/common/nets/module.py:159-245) decided once per SOURCE row and carried out as one move of all rows.  That is
 * possible because clones never split (their padded gradient is zero, module.py:191-192), clones and split children inherit
 * their source's opacity, and a child's scale is a function of its source's scale.
 *
 * exa_raster_densify_plan classifies the P0 rows and scans the counts; it enqueues two launches and does not synchronise.
 * Per row i, every line one rounded fp32 operation (the doubles of the call are rounded to float once, as CPU torch rounds
 * Python scalars against float32 tensors):
 *     g    = grad_accum[i] / track_cnt[i];  NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX          (nan_to_num)
 *     hot  = g >= (float)grad_thr
 *     m    = max_k expf(scale[3 i + k])                                                           (a NaN wins, as torch.max)
 *     big  = m > (float)dense_percent * extent[0]
 *     low  = 1 / (1 + expf(-opacity[i])) < (float)opacity_min
 *   with prune_big != 0 (otherwise all three are false):
 *     wide       = m > 0.1f * extent[0]
 *     wide_child = max_k expf(logf(expf(scale[3 i + k]) / (float)(0.8 * split_factor))) > 0.1f * extent[0]
 *     screen     = radius_max != NULL && radius_max[i] > (float)screen_size_max
 * (radius_max = NULL reproduces the reference, whose screen-space test reads statistics that densify() has just zeroed.)
 *     EXA_RASTER_DENSIFY_KEEP   the original survives          !(hot && big) && !low && !wide && !screen
 *     EXA_RASTER_DENSIFY_CLONE  a copy of it survives          hot && !big && !low && !wide
 *     EXA_RASTER_DENSIFY_SPLIT  split_factor children survive  hot && big && !low && !wide_child
 *     EXA_RASTER_DENSIFY_CAND   a split candidate              hot && big         (the reference draws noise for it)
 * With mask != NULL (mask mode, prune_points) the code of row i is KEEP when mask[i] == 0 and 0 otherwise, and none of the
 * statistics pointers is looked at.
 *
 * The workspace ([dev], 16-byte aligned, exa_raster_densify_workspace_size(P0) bytes, every byte the move reads is written
 * by the plan) begins with the 16-byte record {n_keep, n_clone, n_split, n_cand} (uint32 each) -- the one thing the host
 * reads back -- followed by one 16-byte record of exclusive offsets per block of EXA_RASTER_DENSIFY_BLOCK rows and one code
 * byte per row:  size = 16 + 16 * ceil(P0 / BLOCK) + 16 * ceil(P0 / 16).
 * The scan is one workgroup of EXA_RASTER_DENSIFY_SCAN threads that loops when there are more blocks than threads.
 *
 * exa_raster_densify_move takes that workspace, the four totals BY VALUE and n_seg segments (a host array; they travel by
 * value in the kernel arguments, EXA_RASTER_DENSIFY_MAX_SEGMENTS per launch, more are issued as several launches).  A
 * segment moves one tensor: src holds P0 rows of row_floats floats, dst has room for dst_rows >= n_out rows,
 *     n_out = n_keep + n_clone + split_factor * n_split,
 * and EVERY element of the first n_out rows of dst is written (no zeros_like before the call).  Output row order, the
 * reference's final order:  surviving originals in source order; surviving clones in source order; copy 0 of every surviving
 * split row in source order; copy 1 of every one; ...   By role:
 *     EXA_RASTER_DENSIFY_COPY    every output row is its source row, bit for bit
 *     EXA_RASTER_DENSIFY_STATE   surviving originals keep their row; every new row is +0.0 (optimizer moments, statistics)
 *     EXA_RASTER_DENSIFY_SCALE   as COPY for originals and clones; a child's element is logf(expf(s) / (float)(0.8 * split_factor))
 *     EXA_RASTER_DENSIFY_MEAN    (row_floats = 3) as COPY for originals and clones; copy c of the k-th split CANDIDATE
 *                                (k counts candidates in source order, surviving or not) is
 *                                    n_j = noise[3 (c * n_cand + k) + j] * expf(scale[3 i + j])
 *                                    out_r = ((R_r0 * n_0 + R_r1 * n_1) + R_r2 * n_2) + mean[3 i + r]
 *                                with R = rotation_6d_to_matrix(rotation[6 i ..]) (csrc/rot6d.h: rows b1, b2, b3) -- the
 *                                reference's draw order (module.py:196-201), so the result can be compared with it row for
 *                                row on the same noise.  `rotation` [P0, 6], `scale` [P0, 3] and `noise`
 *                                [split_factor * n_cand, 3] are the call's; they are needed only for MEAN segments.
 * A workgroup owns one block of source rows, rebuilds the compact lists of its kept, cloned and split rows in LDS (ballot
 * and popcount) and walks its slice of every output range as a flat run of floats.  All accesses are 4 bytes wide and need
 * 4-byte alignment only.  A workgroup that finds other totals in the workspace's record than the call's stores nothing.
 * No global atomics, no memset, no allocation, no synchronisation, no state: the same inputs give the same bits.
 *
 * Checked on the host before any launch: a NULL pointer that the call would read or write: EXA_RASTER_E_NULLPTR; a negative
 * size or total, totals beyond P0 or n_split > n_cand, split_factor outside 1..8, row_floats < 1, a MEAN segment with
 * row_floats != 3, an unknown role, dst_rows < n_out: EXA_RASTER_E_INVALID; workspace_bytes below the size query, or a
 * workspace that is not 16-byte aligned: EXA_RASTER_E_WORKSPACE; a dst range that overlaps a src range, another dst range,
 * the workspace or one of rotation / scale / noise: EXA_RASTER_E_ALIAS.  P0 = 0 (and, for the move, n_seg = 0): returns 0
 * without a launch.
 */
#define EXA_RASTER_DENSIFY_MAX_SEGMENTS 64
#define EXA_RASTER_DENSIFY_BLOCK 256        /* source rows per workgroup */
#define EXA_RASTER_DENSIFY_SCAN 256         /* count records per round of the scan */
#define EXA_RASTER_DENSIFY_KEEP 1
#define EXA_RASTER_DENSIFY_CLONE 2
#define EXA_RASTER_DENSIFY_SPLIT 4
#define EXA_RASTER_DENSIFY_CAND 8
#define EXA_RASTER_DENSIFY_COPY 0
#define EXA_RASTER_DENSIFY_STATE 1
#define EXA_RASTER_DENSIFY_MEAN 2
#define EXA_RASTER_DENSIFY_SCALE 3
typedef struct ExaRasterDensifySegment {
    const float* src;                       /* [dev] P0 rows of row_floats floats */
    float* dst;                             /* [dev] dst_rows rows of row_floats floats; the first n_out are written */
    int64_t row_floats;
    int64_t dst_rows;
    int32_t role;                           /* EXA_RASTER_DENSIFY_COPY / _STATE / _MEAN / _SCALE */
    int32_t reserved;
} ExaRasterDensifySegment;
int exa_raster_densify_workspace_size(int32_t P0, uint64_t* bytes);
int exa_raster_densify_plan(int32_t P0, const float* grad_accum, const float* track_cnt, const float* scale,
                            const float* opacity, const float* radius_max, const float* extent, const uint8_t* mask,
                            double grad_thr, double dense_percent, double opacity_min, int32_t prune_big,
                            int32_t split_factor, double screen_size_max, void* workspace, uint64_t workspace_bytes,
                            void* stream);
int exa_raster_densify_move(int32_t P0, int32_t split_factor, const void* workspace, uint64_t workspace_bytes,
                            int32_t n_keep, int32_t n_clone, int32_t n_split, int32_t n_cand,
                            const ExaRasterDensifySegment* segs, int32_t n_seg, const float* rotation, const float* scale,
                            const float* noise, void* stream);

/*
 * Optional per-kernel timing for benchmarks (the only state the library ever keeps, process-wide,
 * off by default, not thread-safe).  While enabled, every kernel / memset the library enqueues is bracketed by a
 * pair of hipEvents recorded on the caller's stream.  exa_raster_timing_read() synchronises on the
 * events of the most recent calls and returns their durations in milliseconds (-1 for a slot that
 * did not run), then clears the slots.  Slot names: exa_raster_timing_name(i), i < EXA_RASTER_TIMING_SLOTS.
 * Must not be enabled during hipGraph capture.
 */
#define EXA_RASTER_TIMING_SLOTS 9
int exa_raster_timing_enable(int32_t on);
int exa_raster_timing_read(float* ms_out, int32_t n);
const char* exa_raster_timing_name(int32_t slot);

#ifdef __cplusplus
}
#endif
#endif /* EXA_RASTER_H */
