/*
 * exa_mesh.h -- C ABI of the MI355X-native differentiable triangle rasterizer with a fused UV-texture sample.
 *
 * This is the native boundary under ExAvatar's face render: pytorch3d's `MeshRasterizer` + `TexturesUV` as the
 * reference calls them in `get_face_index_map_xy` / `MeshRenderer` (avatar/common/nets/layer.py:23-68).  The Python
 * drop-ins over it are `exavatar_release_amd.mesh.MeshRenderer` and `exavatar_release_amd.mesh.get_face_index_map_xy`;
 * the conventions (projection, coverage, depth test, perspective-correct barycentrics, texture sampling) are written
 * out in that module's docstring.  It lives in the same `libexa_raster.so` as include/exa_raster.h.
 *
 * The same raster also shades: `exa_mesh_vertex_normals` + `exa_mesh_forward_shaded` are the Phong-shaded mesh panel of
 * the reference's `render_mesh` (avatar/common/utils/vis.py:73-109: pytorch3d `SoftPhongShader`, `PointLights`,
 * `Materials`, `TexturesVertex` of ones), under `exavatar_release_amd.mesh.shade_mesh` / `render_mesh`.
 *
 * The mesh regulariser lives here too: `exa_mesh_neighbor_transpose` + `exa_mesh_laplacian_*` are the reference's
 * `LaplacianReg` (avatar/common/nets/loss.py:97-131) under `exavatar_release_amd.mesh_reg.LaplacianReg`.  It is a
 * per-vertex gather over a fixed-order CSR like `exa_mesh_vertex_normals`, and the ABI test pins one ABI per header
 * and the set of headers, so it joins this ABI instead of opening a seventh.  The additions change no existing
 * prototype or struct: EXA_MESH_VERSION stays 100.
 *
 * So do the blend-shape offsets of the same upsampled mesh: `exa_mesh_blend_*` are the reference's pose correctives and
 * expression offsets (avatar/common/nets/module.py:484-493,537) under `exavatar_release_amd.blend_shapes.BlendShapes`.
 *
 * And the forward kinematics that feed the skinning of that mesh: `exa_mesh_kinematics_*` are the reference's
 * `get_transform_mat_joint` (avatar/common/nets/module.py:389-411) under `exavatar_release_amd.kinematics`.
 *
 * And the SMPL-X template stage in front of all of them: `exa_mesh_upsample_*` are the reference's `upsample_mesh`
 * (avatar/common/utils/smpl_x.py:84-91, pytorch3d `SubdivideMeshes`) and `exa_mesh_body_*` its
 * `get_neutral_pose_human(jaw_zero_pose=True, use_id_info=True)` + `get_zero_pose_human()`
 * (avatar/common/nets/module.py:337-387), under `exavatar_release_amd.body`.
 *
 * And the arm and hand regularisers of that mesh: `exa_mesh_arm_*` and `exa_mesh_hand_*` are the reference's
 * `ArmRGBReg`, `HandRGBReg` and `HandMeanReg` (avatar/common/nets/loss.py:148-197), under
 * `exavatar_release_amd.vertex_regs`.
 *
 * And the pose parameters in front of the kinematics: `exa_mesh_pose_*` are the reference's `SMPLXParamDict.forward`
 * (avatar/common/nets/module.py:649-684) and the detached pose features of module.py:464,484,498, under
 * `exavatar_release_amd.pose_params`.
 *
 * And the last four terms of the loss block: `exa_mesh_offset_regs_*` are the reference's `gaussian_mean_reg`,
 * `gaussian_scale_reg`, `joint_offset_reg` and `JointOffsetSymmetricReg` (avatar/main/model.py:217-232, 253-257,
 * avatar/common/nets/loss.py:133-146), under `exavatar_release_amd.offset_regs`.
 *
 * And the face texture that the face render samples: `exa_mesh_forward_ortho` is the same raster under pytorch3d's
 * `OrthographicCameras` (the reference's `get_face_index_map_uv`, fitting/common/nets/layer.py:9-23) and
 * `exa_mesh_unwrap` the reference's `XY2UV.forward` with the accumulation of fitting/main/unwrap.py:76-83
 * (layer.py:41-102), under `exavatar_release_amd.unwrap`.  Forward only.
 *
 * And the mesh terms of the fitting program's loss: `exa_mesh_edge_length_*`, `exa_mesh_flip_symmetry_*`,
 * `exa_mesh_pose_loss_*` and `exa_mesh_centered_v2v_*` are the reference's `EdgeLengthLoss`, `FaceOffsetSymmetricReg`,
 * `PoseLoss` (fitting/common/nets/loss.py:73-87, 125-167) and the centred vertex-to-vertex term of
 * fitting/main/model.py:235-237, under `exavatar_release_amd.fit_terms`.
 *
 * And the keypoints of that loss: `exa_mesh_keypoints_*` are the tail of the SMPL-X layer (extra joints, static and dynamic
 * landmarks; smplx/body_models.py:1257-1283) with the tail of `get_smplx_coord` / `get_flame_coord`
 * (fitting/main/model.py:97-117, 140-157), and `exa_mesh_coord_loss_*` the reference's `CoordLoss`
 * (fitting/common/nets/loss.py:9-71), under `exavatar_release_amd.keypoints`.
 *
 * Conventions (those of exa_raster.h)
 *   - plain C types only: device pointers, sizes, a `hipStream_t` passed as `void*`.
 *   - every pointer marked [dev] is a device pointer owned by the caller; the library allocates nothing and keeps no
 *     state between calls.  Workspace sizes follow from the shapes alone (exa_mesh_workspace_sizes): there is no
 *     capacity and no overflow path.
 *   - fp32 geometry and texture, int32 topology, int64 `pix_to_face`; contiguous row-major arrays.
 *   - N meshes of ONE topology per call (the packed layout): verts[N,V,3] in camera space (x right, y down, z forward;
 *     the reference's world->camera transform stays with the caller), faces[F,3], focal[N,2], princpt[N,2].
 *   - work is enqueued on `stream`; no call synchronises the device.
 *   - return value: 0 = ok; < 0 = invalid argument (EXA_MESH_E_*); > 0 = HIP error code (hipError_t).
 *   - the backward is atomic-free and bit-deterministic: the same inputs give the same bits on every call.
 */
#ifndef EXA_MESH_H
#define EXA_MESH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EXA_MESH_VERSION 100            /* 0.1.0.0: first version */
#define EXA_MESH_CELL 64                /* faces are binned to 64x64-pixel cells */
#define EXA_MESH_TILE 16                /* the forward raster runs one workgroup per 16x16-pixel tile */
#define EXA_MESH_MAX_CHANNELS 8         /* texture channels per call */

#define EXA_MESH_E_INVALID (-1)
#define EXA_MESH_E_NULLPTR (-2)

/* One call's scene: N meshes of one topology seen by N pinhole cameras, rendered at H x W. */
typedef struct ExaMeshGeometry {
    int32_t N, V, F;                    /* meshes, vertices per mesh, faces */
    int32_t H, W;                       /* image rows, columns */
    const float* verts;                 /* [dev] [N, V, 3] camera-space positions */
    const int32_t* faces;               /* [dev] [F, 3] vertex indices, each in [0, V) */
    const float* focal;                 /* [dev] [N, 2] (fx, fy) in pixels */
    const float* princpt;               /* [dev] [N, 2] (cx, cy) in pixels */
} ExaMeshGeometry;

/* The UV texture of a fused render (pytorch3d TexturesUV): `face_uvs` holds the three corner uvs of every face, already
 * in pytorch3d's convention (v up); the map is sampled vertically flipped, bilinear, align_corners, border padding. */
typedef struct ExaMeshTexture {
    int32_t C;                          /* channels, 1 .. EXA_MESH_MAX_CHANNELS */
    int32_t tex_H, tex_W;               /* texture rows, columns (each >= 1) */
    int32_t tex_N;                      /* 1 (one map for all meshes) or N */
    const float* texture;               /* [dev] [tex_N, C, tex_H, tex_W] */
    const float* face_uvs;              /* [dev] [F, 3, 2] */
} ExaMeshTexture;

/* Phong shading of a forward_shaded call (pytorch3d `phong_shading` with one point light and vertex colours of one).
 * Every vector is in this header's camera frame (x right, y down, z forward); the camera centre is the origin.  At a
 * covered pixel, with p and n the perspective-correct interpolations of the nearest face's positions and vertex
 * normals, l^ = normalize(light_location - p), n^ = normalize(n), v^ = normalize(-p), cos = n^ . l^ (no flip towards the
 * viewer: the winding decides which side is lit), r = -l^ + 2 cos n^:
 *   colour = light_ambient * material_ambient + light_diffuse * material_diffuse * max(cos, 0)
 *          + light_specular * material_specular * (max(v^ . r, 0) * [cos > 0]) ^ shininess        (0 ^ 0 = 1)
 * per channel; normalize(x) = x / max(|x|, 1e-6).  Empty pixels get `background`. */
typedef struct ExaMeshShading {
    float light_location[3];
    float light_ambient[3], light_diffuse[3], light_specular[3];
    float material_ambient[3], material_diffuse[3], material_specular[3];
    float shininess;                    /* >= 0 */
    float background[3];
} ExaMeshShading;

typedef struct ExaMeshWorkspaceSizes {
    uint64_t face_bytes;                /* per-face screen records: written by forward, read by backward */
    uint64_t bin_bytes;                 /* per-cell face bitmasks: forward only */
    uint64_t grad_bytes;                /* per-face corner gradients: backward only */
} ExaMeshWorkspaceSizes;

int exa_mesh_version(void);
/* Message of the most recent failing call of this thread ("" if none). */
const char* exa_mesh_last_error(void);

int exa_mesh_workspace_sizes(int32_t N, int32_t F, int32_t H, int32_t W, ExaMeshWorkspaceSizes* out);

/* Host-side helper: the vertex -> (face, corner) lists the backward gathers over, in CSR form and in a fixed order
 * (ascending face, then corner).  `faces` [F,3], `offsets` [V+1] and `entries` [3F] (value 3 * face + corner) are HOST
 * memory.  Build once per topology and copy to the device. */
int exa_mesh_vertex_faces(int32_t V, int32_t F, const int32_t* faces, int32_t* offsets, int32_t* entries);

/* Rasterize (and, with `tex` != NULL, texture) N meshes.
 *   face_ws, bin_ws  [dev] workspaces of the sizes above; face_ws must stay untouched until the matching backward.
 *   pix_to_face      [dev] [N, H, W] int64: n * F + f of the nearest covering face, -1 for background (required).
 *   zbuf             [dev] [N, H, W] or NULL: interpolated view-space z, -1 for background.
 *   bary             [dev] [N, H, W, 3] or NULL: perspective-correct barycentrics, -1 for background.
 *   render           [dev] [N, C, H, W]: the sampled texture, -1 in every channel of a background pixel; required with
 *                    `tex`, ignored without. */
int exa_mesh_forward(const ExaMeshGeometry* g, const ExaMeshTexture* tex, void* face_ws, void* bin_ws,
                     int64_t* pix_to_face, float* zbuf, float* bary, float* render, void* stream);

/* dL/dverts from the gradients of the forward's outputs.  `g`, `tex`, `face_ws` and `pix_to_face` are those of the
 * forward.  Any of dL_dzbuf [N,H,W], dL_dbary [N,H,W,3] and dL_drender [N,C,H,W] may be NULL (no gradient);
 * dL_drender needs `tex`.  vert_offsets / vert_entries: exa_mesh_vertex_faces' CSR, on the device.
 *   grad_ws    [dev] workspace of grad_bytes.
 *   dL_dverts  [dev] [N, V, 3], fully written (vertices no face uses get 0). */
int exa_mesh_backward(const ExaMeshGeometry* g, const ExaMeshTexture* tex, const void* face_ws,
                      const int64_t* pix_to_face, const float* dL_dzbuf, const float* dL_dbary, const float* dL_drender,
                      const int32_t* vert_offsets, const int32_t* vert_entries, void* grad_ws, float* dL_dverts,
                      void* stream);

/* Area-weighted vertex normals (pytorch3d `_compute_vertex_normals`): every face adds, at each corner k, the cross
 * product (v_{k+1} - v_k) x (v_{k+2} - v_k) -- culled and hidden faces too -- and each sum is normalised as
 * x / max(|x|, 1e-6).  Gathered over exa_mesh_vertex_faces' CSR in its fixed order: atomic-free, bit-deterministic.
 * Uses g's N, V, F, verts and faces (H, W unused).
 *   vert_offsets, vert_entries  [dev] the CSR of `faces`.
 *   normals                     [dev] [N, V, 3], fully written (vertices no face uses get 0). */
int exa_mesh_vertex_normals(const ExaMeshGeometry* g, const int32_t* vert_offsets, const int32_t* vert_entries,
                            float* normals, void* stream);

/* Rasterize N meshes (as exa_mesh_forward) and Phong-shade the nearest face of every pixel.
 *   shading          HOST pointer: lights, materials, background.
 *   normals          [dev] [N, V, 3]: exa_mesh_vertex_normals of the same verts.
 *   face_ws, bin_ws  [dev] workspaces of exa_mesh_workspace_sizes (face_bytes, bin_bytes).
 *   pix_to_face      [dev] [N, H, W] int64 or NULL: as exa_mesh_forward.
 *   zbuf             [dev] [N, H, W] or NULL: as exa_mesh_forward.
 *   image            [dev] [N, H, W, 3] (channel-last): the shaded colour, `background` at empty pixels (required). */
int exa_mesh_forward_shaded(const ExaMeshGeometry* g, const ExaMeshShading* shading, const float* normals, void* face_ws,
                            void* bin_ws, int64_t* pix_to_face, float* zbuf, float* image, void* stream);

/* ---- Face-texture unwrap (reference XY2UV and get_face_index_map_uv, fitting/common/nets/layer.py:9-23, 41-102) -----
 * Forward only: nothing in the reference differentiates through the unwrap.
 *
 * exa_mesh_forward_ortho is exa_mesh_forward under pytorch3d's OrthographicCameras(in_ndc=False) with focal 1 and
 * principal point 0: x and y of `verts` are screen coordinates in pixels (the centre of pixel (row i, col j) lies at
 * (j + 0.5, i + 0.5)), z is the depth; g->focal and g->princpt are ignored and may be NULL.  Coverage, the degenerate-face
 * rule, the z <= 1e-6 cull and the tie rule are exa_mesh_forward's.  pytorch3d corrects barycentrics for perspective only
 * under a perspective camera, so `bary` holds the plain screen barycentrics b_k = E_k / A and
 * zbuf = (b_0 z_0 + b_1 z_1) + b_2 z_2; -1 at background pixels in all three outputs.  The reference's UV raster is this call
 * on (u * W, v * H, 1).  Same workspaces as exa_mesh_forward; zbuf and bary may be NULL. */
int exa_mesh_forward_ortho(const ExaMeshGeometry* g, void* face_ws, void* bin_ws, int64_t* pix_to_face, float* zbuf,
                           float* bary, void* stream);

/* One unwrap: B images [B, C, H, W] sampled into B maps [B, C, Hu, Wu] through a mesh of V vertices and F faces.
 *
 * VISIBLE FACES.  Face f of item n is visible when some pixel of pix_to_face_xy[n] holds n * F + f (the packed index
 * exa_mesh_forward writes).  The reference's wrap-around is reproduced: its torch.unique keeps the -1 of background
 * pixels and `valid_face_mask[-1] = 1` then marks the LAST face, so when item n has at least one background pixel, face
 * F - 1 is visible whether it was hit or not.  A value outside {-1} and [n F, (n + 1) F) marks nothing.
 *
 * TEXELS.  Texel t = (row, col) of the map holds face f = pix_to_face_uv[t] and barycentrics b = bary_uv[t] (item 0 of
 * an exa_mesh_forward_ortho of the UV atlas: f is an index into `faces`).  Where f is -1 (or outside [0, F)), or face f of
 * item n is not visible: value = +0.0 and mask = 0 in every channel (the reference has -0.0 there).  Otherwise, with
 * (X_k, Y_k, Z_k) = verts[n, faces[f, k]], every operation rounded in fp32, never contracted, in this order:
 *   x_k = (X_k / Z_k) * fx + cx,   y_k = (Y_k / Z_k) * fy + cy                        (fx, fy) = focal[n], (cx, cy) = princpt[n]
 *   px  = (x_0 b_0 + x_1 b_1) + x_2 b_2,   py likewise
 *   gx  = ((px / (float)(W - 1)) * 2) - 1,   gy = ((py / (float)(H - 1)) * 2) - 1
 *   ix  = ((gx + 1) / 2) * (float)(W - 1),   iy = ((gy + 1) / 2) * (float)(H - 1)      F.grid_sample, align_corners=True
 *   x0 = floor(ix), y0 = floor(iy);  nw = ((x0 + 1) - ix) * ((y0 + 1) - iy),  ne = (ix - x0) * ((y0 + 1) - iy),
 *   sw = ((x0 + 1) - ix) * (iy - y0),  se = (ix - x0) * (iy - y0)
 *   v = +0.0; v = v + img(y0, x0) * nw; v = v + img(y0, x0 + 1) * ne; v = v + img(y0 + 1, x0) * sw;
 *   v = v + img(y0 + 1, x0 + 1) * se                       a tap outside the image is skipped (padding_mode='zeros')
 *   mask = (v != -1);  value = mask ? v : +0.0             per channel
 * A position that is not finite (an image of one row or column divides by zero, as in the reference) has no tap inside:
 * v = +0.0, mask = 1.  A raster-visible face has every corner at Z > 1e-6.  The wrap-around can mark a last face that the
 * raster culled; where one of its corners has Z <= 1e-6 the reference samples through a mirrored or non-finite
 * projection, and this call writes value = +0.0 and mask = 0 instead: the one deliberate difference.
 *
 * ACCUMULATION (reference fitting/main/unwrap.py:76-83), when tex_sum is given: one thread owns a texel and adds the items
 * in index order, so there are no atomics and the same inputs give the same bits:
 *   tex_sum[c, t]  = tex_sum[c, t]  + (value[n, c, t] * uv_weight[t]) * face_valid[n]           n = 0 .. B - 1
 *   mask_sum[c, t] = mask_sum[c, t] + ((float)mask[n, c, t] * uv_weight[t]) * face_valid[n]
 * in place.  uvmap and mask may then be NULL (no [B, C, Hu, Wu] array is written). */
typedef struct ExaMeshUnwrap {
    int32_t B, V, F, C;                 /* items, vertices per item, faces, channels (1 .. EXA_MESH_MAX_CHANNELS) */
    int32_t H, W;                       /* image rows, columns */
    int32_t Hu, Wu;                     /* map rows, columns */
    const float* img;                   /* [dev] [B, C, H, W] */
    const float* verts;                 /* [dev] [B, V, 3] camera space */
    const int32_t* faces;               /* [dev] [F, 3] */
    const float* focal;                 /* [dev] [B, 2] */
    const float* princpt;               /* [dev] [B, 2] */
    const int64_t* pix_to_face_xy;      /* [dev] [B, H, W]: exa_mesh_forward's of the same verts at H x W (an INPUT) */
    const int64_t* pix_to_face_uv;      /* [dev] [Hu, Wu] */
    const float* bary_uv;               /* [dev] [Hu, Wu, 3] */
    const float* uv_weight;             /* [dev] [Hu, Wu]; required with tex_sum, else ignored */
    const float* face_valid;            /* [dev] [B] or NULL (every item counts 1); read with tex_sum only */
} ExaMeshUnwrap;

/* Bytes of the visibility flags ([B, F], one byte each, rounded up to 256). */
int exa_mesh_unwrap_workspace_size(int32_t B, int32_t F, uint64_t* out_bytes);

/* Three launches: the flags are cleared by a kernel of the library's (no memset), marked by one thread per image pixel
 * (every writer stores the same byte: no atomics), and one thread per texel writes all items and channels.
 *   flag_ws            [dev] of ws_bytes >= exa_mesh_unwrap_workspace_size.
 *   uvmap              [dev] [B, C, Hu, Wu] float, fully written; mask [dev] [B, C, Hu, Wu] bytes (0 / 1), fully written.
 *                      Both or neither; required without tex_sum.
 *   tex_sum, mask_sum  [dev] [C, Hu, Wu] float, updated in place; both or neither.
 * B == 0 or Hu * Wu == 0 is a successful no-op. */
int exa_mesh_unwrap(const ExaMeshUnwrap* u, void* flag_ws, uint64_t ws_bytes, float* uvmap, uint8_t* mask,
                    float* tex_sum, float* mask_sum, void* stream);

/* ---- Mesh Laplacian regulariser (reference LaplacianReg) ------------------------------------------------------------
 * x [B, V, C] fp32 (1 <= C <= EXA_MESH_LAP_MAX_CHANNELS), a neighbour table nbr_idx [V, K] int32 / nbr_w [V, K] fp32
 * (1 <= K <= EXA_MESH_LAP_MAX_NEIGHBORS; general weights, the reference's are -1/n in the first n slots and its
 * padded slots hold the vertex itself with weight 0).  V * K <= 2^28.
 *
 * Arithmetic, every operation rounded in fp32, no fused multiply-add, in exactly this order:
 *   lap(x)[b,v,c] = x[b,v,c];  for k = 0 .. K-1 in order:  lap = lap + x[b, nbr_idx[v,k], c] * nbr_w[v,k]
 *   d    = lap(out)                  without a target
 *   d    = lap(out) - lap(target)    with a target [Bt, V, C], Bt == B or Bt == 1 (broadcast over b)
 *   loss = d * d,  then  loss = loss * weight[v]  with a weight [V]
 * Padded slots are evaluated like any other slot.  A slot whose index lies outside [0, V) reads nothing and
 * contributes NaN.
 *
 * Backward, atomic-free and bit-deterministic.  g[b,u,c] = (grad_loss[b,u,c] * weight[u]) * (2 * d[b,u,c]) (the first
 * product only with a weight), then
 *   dL_dout[b,v,c] = g[b,v,c];  for every (u, k) with nbr_idx[u,k] == v, ascending u then ascending k:
 *                    dL_dout = dL_dout + nbr_w[u,k] * g[b,u,c]
 * over the transposed table of exa_mesh_neighbor_transpose.  target and weight get no gradient.  B == 0 or V == 0 is
 * a successful no-op in every call. */
#define EXA_MESH_LAP_MAX_CHANNELS 8
#define EXA_MESH_LAP_MAX_NEIGHBORS 16

/* Host-side helper: the incoming lists of the backward, in CSR form: for every vertex v the slots (u, k) with
 * nbr_idx[u,k] == v, ascending u then k.  `nbr_idx` [V,K], `offsets` [V+1] and `entries` [V*K] (value u * K + k) are
 * HOST memory.  EXA_MESH_E_INVALID, with a message naming it, for the first index outside [0, V).  Build once per
 * topology and copy to the device. */
int exa_mesh_neighbor_transpose(int32_t V, int32_t K, const int32_t* nbr_idx, int32_t* offsets, int32_t* entries);

/* One launch.  out [dev] [B,V,C]; target [dev] [Bt,V,C] or NULL (then Bt is ignored); nbr_idx, nbr_w [dev] [V,K];
 * weight [dev] [V] or NULL; loss, d [dev] [B,V,C], fully written (d is what the backward reads). */
int exa_mesh_laplacian_forward(int32_t B, int32_t Bt, int32_t V, int32_t C, int32_t K, const float* out,
                               const float* target, const int32_t* nbr_idx, const float* nbr_w, const float* weight,
                               float* loss, float* d, void* stream);

/* Bytes of the backward's workspace (g, staged by its first launch). */
int exa_mesh_laplacian_workspace_size(int32_t B, int32_t V, int32_t C, uint64_t* out_bytes);

/* Two launches.  d [dev] the forward's; grad_loss [dev] [B,V,C]; nbr_w, weight as in the forward; in_offsets [dev]
 * [V+1] and in_entries [dev] [V*K]: exa_mesh_neighbor_transpose's CSR; ws [dev] of ws_bytes >=
 * exa_mesh_laplacian_workspace_size (NULL only when that is 0); dL_dout [dev] [B,V,C], fully written. */
int exa_mesh_laplacian_backward(int32_t B, int32_t V, int32_t C, int32_t K, const float* d, const float* grad_loss,
                                const float* nbr_w, const float* weight, const int32_t* in_offsets,
                                const int32_t* in_entries, void* ws, uint64_t ws_bytes, float* dL_dout, void* stream);

/* ---- Blend-shape offsets (reference pose correctives and expression offsets) ---------------------------------------
 * The reference's `torch.matmul(pose, pose_dirs)` with its hand / face mask (module.py:484-493) and its
 * `(expr[None,None,:] * expr_dirs).sum(2)` (module.py:537) are one operation: a coefficient vector coef [K]
 * (1 <= K <= EXA_MESH_BLEND_MAX_K) times a matrix of which only some columns matter, scattered to a flat output [M]
 * (M = 3 V for a [V, 3] result, M <= 2^30).  The matrix travels compacted, as a plan built once per model
 * (exavatar_release_amd.blend_shapes builds it):
 *   table [K, ld]  feature-major, fp32: column s < N is kept column cols[s] of the full matrix; ld >= N is a multiple
 *                  of 4 (rows start on 16-byte boundaries; the pointer is 16-byte aligned); columns N .. ld-1 are zero.
 *   cols  [N]      int32, ascending: compact column -> flat output index in [0, M).
 *   inv   [M]      int32: flat output index -> compact column, -1 where no column covers it.
 * Like exa_mesh_laplacian_* this is a per-vertex operation on the upsampled mesh, and the ABI test pins one ABI per
 * header and the set of headers, so it joins this ABI; no existing prototype changes: EXA_MESH_VERSION stays 100.
 *
 * Forward.  Every operation rounded in fp32, no fused multiply-add, in exactly this order, which depends on K alone:
 * the rows are cut into EXA_MESH_BLEND_SEGMENTS = 8 segments of L = ceil(K / 8) rows, segment s = rows s L ..
 * min(K, (s + 1) L) - 1 (empty where s L >= K);
 *   p_s = +0.0;  for k in segment s, ascending:  p_s = p_s + coef[k] * table[k, col]
 *   sum = p_0;   for s = 1 .. 7 in order:        sum = sum + p_s
 *   out[cols[col]] = sum, out_masked[cols[col]] = +0.0                 for every column col < N
 *   out[j] = out_masked[j] = base[j]  (+0.0 without a base)            for every j with inv[j] < 0
 * Every element of out and out_masked is written exactly once; nothing is memset.  This is the reference's
 * (output, mean_offset_offset) pair of module.py:493 with base = mean_offset_offset, up to the sign of a zero.
 *
 * Backward, atomic-free and bit-deterministic.  With g = g_out gathered through cols (0 for columns >= N):
 *   dL_dbase[j] = g_out[j] + g_masked[j] where inv[j] < 0 (one of them alone where the other is NULL), +0.0 elsewhere.
 *   dL_dcoef[k]: the compact columns are cut into chunks of EXA_MESH_BLEND_CHUNK = 1024.  In a chunk, lane t of 256
 *     owns columns 4 t .. 4 t + 3 and forms q_t = ((T0 g0 + T1 g1) + T2 g2) + T3 g3; the 64 lanes of each of the four
 *     waves (lanes 64 w .. 64 w + 63) are added as a tree, for off = 32, 16, 8, 4, 2, 1 in order q_i = q_i + q_(i+off)
 *     for i < off; the chunk's partial is ((w_0 + w_1) + w_2) + w_3; and
 *     dL_dcoef[k] = +0.0, then for chunk = 0, 1, .. in order: dL_dcoef[k] = dL_dcoef[k] + partial[chunk, k].
 * The table is data: it gets no gradient.  M == 0 is a successful no-op; N == 0 is valid (everything is uncovered). */
#define EXA_MESH_BLEND_MAX_K 512
#define EXA_MESH_BLEND_SEGMENTS 8
#define EXA_MESH_BLEND_CHUNK 1024

/* One launch.  coef [dev] [K]; table [dev] [K, ld]; cols [dev] [N]; inv [dev] [M]; base [dev] [M] or NULL;
 * out [dev] [M]; out_masked [dev] [M] or NULL (not wanted).  table and cols may be NULL when N == 0. */
int exa_mesh_blend_forward(int32_t K, int32_t N, int32_t ld, int32_t M, const float* coef, const float* table,
                           const int32_t* cols, const int32_t* inv, const float* base, float* out, float* out_masked,
                           void* stream);

/* Bytes of the backward's workspace (the chunks' partials, [ceil(N / 1024), K]).  Host only. */
int exa_mesh_blend_workspace_size(int32_t K, int32_t N, uint64_t* out_bytes);

/* At most two launches.  table, cols, inv as in the forward; g_out, g_masked [dev] [M]: the gradients of out and
 * out_masked (g_masked may be NULL; g_out may be NULL when dL_dcoef is); ws [dev] of ws_bytes >=
 * exa_mesh_blend_workspace_size, needed for dL_dcoef only (NULL when that size is 0); dL_dcoef [dev] [K] or NULL (not
 * wanted: the table is not read); dL_dbase [dev] [M] or NULL (not wanted).  Both are fully written. */
int exa_mesh_blend_backward(int32_t K, int32_t N, int32_t ld, int32_t M, const float* table, const int32_t* cols,
                            const int32_t* inv, const float* g_out, const float* g_masked, void* ws, uint64_t ws_bytes,
                            float* dL_dcoef, float* dL_dbase, void* stream);

/* ---- Forward kinematics (reference get_transform_mat_joint) ---------------------------------------------------------
 * The pose -> joint-transform chain in front of the skinning: pytorch3d's `axis_angle_to_matrix`, smplx's
 * `batch_rigid_transform` (avatar/common/utils/smplx/smplx/lbs.py:361-417) and the `bmm` with the big-pose transforms
 * (avatar/common/nets/module.py:389-411), under `exavatar_release_amd.kinematics.joint_transforms`.  B skeletons of one
 * tree per call, J joints (1 <= J <= EXA_MESH_KIN_MAX_JOINTS), one wave per skeleton, one launch each way, no
 * workspace.  Like the Laplacian and the blend shapes it joins this ABI; no existing prototype changes:
 * EXA_MESH_VERSION stays 100.
 *
 * `parents` is a HOST int32[J]: parents[0] == -1 and 0 <= parents[i] < i.  It is checked before any GPU work and
 * travels to the kernel by value; the library keeps nothing between calls.  depth(0) = 0, depth(i) =
 * depth(parents[i]) + 1.
 *
 * Forward.  Every operation rounded in fp32, no fused multiply-add, in exactly this order, per joint j:
 *   1. R_j.  With `rot_in`: R_j = rot_in[j].  With `pose` = (x, y, z), pytorch3d's quaternion route:
 *        angle = sqrt((x x + y y) + z z);  half = 0.5 angle
 *        s = sin(half) / angle, or 0.5 - (angle angle) / 48 when angle < 1e-6
 *        (r, i, j, k) = (cos(half), s x, s y, s z);  n = ((r r + i i) + j j) + k k;  two_s = 2 / n
 *        R = [1 - two_s (j j + k k),  two_s (i j - k r),      two_s (i k + j r);
 *             two_s (i j + k r),      1 - two_s (i i + k k),  two_s (j k - i r);
 *             two_s (i k - j r),      two_s (j k + i r),      1 - two_s (i i + j j)]
 *      sin and cos are the device library's sinf / cosf: this is the one step a CPU does not reproduce bit for bit.
 *      R_j is written to `rot`.
 *   2. L_j = [R_j | t_j],  t_j = joints[j] - joints[parents[j]]  (t_0 = joints[0]).
 *   3. W_0 = L_0; then for depth 1, 2, .. (a joint after its parent p), rows r = 0 .. 2:
 *        W_j[r][c] = (W_p[r][0] R_j[0][c] + W_p[r][1] R_j[1][c]) + W_p[r][2] R_j[2][c]            c = 0 .. 2
 *        W_j[r][3] = ((W_p[r][0] t_j[0] + W_p[r][1] t_j[1]) + W_p[r][2] t_j[2]) + W_p[r][3]
 *      posed_joints[j] = W_j[:, 3].
 *   4. A_j[r][c] = W_j[r][c] (c < 3),  A_j[r][3] = W_j[r][3] - ((W_j[r][0] J_0 + W_j[r][1] J_1) + W_j[r][2] J_2) with
 *      J = joints[j];  row 3 of A_j = (0, 0, 0, 1).
 *   5. Without `pre`: transforms[j] = A_j.  With `pre`: rows r = 0 .. 2
 *        transforms[j][r][c] = ((A[r][0] pre[0][c] + A[r][1] pre[1][c]) + A[r][2] pre[2][c]) + A[r][3] pre[3][c]
 *      and row 3 = row 3 of pre[j].
 *
 * Backward, atomic-free and bit-deterministic.  g = grad_transforms[j] (zero when NULL), gp = grad_posed_joints[j]
 * (zero when NULL); W is recomputed exactly as above from the saved `rot`.
 *   GA[r][k] = g[r][k] without `pre`, else ((g[r][0] pre[k][0] + g[r][1] pre[k][1]) + g[r][2] pre[k][2]) +
 *              g[r][3] pre[k][3]                                                       r = 0 .. 2, k = 0 .. 3
 *   grad_pre[k][c] = (A[0][k] g[0][c] + A[1][k] g[1][c]) + A[2][k] g[2][c]  for k < 3, and
 *   grad_pre[3][c] = ((A[0][3] g[0][c] + A[1][3] g[1][c]) + A[2][3] g[2][c]) + g[3][c]
 *   GW_j[r][c] = GA[r][c] - GA[r][3] J_c (c < 3),  GW_j[r][3] = GA[r][3] + gp[r]         the joint's own term
 *   rest_c = (GA[0][3] W_j[0][c] + GA[1][3] W_j[1][c]) + GA[2][3] W_j[2][c]
 *   for depth d = deepest .. 1: every parent p of depth d - 1 adds, over its children i of depth d in ascending i,
 *        GW_p[r][k] = GW_p[r][k] + (((GW_i[r][0] R_i[k][0] + GW_i[r][1] R_i[k][1]) + GW_i[r][2] R_i[k][2]) +
 *                                   GW_i[r][3] t_i[k])       k < 3,       GW_p[r][3] = GW_p[r][3] + GW_i[r][3]
 *      (GW_i is final by then: its own children were added one level earlier)
 *   GL_j[k][c] = (W_p[0][k] GW_j[0][c] + W_p[1][k] GW_j[1][c]) + W_p[2][k] GW_j[2][c]   (GL_0 = GW_0), k < 3, c < 4
 *   grad_rot[j] = GL_j[:, 0 .. 2]
 *   grad_joints[j][c] = (-rest_c + GL_j[c][3]), then for the children i of j in ascending i: - GL_i[c][3]
 *   grad_pose[j] = the analytic Jacobian of step 1 applied to grad_rot[j], with d angle / d x := 0 at angle == 0 (what
 *      torch's `norm` gives): a zero pose row gets the finite gradient of q = (1, x / 2, y / 2, z / 2), not NaN.
 * B == 0 is a successful no-op in every call. */
#define EXA_MESH_KIN_MAX_JOINTS 64

/* Host-only helper: validates the tree (EXA_MESH_E_INVALID with a message naming the first bad entry) and writes every
 * joint's depth.  parents [J] and depth_out [J] are HOST memory. */
int exa_mesh_kinematics_depths(int32_t J, const int32_t* parents, int32_t* depth_out);

/* One launch.  parents HOST [J]; exactly one of pose [dev] [B, J, 3] (axis-angle) and rot_in [dev] [B, J, 3, 3];
 * joints [dev] [B, J, 3]; pre [dev] [B, J, 4, 4] or NULL; transforms [dev] [B, J, 4, 4], posed_joints [dev] [B, J, 3]
 * and rot [dev] [B, J, 3, 3]: all required, fully written. */
int exa_mesh_kinematics_forward(int32_t B, int32_t J, const int32_t* parents, const float* pose, const float* rot_in,
                                const float* joints, const float* pre, float* transforms, float* posed_joints,
                                float* rot, void* stream);

/* One launch.  pose as in the forward (read for grad_pose only, else NULL); rot [dev] the forward's output; joints, pre
 * as in the forward; grad_transforms [dev] [B, J, 4, 4] and grad_posed_joints [dev] [B, J, 3]: either may be NULL
 * (zero).  Outputs, each [dev], optional (NULL: not wanted) and fully written when given: grad_pose [B, J, 3] (needs
 * pose), grad_rot [B, J, 3, 3], grad_joints [B, J, 3], grad_pre [B, J, 4, 4] (needs pre). */
int exa_mesh_kinematics_backward(int32_t B, int32_t J, const int32_t* parents, const float* pose, const float* rot,
                                 const float* joints, const float* pre, const float* grad_transforms,
                                 const float* grad_posed_joints, float* grad_pose, float* grad_rot, float* grad_joints,
                                 float* grad_pre, void* stream);

/* ---- Pose parameters (reference SMPLXParamDict.forward) and the detached pose features -------------------------------
 * `matrix_to_axis_angle(rotation_6d_to_matrix(p))` for the pose tensors of the frames of a call
 * (avatar/common/nets/module.py:673-684), under `exavatar_release_amd.pose_params`: the per-frame 6D rotation parameters
 * become the axis-angle rows the kinematics take, in ONE launch each way.  It joins this ABI like the kinematics it
 * feeds; no existing prototype changes: EXA_MESH_VERSION stays 100.
 *
 * A call takes n_seg <= EXA_MESH_POSE_MAX_SEGMENTS segments: separately allocated [rows[s], 6] inputs (the parameters as
 * they are; nothing is concatenated).  `rows`, and the arrays of pointers, are HOST arrays of n_seg entries whose
 * pointers are device pointers; they are checked before any GPU work and travel to the kernel by value: no device
 * buffer, no copy, no state between calls.  A segment of 0 rows is valid (its pointers are not read); n_seg == 0 and a
 * call without rows are successful no-ops.  R = the sum of rows (<= EXA_MESH_POSE_MAX_ROWS); packed row start[s] + k is
 * row k of segment s, start[s] = rows[0] + .. + rows[s - 1].  For one frame in the order root, body, jaw, leye, reye,
 * lhand, rhand (1, 21, 1, 1, 1, 15, 15 rows) `packed` is the [55, 3] pose of exa_mesh_kinematics_forward.
 *
 * Forward, per row a = (a1, a2) of six floats; every operation rounded in fp32, no fused multiply-add, in this order
 * (eps = 1e-12, F.normalize's):
 *   1. rotation_6d_to_matrix:
 *        n1 = sqrt((a1_0 a1_0 + a1_1 a1_1) + a1_2 a1_2);  d1 = max(n1, eps);  b1 = a1 / d1
 *        dot = (b1_0 a2_0 + b1_1 a2_1) + b1_2 a2_2;  c = a2 - dot b1
 *        n2, d2 of c likewise;  b2 = c / d2;  b3 = b1 x b2 = (b1_1 b2_2 - b1_2 b2_1, b1_2 b2_0 - b1_0 b2_2,
 *        b1_0 b2_1 - b1_1 b2_0);  m = rows (b1, b2, b3)
 *   2. matrix_to_quaternion:
 *        x0 = ((1 + m00) + m11) + m22;  x1 = ((1 + m00) - m11) - m22;  x2 = ((1 - m00) + m11) - m22;
 *        x3 = ((1 - m00) - m11) + m22;  i = the LOWEST index of the largest x;  q = sqrt(x_i);  qq = q q;  D = 2 q
 *        A = m21 - m12, B = m02 - m20, C = m10 - m01, E = m10 + m01, F = m02 + m20, G = m12 + m21
 *        row = (qq, A, B, C) | (A, qq, E, F) | (B, E, qq, G) | (C, F, G, qq) for i = 0 | 1 | 2 | 3
 *        quat = row / D, negated as a whole when its first element is < 0.  (x_i >= 1, so neither the 0.1 floor nor
 *        the positive part of pytorch3d's formula can bind.)  Steps 1 and 2 are exa_raster_scene_assets_forward's, bit
 *        for bit; `quat` = (w, x, y, z) is written when asked for.
 *   3. quaternion_to_axis_angle:
 *        n = sqrt((x x + y y) + z z);  half = atan2(n, w);  angle = 2 half
 *        s = sin(half) / angle, or 0.5 - (angle angle) / 48 when |angle| < 1e-6
 *        out = (x / s, y / s, z / s)
 *      atan2 and sin are the device library's atan2f / sinf: the steps a CPU does not reproduce bit for bit.
 *
 * Backward, atomic-free and bit-deterministic; everything is recomputed from the 6D row.  The row's cotangent g:
 * grad_out[s]'s row when only that is given, grad_packed's when only that is, grad_out + grad_packed (one rounded
 * addition) when both are, +0 when neither is.  torch's conventions: no gradient through the candidate index, the sign
 * flip or the choice of the series; norm's gradient is 0 at 0; clamp_min passes the gradient where n >= eps.
 *   T = (g_0 x + g_1 y) + g_2 z;  gs = -(T / (s s))
 *   series:  g_angle = -(gs (angle / 24));           g_half = 2 g_angle
 *   else:    g_angle = -(gs (s / angle));            g_half = 2 g_angle + (gs / angle) cos(half)      (cosf)
 *   den = n n + w w;  gn = g_half (w / den);  gw = -(g_half (n / den));  k = gn / n, or 0 when n == 0
 *   g_quat = (gw, g_0 / s + x k, g_1 / s + y k, g_2 / s + z k)
 *   then the backward of steps 2 and 1 exactly as exa_raster_scene_assets_backward states it for the quaternion's
 *   cotangent (exa_raster.h), giving the six floats of grad_d6's row.
 * The identity row (1, 0, 0, 0, 1, 0) therefore gets the finite gradient (0, -1, 1, 0, 0, -1) for g = (1, 1, 1).
 * Nothing is summed across rows: no workspace.
 *
 * exa_mesh_pose_features: from the kinematics' rot [J, 3, 3], the two detached features of module.py:464,484,498:
 *   pose6d[6 j + k] = rot[1 + j] element k, k = 0 .. 5 (its first two rows: matrix_to_rotation_6d), j = 0 .. n_body - 1
 *   pose_feat[9 j + k] = rot[1 + j] element k - (1 when k is 0, 4 or 8, else 0), j = 0 .. J - 2     (rot[1:] - I) */
#define EXA_MESH_POSE_MAX_SEGMENTS 64
#define EXA_MESH_POSE_MAX_ROWS (1 << 24)  /* R */

/* One launch.  rows HOST int32 [n_seg]; d6 HOST [n_seg] of [dev] [rows[s], 6]; out HOST [n_seg] of [dev] [rows[s], 3],
 * or NULL, and any entry may be NULL (not wanted); packed [dev] [R, 3] or NULL; quat [dev] [R, 4] or NULL.  What is
 * given is fully written; with nothing wanted there is no launch. */
int exa_mesh_pose_params_forward(int32_t n_seg, const int32_t* rows, const float* const* d6, float* const* out,
                                 float* packed, float* quat, void* stream);

/* One launch.  rows, d6 as in the forward; grad_out HOST [n_seg] of [dev] [rows[s], 3] or NULL, entries may be NULL;
 * grad_packed [dev] [R, 3] or NULL; grad_d6 HOST [n_seg] of [dev] [rows[s], 6]: a NULL entry is a segment whose
 * gradient is not wanted, and nothing is computed for it; the others are fully written.  All entries NULL: no launch. */
int exa_mesh_pose_params_backward(int32_t n_seg, const int32_t* rows, const float* const* d6,
                                  const float* const* grad_out, const float* grad_packed, float* const* grad_d6,
                                  void* stream);

/* One launch, forward only.  rot [dev] [J, 3, 3] (1 <= J <= EXA_MESH_KIN_MAX_JOINTS), 0 <= n_body <= J - 1;
 * pose6d [dev] [6 n_body] and pose_feat [dev] [9 (J - 1)], either may be NULL. */
int exa_mesh_pose_features(int32_t J, int32_t n_body, const float* rot, float* pose6d, float* pose_feat, void* stream);

/* ---- Mesh upsampling (reference upsample_mesh: pytorch3d SubdivideMeshes.subdivide_homogeneous, once or twice) -----
 * One round appends, after the V vertices of a mesh, one vertex per unique edge, in ascending order of (low, high) (the
 * edge's two vertex indices sorted); a face (v0, v1, v2) with the midpoints (m0 opposite v0: edge (v1, v2); m1: edge
 * (v2, v0); m2: edge (v0, v1)) becomes (v0, m2, m1), (v1, m0, m2), (v2, m1, m0), (m0, m1, m2), the four groups of all
 * faces concatenated in that order.  `levels` rounds (1 or 2) take V0 vertices to V1 = V0 + E0 and Vn = V1 + E1
 * (Vn = V1 with one round).  The plan is flat:
 *   par  [Vn - V0, 2] int32  the two parents (low, high) of fine vertex V0 + i: indices below V0 for i < V1 - V0 (a
 *                            round-1 vertex), indices below V1 for the others (a round-2 vertex).
 *   off1 [V0 + 1], dep1 [2 (V1 - V0)]  CSR: for every vertex p < V0 its dependants, the round-1 vertices d (V0 <= d <
 *                            V1) that have p as a parent, ascending d (a vertex whose two parents are both p is
 *                            listed twice).  off2 [V1 + 1], dep2 [2 (Vn - V1)]: the same for round 2 over p < V1 and
 *                            V1 <= d < Vn.  The order is a function of the topology alone.
 * Forward, one launch, x [V0, C] -> out [Vn, C] (1 <= C <= EXA_MESH_UP_MAX_CHANNELS), every operation rounded in fp32:
 *   out[i] = x[i]                                 i < V0
 *   out[i] = (val(a) + val(b)) * 0.5              (a, b) = par[i - V0];  val(p) = x[p] for p < V0, and for a round-1
 *                                                 parent p the same expression over its own parents, recomputed in
 *                                                 the thread (no second launch, no grid dependency)
 * -- bit for bit what two `mean`s over two elements give.
 * Backward, `levels` launches, no atomics.  With g [Vn, C]:
 *   two rounds:  h[p] = g[p], then for d in p's round-2 dependants in order: h[p] = h[p] + g[d] * 0.5     (p < V1)
 *   one round:   h = g
 *   dx[v] = h[v]  (g_extra[v] + h[v] with a g_extra), then for d in v's round-1 dependants in order:
 *           dx[v] = dx[v] + h[d] * 0.5                                                                      (v < V0)
 * h is staged in the caller's workspace: V1 * C floats with two rounds, nothing with one.
 * exa_mesh_upsample_plan is where every index is checked; the kernels still bound every offset and index they read from
 * the plan (a parent outside its level gives NaN, a dependant or an offset outside its array is skipped), so no plan can
 * make them read out of range. */
#define EXA_MESH_UP_MAX_CHANNELS 8
#define EXA_MESH_UP_MAX_VERTS (1 << 26)   /* Vn */

typedef struct ExaMeshUpsample {
    int32_t levels;                     /* 1 or 2 */
    int32_t V0, V1, Vn;                 /* Vn == V1 with one round */
    const int32_t* par;                 /* [dev] [Vn - V0, 2] */
    const int32_t* off1;                /* [dev] [V0 + 1] */
    const int32_t* dep1;                /* [dev] [2 (V1 - V0)] */
    const int32_t* off2;                /* [dev] [V1 + 1]; unused with one round */
    const int32_t* dep2;                /* [dev] [2 (Vn - V1)]; unused with one round */
} ExaMeshUpsample;

/* Host only: builds the plan of `levels` rounds over `faces` [F0, 3] (every index must lie in [0, V0):
 * EXA_MESH_E_INVALID with a message naming the first that does not).  counts [3] receives V1, Vn and Fn = 4^levels F0.
 * The output arrays are HOST memory, all given or all NULL (NULL: only the counts, to size them): par [Vn - V0, 2],
 * faces_out [Fn, 3], off1 [V0 + 1], dep1 [2 (V1 - V0)], and with two rounds off2 [V1 + 1], dep2 [2 (Vn - V1)]. */
int exa_mesh_upsample_plan(int32_t V0, int32_t F0, const int32_t* faces, int32_t levels, int32_t* counts, int32_t* par,
                           int32_t* faces_out, int32_t* off1, int32_t* dep1, int32_t* off2, int32_t* dep2);

/* One launch.  up HOST pointer (its arrays [dev]); x [dev] [V0, C]; out [dev] [Vn, C], fully written. */
int exa_mesh_upsample_forward(const ExaMeshUpsample* up, int32_t C, const float* x, float* out, void* stream);

/* `levels` launches.  g [dev] [Vn, C]; g_extra [dev] [V0, C] or NULL; ws [dev] of ws_bytes >= 4 V1 C with two rounds
 * (NULL with one); dx [dev] [V0, C], fully written. */
int exa_mesh_upsample_backward(const ExaMeshUpsample* up, int32_t C, const float* g, const float* g_extra, void* ws,
                               uint64_t ws_bytes, float* dx, void* stream);

/* ---- SMPL-X template stage (reference get_neutral_pose_human(True, True) + get_zero_pose_human) ---------------------
 * What the reference computes with two `smplx_layer` forwards, a third `batch_rigid_transform` and two mesh
 * subdivisions, as one stage.  Both poses are constants there (the big pose and its inverse; zero), so their rotations
 * and pose-corrective offsets are data; what varies is coef [L] (shape, and expression if its directions are
 * concatenated) and joint_offset [J, 3].  V vertices, 1 <= L <= EXA_MESH_BODY_MAX_COEF, 1 <= J <=
 * EXA_MESH_KIN_MAX_JOINTS.  Every operation is rounded in fp32 and never contracted; every sum runs in an order that
 * depends on the sizes and the tables alone.  With m = 3 v + c:
 *   s = +0.0; for l = 0 .. L-1 in order: s = s + coef[l] * dirs[l][m];   v_shaped[m] = v_base[m] + s
 *       (v_base = v_template + face_offset, added once by the caller; dirs is feature-major [L, 3 V])
 *   v_posed[m] = v_shaped[m] + pose_offsets[m]                    (v_posed = v_shaped without pose_offsets)
 *   Jr[j][c]: row j of the joint regressor travels compacted to its n_j non-zeros (jreg_off / jreg_col / jreg_val, a
 *       CSR in ascending vertex order).  Lane t of 64 forms p_t = +0.0, then for i = t, t + 64, .. < n_j in order
 *       p_t = p_t + val[i] * v_shaped[col[i]][c]; the 64 lanes are added as a tree, for off = 32, 16, 8, 4, 2, 1 in
 *       order p_i = p_i + p_(i+off) for i < off; Jr[j][c] = p_0 + joint_offset[j][c] for j != root, p_0 for j == root.
 *   chain A = exa_mesh_kinematics_forward(rot_in = rot_pose, joints = Jr): joint_neutral_pose (its posed joints), A
 *   mesh = exa_skin_forward(points = v_posed, T = A, weights, no idx, trans = +0.0, no camera step)
 *   mesh_upsampled = the upsampling above of mesh (C = 3)
 *   chain B = exa_mesh_kinematics_forward(rot_in = rot_inverse, joints = joint_neutral_pose): transform_mat_neutral_pose
 *   chain C = exa_mesh_kinematics_forward(rot_in = rot_identity, joints = Jr): joint_zero_pose (its posed joints)
 * Seven launches.
 *
 * Backward, at most ten launches, no atomics.  Any of the five cotangents may be NULL (none); a step nothing reaches is
 * not launched.
 *   gB = grad_joints of exa_mesh_kinematics_backward(chain B; grad_transforms = g_transform_mat)
 *   gm = the upsampling's backward (g = g_mesh_upsampled, g_extra = g_mesh);  gm = g_mesh without g_mesh_upsampled
 *   exa_skin_backward(points = v_posed, grad_out = gm): grad_points = g_vp, grad_T = g_A
 *   g_pA = g_joint_neutral_pose + gB (one of them alone where the other is missing)
 *   gJA = grad_joints of exa_mesh_kinematics_backward(chain A; grad_transforms = g_A, grad_posed_joints = g_pA)
 *   gJC = grad_joints of exa_mesh_kinematics_backward(chain C; grad_posed_joints = g_joint_zero_pose)
 *   dJ[j][c] = gJA + gJC (one alone where the other is missing, +0.0 without both)
 *   dL_djoint_offset[j] = dJ[j] for j != root, +0.0 for j == root
 *   dvs[v][c] = g_vp[v][c] (+0.0 without gm), then for every non-zero (j, v) of the regressor in ascending j
 *               (jregT_off / jregT_row / jregT_val, the transposed CSR): dvs = dvs + val * dJ[j][c]
 *   dL_dcoef[l]: the 3 V elements m are cut into chunks of EXA_MESH_BODY_CHUNK = 256; in a chunk lane t owns element
 *       m_t and forms q_t = dirs[l][m_t] * dvs[m_t] (+0.0 past 3 V); the 64 lanes of each of the four waves are added
 *       by the tree above, the chunk's partial is ((w_0 + w_1) + w_2) + w_3, and
 *       dL_dcoef[l] = +0.0, then for chunk = 0, 1, .. in order: dL_dcoef[l] = dL_dcoef[l] + partial[chunk][l].
 * The forward's workspace holds what the backward reads (v_posed, Jr, A) and must stay untouched until then. */
#define EXA_MESH_BODY_MAX_COEF 512
#define EXA_MESH_BODY_CHUNK 256
#define EXA_MESH_BODY_MAX_VERTS (1 << 24)   /* V */

typedef struct ExaMeshBody {
    int32_t V, L, J;                    /* vertices, coefficients, joints */
    int32_t nnz;                        /* non-zeros of the joint regressor, 0 .. J V */
    int32_t root;                       /* the joint whose joint_offset row is ignored, in [0, J) */
    const int32_t* parents;             /* HOST [J]: the tree, as exa_mesh_kinematics_* take it */
    const float* v_base;                /* [dev] [V, 3] */
    const float* dirs;                  /* [dev] [L, 3 V] feature-major */
    const float* pose_offsets;          /* [dev] [V, 3] or NULL */
    const int32_t* jreg_off;            /* [dev] [J + 1] */
    const int32_t* jreg_col;            /* [dev] [nnz] vertex of every non-zero, rows in order, ascending in a row */
    const float* jreg_val;              /* [dev] [nnz] */
    const int32_t* jregT_off;           /* [dev] [V + 1] */
    const int32_t* jregT_row;           /* [dev] [nnz] joint of every non-zero, vertices in order, ascending in one */
    const float* jregT_val;             /* [dev] [nnz] */
    const float* weights;               /* [dev] [V, J] skinning weights */
    const float* rot_pose;              /* [dev] [J, 3, 3] */
    const float* rot_inverse;           /* [dev] [J, 3, 3] */
    const float* rot_identity;          /* [dev] [J, 3, 3] identities */
    const ExaMeshUpsample* up;          /* HOST pointer; up->V0 == V */
} ExaMeshBody;

/* Host only: the bytes of the forward's and the backward's workspace, from V, L, J and up's counts alone. */
int exa_mesh_body_workspace_sizes(const ExaMeshBody* body, uint64_t* fwd_bytes, uint64_t* bwd_bytes);

/* body HOST pointer; coef [dev] [L]; joint_offset [dev] [J, 3]; fwd_ws [dev] of fwd_ws_bytes >= fwd_bytes.  Outputs,
 * each [dev], required, fully written: mesh_upsampled [Vn, 3], mesh [V, 3], joint_neutral_pose [J, 3],
 * transform_mat_neutral_pose [J, 4, 4], joint_zero_pose [J, 3]. */
int exa_mesh_body_forward(const ExaMeshBody* body, const float* coef, const float* joint_offset, void* fwd_ws,
                          uint64_t fwd_ws_bytes, float* mesh_upsampled, float* mesh, float* joint_neutral_pose,
                          float* transform_mat_neutral_pose, float* joint_zero_pose, void* stream);

/* fwd_ws, joint_neutral_pose: the forward's.  g_* [dev], shaped as the outputs, each may be NULL.  bwd_ws [dev] of
 * bwd_ws_bytes >= bwd_bytes.  dL_dcoef [dev] [L] and dL_djoint_offset [dev] [J, 3]: each may be NULL (not wanted: the
 * steps only it needs are not launched), fully written when given. */
int exa_mesh_body_backward(const ExaMeshBody* body, const void* fwd_ws, uint64_t fwd_ws_bytes,
                           const float* joint_neutral_pose, const float* g_mesh_upsampled, const float* g_mesh,
                           const float* g_joint_neutral_pose, const float* g_transform_mat_neutral_pose,
                           const float* g_joint_zero_pose, void* bwd_ws, uint64_t bwd_ws_bytes, float* dL_dcoef,
                           float* dL_djoint_offset, void* stream);

/* ---- Posed SMPL-X stage (reference Model.get_smplx_outputs, avatar/main/model.py:37-58) -----------------------------
 * The `smplx_layer` call whose pose varies per frame, one sample per call: smplx's `batch_rodrigues`, the two blend-shape
 * sums, the pose correctives, `batch_rigid_transform`, the dense skinning, `+ transl` and the camera -> world step, as
 * one C call each way.  V vertices, L = Lb + Le coefficients (1 <= L <= EXA_MESH_BODY_MAX_COEF; betas [Lb] and
 * expression [Le] are two pointers, either may be empty), 1 <= J <= EXA_MESH_KIN_MAX_JOINTS, P = 9 (J - 1) pose features.
 * It joins this ABI like the template stage whose launches it shares; no existing prototype changes: EXA_MESH_VERSION
 * stays 100.  Every operation is rounded in fp32 and never contracted; every sum runs in an order that depends on the
 * sizes and the tables alone.  With m = 3 v + c and I the identity:
 *   1. f = pose[j] + pose_mean[j]  (f = pose[j] without a pose_mean);  e = f + 1e-8f  (per component)
 *   2. a = sqrt((e_0 e_0 + e_1 e_1) + e_2 e_2);  d = f / a;  s = sin(a), c = cos(a)  (the device library's sinf / cosf:
 *      the one step a CPU does not reproduce bit for bit; both are kept for the backward);  q = 1 - c
 *      K = [0, -d_2, d_1;  d_2, 0, -d_0;  -d_1, d_0, 0];   KK[r][k] = (K[r][0] K[0][k] + K[r][1] K[1][k]) + K[r][2] K[2][k]
 *      rot[j][r][k] = (I[r][k] + s K[r][k]) + q KK[r][k]                   (smplx lbs.py:311-345, not pytorch3d's route)
 *   3. v_shaped[m] = v_base[m] + S,  S = +0.0, then for l = 0 .. L-1 in order S = S + coef[l] * dirs[l][m], coef[l] =
 *      betas[l] for l < Lb and expression[l - Lb] for the others  (v_base = v_template + face_offset, added once by the
 *      caller; dirs is feature-major [L, 3 V])
 *   4. Jr[j][c] = the template stage's regressor sum over v_shaped (lanes, then the tree) + joint_offset[j][c], for EVERY
 *      joint, the root included (model.py:50 passes the parameter as it is); without a joint_offset nothing is added
 *   5. feat[9 (j - 1) + 3 r + k] = rot[j][r][k] - I[r][k]                  j = 1 .. J-1
 *   6. v_posed[m] = v_shaped[m] + C,  C = +0.0, then for p = 0 .. P-1 in order C = C + feat[p] * posedirs[p][m]
 *      (posedirs [P, 3 V] in the layer's own layout; J == 1: v_posed = v_shaped)
 *   7. chain = exa_mesh_kinematics_forward(rot_in = rot, joints = Jr): posed joints, A
 *   8, 9. vertices = exa_skin_forward(points = v_posed, T = A, weights, no idx, trans = transl, no camera step)
 *   10. joints[j][c] = posed_joints[j][c] + transl[c]
 *   11. with Rinv and t: d = vertices[v] - t;  vertices_world[v][r] = (Rinv[r][0] d_0 + Rinv[r][1] d_1) + Rinv[r][2] d_2
 * Seven launches (six for J == 1): posed_rodrigues, body_shape, body_jreg, body_shape over posedirs, kin_fwd, skin_fwd,
 * posed_finish.
 *
 * Backward, at most ten launches, no atomics.  Any of the three cotangents may be NULL (none); a step nothing reaches,
 * or that only unwanted gradients need, is not launched.
 *   gv[v][c] = g_vertices[v][c] + ((Rinv[0][c] g_0 + Rinv[1][c] g_1) + Rinv[2][c] g_2),  g = g_vertices_world[v]  (one of
 *              them alone where the other is missing)
 *   exa_skin_backward(points = v_posed, grad_out = gv): grad_points = g_vp, grad_T = g_A, grad_trans = g_tr
 *   exa_mesh_kinematics_backward(chain; grad_transforms = g_A, grad_posed_joints = g_joints): grad_rot = g_R,
 *              grad_joints = g_J
 *   dL_djoint_offset = g_J  (+0.0 where nothing reaches the chain)
 *   dvs[v][c] = g_vp[v][c] (+0.0 without gv), then the regressor's transpose over g_J as in the template stage
 *   dL_dbetas, dL_dexpression: the template stage's two-level sum of dirs[l][m] * dvs[m] over chunks of
 *              EXA_MESH_BODY_CHUNK, for the rows of the wanted tensors only
 *   g_feat[p] = the same two-level sum of posedirs[p][m] * g_vp[m]: the correctives' transpose, 3 V terms per feature
 *   G = g_R[j] + g_feat[9 (j - 1) ..] (one alone where the other is missing or j == 0, +0.0 without both), then with s, c
 *   of the forward and f, e, a, d, K, KK recomputed as above:
 *       g_s = +0.0, then for k = 0 .. 8 (row-major) in order g_s = g_s + G[k] K[k];   g_q likewise over KK
 *       X[r][k] = (G[r][0] K[k][0] + G[r][1] K[k][1]) + G[r][2] K[k][2];   Y[r][k] = (K[0][r] G[0][k] + K[1][r] G[1][k]) +
 *       K[2][r] G[2][k];   g_K[r][k] = s G[r][k] + q (X[r][k] + Y[r][k])
 *       g_d = (g_K[2][1] - g_K[1][2],  g_K[0][2] - g_K[2][0],  g_K[1][0] - g_K[0][1])
 *       g_a = (g_s c + g_q s) - ((g_d0 d_0 + g_d1 d_1) + g_d2 d_2) / a
 *       dL_dpose[j][k] = g_d[k] / a + g_a (e_k / a)
 *   The 1e-8 keeps a > 0 at a zero row, whose gradient is therefore finite.
 *   dL_dtransl[c] = g_tr[c] + T,  T = +0.0, then for j = 0 .. J-1 in order T = T + g_joints[j][c]  (one alone where the
 *              other is missing)
 * The forward's workspace holds what the backward reads (sin / cos, rot, v_posed, Jr, A) and must stay untouched until
 * then; its first 2 J floats are (sin a_j, cos a_j).  pose_mean, face_offset and the camera get no gradient. */
typedef struct ExaMeshPosed {
    int32_t V, L, J;                    /* vertices, coefficients (Lb + Le), joints */
    int32_t nnz;                        /* non-zeros of the joint regressor, 0 .. J V */
    const int32_t* parents;             /* HOST [J]: the tree, as exa_mesh_kinematics_* take it */
    const float* v_base;                /* [dev] [V, 3] */
    const float* dirs;                  /* [dev] [L, 3 V] feature-major */
    const float* posedirs;              /* [dev] [9 (J - 1), 3 V]; unused with J == 1 */
    const float* pose_mean;             /* [dev] [J, 3] or NULL */
    const int32_t* jreg_off;            /* [dev] [J + 1]; the six regressor arrays as in ExaMeshBody */
    const int32_t* jreg_col;            /* [dev] [nnz] */
    const float* jreg_val;              /* [dev] [nnz] */
    const int32_t* jregT_off;           /* [dev] [V + 1] */
    const int32_t* jregT_row;           /* [dev] [nnz] */
    const float* jregT_val;             /* [dev] [nnz] */
    const float* weights;               /* [dev] [V, J] skinning weights */
} ExaMeshPosed;

/* Host only: the bytes of the forward's and the backward's workspace, from V, L and J alone. */
int exa_mesh_posed_workspace_sizes(const ExaMeshPosed* posed, uint64_t* fwd_bytes, uint64_t* bwd_bytes);

/* posed HOST pointer; 0 <= Lb <= L; pose [dev] [J, 3]; betas [dev] [Lb] and expression [dev] [L - Lb] (NULL where
 * empty); transl [dev] [3]; joint_offset [dev] [J, 3] or NULL; Rinv [dev] [3, 3] and t [dev] [3], both or neither; fwd_ws
 * [dev] of fwd_ws_bytes >= fwd_bytes.  Outputs, each [dev], fully written: vertices [V, 3], joints [J, 3], rot [J, 3, 3]
 * (required) and vertices_world [V, 3] (given exactly when Rinv is).  Everything is validated on the host before any
 * GPU work. */
int exa_mesh_posed_forward(const ExaMeshPosed* posed, int32_t Lb, const float* pose, const float* betas,
                           const float* expression, const float* transl, const float* joint_offset, const float* Rinv,
                           const float* t, void* fwd_ws, uint64_t fwd_ws_bytes, float* vertices, float* joints,
                           float* vertices_world, float* rot, void* stream);

/* pose, Rinv, fwd_ws: the forward's.  g_* [dev], shaped as the outputs, each may be NULL.  bwd_ws [dev] of bwd_ws_bytes
 * >= bwd_bytes.  dL_dpose [J, 3], dL_dbetas [Lb], dL_dexpression [L - Lb], dL_dtransl [3], dL_djoint_offset [J, 3]: each
 * [dev], each may be NULL (not wanted: the steps only it needs are not launched), fully written when given.  With none
 * wanted there is no launch. */
int exa_mesh_posed_backward(const ExaMeshPosed* posed, int32_t Lb, const float* pose, const float* Rinv,
                            const void* fwd_ws, uint64_t fwd_ws_bytes, const float* g_vertices, const float* g_joints,
                            const float* g_vertices_world, void* bwd_ws, uint64_t bwd_ws_bytes, float* dL_dpose,
                            float* dL_dbetas, float* dL_dexpression, float* dL_dtransl, float* dL_djoint_offset,
                            void* stream);

/* ---- Arm and hand regularisers (reference ArmRGBReg, HandRGBReg, HandMeanReg, loss.py:148-197) -----------------------
 * Three more per-vertex losses of the upsampled mesh, V vertices, B batch elements, three channels.  Every operation
 * is rounded in fp32 and never contracted; every sum runs in the order stated here.  No atomics, no memset: every
 * output element is written by the launch that owns it.  Masks are bytes (0 = out, anything else = in).
 *
 * ARM.  is_upper / is_lower [V] select U upper-arm and L lower-arm vertices.  For a lower vertex l and an upper vertex u
 *   dx = x_l - x_u, dy = y_l - y_u, dz = z_l - z_u;   the pair is VALID iff |dx| < dist_x_thr  (a float32 comparison)
 *   d2 = (dx * dx + dy * dy) + dz * dz;   key(l, u) = (bits(d2), u), ordered by bits(d2), then by the vertex index u.
 *       bits(d2) is the IEEE pattern of d2 as an unsigned integer -- d2 >= +0, so that is its numeric order -- and
 *       0x7fc00000 for a NaN, which therefore sorts after +inf.  No square root is taken: it is monotone, so it can
 *       only merge neighbouring keys into ties; the reference's 9999 sentinel of an invalid pair never wins, because
 *       k <= n_min.
 *   n_l = number of valid u;   n_min = min over the lower vertices of n_l (0 when L == 0);   k = min(K_max, n_min)
 *   target[b,l,c] = t / (float)k  where  t = +0.0, then for the k smallest keys of l in ascending order:
 *                   t = t + rgb[b, u, c].    k == 0 gives 0 / 0 = NaN, the reference's mean over an empty set; it
 *                   is not trapped.
 *   d = rgb[b,l,c] - target;   loss[b,l,c] = d * d;   every vertex outside the lower list: loss = d = +0.0
 *   backward: dL_drgb[b,l,c] = (2 * d) * grad_loss[b,l,c];  +0.0 for every vertex outside the lower list.  The target
 *   is detached and the mesh gets no gradient (in the reference it reaches only the indices).
 * The lists are in ascending vertex order; the result does not depend on that, the key carries the index.
 *
 * HAND RGB.  Two lists r_idx, l_idx [N] (the right and the left hand's vertices, ascending) and their inverse ranks
 * r_rank, l_rank [V] (position in the list, -1 outside).
 *   mean_r[b,c]: the list is cut into chunks of EXA_MESH_REG_CHUNK = 256 rows; partial[chunk] = +0.0, then for the
 *       chunk's rows i in list order partial = partial + rgb[b, r_idx[i], c];  s = +0.0, then for chunk = 0, 1, .. in
 *       order s = s + partial[chunk];  mean_r = s / (float)N.   mean_l the same over l_idx.
 *   loss[b,i,c] = dr * dr + dl * dl,   dr = rgb[b, r_idx[i], c] - mean_r[b,c],  dl = rgb[b, l_idx[i], c] - mean_l[b,c]
 *   backward (the means are detached), per vertex v through the ranks, ir = r_rank[v], il = l_rank[v]:
 *       tr = grad_loss[b,ir,c] * (2 * (rgb[b,v,c] - mean_r[b,c]));   tl = grad_loss[b,il,c] * (2 * (rgb[b,v,c] - mean_l[b,c]))
 *       dL_drgb[b,v,c] = tr + tl in both lists, tr or tl alone in one, +0.0 in neither.
 *
 * HAND MEAN.  h_idx [H] (the union of the hands, ascending) and its inverse ranks h_rank [V]; normal [V, 3].  With
 * o = offset[b,v,:], n = normal[v,:], v = h_idx[j]:
 *   norm = sqrt((o0 * o0 + o1 * o1) + o2 * o2);   s = norm < 1e-12f ? 1e-12f : norm;   q_c = o_c / s
 *   dot = (n0 * q0 + n1 * q1) + n2 * q2;   loss[b,j] = dot < 0 ? +0.0 : dot      (a NaN stays a NaN in both selects)
 *   backward, torch's for normalize and clamp: g = dot >= 0 ? grad_loss[b,j] : 0 (the gradient passes at equality);
 *       dq_c = g * n_c;   a_c = dq_c / s;
 *       norm >= 1e-12f:  t = (dq0 * (q0 / s) + dq1 * (q1 / s)) + dq2 * (q2 / s);  w = (-t) / norm;
 *                        dL_doffset[b,v,c] = a_c + o_c * w
 *       otherwise:       dL_doffset[b,v,c] = a_c        (a zero row gets g * n_c / 1e-12f, which is finite)
 *       +0.0 for every vertex outside the list.  normal gets no gradient.
 * A list entry outside [0, V) reads nothing and contributes NaN.  B == 0 or an empty list is a successful no-op where
 * nothing is left to write. */
#define EXA_MESH_ARM_MAX_K 64           /* K_max: one key per lane of a wave */
#define EXA_MESH_ARM_WAVES 8            /* lower vertices per workgroup of the selection */
#define EXA_MESH_ARM_TILE 1024          /* upper records staged in LDS at a time */
#define EXA_MESH_ARM_HEADER_INTS 4      /* header: U, L, k, n_min */
#define EXA_MESH_REG_CHUNK 256

/* The neighbour plan of one mesh: three launches (compaction by one workgroup; selection, one wave per lower vertex,
 * the grid sized by `rows`; the reduction of the counts to k).  mesh [dev] [V, 3]; is_upper, is_lower [dev] [V] bytes;
 * rows = the caller's bound on L, 0 .. V (V is always safe): a lower vertex of rank >= rows is not selected for and
 * gets NaN in the loss, and n_min runs over the first min(L, rows) lower vertices.  1 <= K_max <= 64; dist_x_thr finite
 * and > 0.  Outputs, all [dev]: upper_rec, lower_rec [V, 4] fp32 records {x, y, z, index bits} (16-byte aligned, the
 * first U and L written); lower_rank [V] int32, fully written; nbr [rows, K_max] int32 (row r < L: the indices of its
 * K_max smallest keys in ascending key order, -1 where it has fewer); n_valid [rows] (n_l, rows < L); wg_min
 * [ceil(rows / EXA_MESH_ARM_WAVES)] scratch; header [EXA_MESH_ARM_HEADER_INTS] int32 {U, L, k, n_min}, fully written.
 * Nothing is read back: U, L and k stay on the device. */
int exa_mesh_arm_plan(int32_t V, int32_t rows, int32_t K_max, float dist_x_thr, const float* mesh,
                      const uint8_t* is_upper, const uint8_t* is_lower, float* upper_rec, float* lower_rec,
                      int32_t* lower_rank, int32_t* nbr, int32_t* n_valid, int32_t* wg_min, int32_t* header,
                      void* stream);

/* One launch.  rgb [dev] [B, V, 3]; lower_rank, nbr, header: the plan's (rows, K_max as there); loss, d [dev] [B, V, 3],
 * fully written (d is what the backward reads). */
int exa_mesh_arm_loss_forward(int32_t B, int32_t V, int32_t rows, int32_t K_max, const float* rgb,
                              const int32_t* lower_rank, const int32_t* nbr, const int32_t* header, float* loss, float* d,
                              void* stream);

/* One launch.  d [dev] the forward's; grad_loss [dev] [B, V, 3]; dL_drgb [dev] [B, V, 3], fully written. */
int exa_mesh_arm_loss_backward(int32_t B, int32_t V, const float* d, const float* grad_loss, const int32_t* lower_rank,
                               float* dL_drgb, void* stream);

/* Bytes of the hand-rgb forward's workspace (the chunk partials). */
int exa_mesh_hand_rgb_workspace_size(int32_t B, int32_t N, uint64_t* out_bytes);

/* Two launches.  rgb [dev] [B, V, 3]; r_idx, l_idx [dev] [N]; ws [dev] of ws_bytes >= the size above; means [dev]
 * [B, 2, 3] (right, left; what the backward reads) and loss [dev] [B, N, 3], fully written. */
int exa_mesh_hand_rgb_forward(int32_t B, int32_t V, int32_t N, const float* rgb, const int32_t* r_idx,
                              const int32_t* l_idx, void* ws, uint64_t ws_bytes, float* means, float* loss, void* stream);

/* One launch.  means [dev] the forward's; grad_loss [dev] [B, N, 3]; r_rank, l_rank [dev] [V]; dL_drgb [dev]
 * [B, V, 3], fully written. */
int exa_mesh_hand_rgb_backward(int32_t B, int32_t V, int32_t N, const float* rgb, const float* means,
                               const float* grad_loss, const int32_t* r_rank, const int32_t* l_rank, float* dL_drgb,
                               void* stream);

/* One launch.  offset [dev] [B, V, 3]; normal [dev] [V, 3]; h_idx [dev] [H]; loss [dev] [B, H], fully written. */
int exa_mesh_hand_mean_forward(int32_t B, int32_t V, int32_t H, const float* offset, const float* normal,
                               const int32_t* h_idx, float* loss, void* stream);

/* One launch.  grad_loss [dev] [B, H]; h_rank [dev] [V]; dL_doffset [dev] [B, V, 3], fully written. */
int exa_mesh_hand_mean_backward(int32_t B, int32_t V, int32_t H, const float* offset, const float* normal,
                                const float* grad_loss, const int32_t* h_rank, float* dL_doffset, void* stream);

/* ---- Gaussian offset and joint offset regularisers (reference model.py:217-232, 253-257, loss.py:133-146) ------------
 * The four remaining terms of the loss block: two over the B V rows of the upsampled mesh, two over the J joints.  Every
 * operation is rounded in fp32 and never contracted; every sum runs in the order stated here.  No atomics, no memset:
 * every output element is written by the launch that owns it.
 *
 * TERMS.  Row i = b V + v, channel c = 0, 1, 2; a = mean_offset, b = mean_offset_offset, z = scale, all [B, V, 3];
 * u = scale_offset, [B, V, 1] (the one value of the row serves its three channels) or [B, V, 3]; w_mean, w_scale [V].
 *   0  mean_map[i,c]  = ((a * a) + (b * b)) * w_mean[v]                                       N_0 = 3 B V
 *   1  scale_map[i,c] = ((z * z) + (u * u)) * w_scale[v]                                      N_1 = 3 B V
 * jo = joint_offset, ref = joint_ref, wj = w_joint, all [J, 3], element e = 3 j + c; pair p = (r, l) = (pair_r[p], pair_l[p]):
 *   2  joint_map[e]   = ((jo[e] - ref[e]) * (jo[e] - ref[e])) * wj[e]                         N_2 = 3 J
 *   3  sym_map[p]     = (|jo[r,0] + jo[l,0]| + |jo[r,1] - jo[l,1]|) + |jo[r,2] - jo[l,2]|     N_3 = n_pairs
 *      A pair index outside [0, J) reads nothing and gives NaN.
 *
 * MEANS.  WG(s) is the workgroup sum of 256 threads' values s: inside each wave of 64 lanes a butterfly over the lane
 * distances 32, 16, 8, 4, 2, 1 (s = s + s[lane ^ distance]), then ((wave 0 + wave 1) + wave 2) + wave 3.
 *   Terms 0, 1: the rows are cut into exa_mesh_offset_regs_blocks(B, V) = ceil(B V / 256) workgroups of
 *       EXA_MESH_OFFSET_ROWS = 256 consecutive rows, one row per thread: row sum = (t[i,0] + t[i,1]) + t[i,2], +0.0 for a
 *       thread past the last row; partial[k][g] = WG(row sums) of workgroup g.  Then thread j of ONE workgroup:
 *       s = +0.0, then s = s + partial[k][j], partial[k][j + 256], .. in that order; sum_k = WG(s).
 *   Term 2: thread j: s = +0.0, then s = s + joint_map[j], joint_map[j + 256], ..; sum_2 = WG(s).  Term 3 the same
 *       over sym_map.
 *   means[k] = sum_k / (float)N_k.   N_k == 0 gives 0 / 0 = NaN, as torch.mean of an empty tensor does.
 *
 * BACKWARD.  The cotangent of element x of term k is g = dL_dmaps[k][x], or in mean mode g = *dL_dmeans[k] * (1 / (float)N_k):
 * the reciprocal is rounded first, as torch's backward of .mean() does on the device.  dL_dmeans[k] points to DEVICE
 * memory: nothing is read back.
 *   dL_dmean_offset[i,c]        = (g0 * w_mean[v]) * (2 * a)        (torch's MulBackward, then PowBackward)
 *   dL_dmean_offset_offset[i,c] = (g0 * w_mean[v]) * (2 * b)
 *   dL_dscale[i,c]              = (g1 * w_scale[v]) * (2 * z)
 *   dL_dscale_offset, [B, V, 3]: (g1 * w_scale[v]) * (2 * u[i,c]);
 *                     [B, V, 1]: r = ((g1[i,0] * w + g1[i,1] * w) + g1[i,2] * w), w = w_scale[v];  r * (2 * u[i])
 *                                (the broadcast is summed first and the power rule applied to the sum, as torch does)
 *   dL_djoint_offset[e] = d_reg + d_sym;   d_reg = (g2 * wj[e]) * (2 * (jo[e] - ref[e]));   for the pair p of joint j,
 *       found through joint_pair[j] = 2 p + side (side 0: j = pair_r[p], 1: j = pair_l[p]; -1: in no pair), with
 *       sign(x) = (x > 0) - (x < 0), so sign(0) = 0:
 *         c = 0:     d_sym = sign(jo[r,0] + jo[l,0]) * g3            on either side
 *         c = 1, 2:  d_sym = sign(jo[r,c] - jo[l,c]) * g3            on the right side, its negation on the left
 *       A joint in no pair gets d_reg alone, and d_sym alone where term 2 has no cotangent.
 * A term without a cotangent (its entry NULL) contributes nothing: the gradients that only it reaches are written +0.0.
 * Every requested gradient is written whole; the caller clears nothing. */
#define EXA_MESH_OFFSET_ROWS 256        /* rows per workgroup of the vertex launch = rows per partial */

/* The partials per term of the vertex launch in mean mode: ceil(B V / 256); 0 for an empty or invalid shape. */
int64_t exa_mesh_offset_regs_blocks(int32_t B, int32_t V);

/* Host only.  pair_r, pair_l [host] [n_pairs]: checks every index against [0, J) and that no joint is named twice
 * (EXA_MESH_E_INVALID), and writes joint_pair [host] [J], the inverse table the backward reads. */
int exa_mesh_offset_regs_pair_table(int32_t J, int32_t n_pairs, const int32_t* pair_r, const int32_t* pair_l,
                                    int32_t* joint_pair);

/* One launch: terms 0 and 1.  mean_offset, mean_offset_offset, scale [dev] [B, V, 3]; scale_offset [dev]
 * [B, V, scale_offset_channels], 1 or 3 channels; w_mean, w_scale [dev] [V].  Map mode: mean_map, scale_map [dev]
 * [B, V, 3], fully written, partials NULL.  Mean mode: both maps NULL, partials [dev] [2, exa_mesh_offset_regs_blocks],
 * fully written.  Both or neither is EXA_MESH_E_INVALID.  B V == 0 is a successful no-op. */
int exa_mesh_offset_regs_vertex_forward(int32_t B, int32_t V, int32_t scale_offset_channels, const float* mean_offset,
                                        const float* mean_offset_offset, const float* scale, const float* scale_offset,
                                        const float* w_mean, const float* w_scale, float* mean_map, float* scale_map,
                                        float* partials, void* stream);

/* One launch of one workgroup: terms 2 and 3 and, in mean mode, the four means.  joint_offset, joint_ref, w_joint [dev]
 * [J, 3]; pair_r, pair_l [dev] [n_pairs] int32, n_pairs <= J / 2.  Map mode: joint_map [dev] [J, 3] and sym_map [dev]
 * [n_pairs], fully written, means NULL.  Mean mode: both maps NULL, partials [dev] the vertex launch's for the same
 * B, V (not read when B V == 0), means [dev] [4], fully written.  Both or neither is EXA_MESH_E_INVALID. */
int exa_mesh_offset_regs_joint_forward(int32_t B, int32_t V, int32_t J, int32_t n_pairs, const float* joint_offset,
                                       const float* joint_ref, const float* w_joint, const int32_t* pair_r,
                                       const int32_t* pair_l, float* joint_map, float* sym_map, const float* partials,
                                       float* means, void* stream);

/* One launch.  The inputs as in the forward; joint_pair [dev] [J] the table of exa_mesh_offset_regs_pair_table.
 * dL_dmaps, dL_dmeans: HOST arrays of four device pointers, indexed by term; either may be NULL, and so may any entry.
 * Entries of both kinds, or no entry at all, is EXA_MESH_E_INVALID.  dL_dmaps[k] has the shape of term k's map;
 * dL_dmeans[k] points to one float.  The five gradients [dev] have the shapes of their inputs; a NULL one is not
 * computed, and with none left to write there is no launch.  Inputs that no requested gradient reads may be NULL. */
int exa_mesh_offset_regs_backward(int32_t B, int32_t V, int32_t scale_offset_channels, int32_t J, int32_t n_pairs,
                                  const float* mean_offset, const float* mean_offset_offset, const float* scale,
                                  const float* scale_offset, const float* w_mean, const float* w_scale,
                                  const float* joint_offset, const float* joint_ref, const float* w_joint,
                                  const int32_t* pair_r, const int32_t* pair_l, const int32_t* joint_pair,
                                  const float* const* dL_dmaps, const float* const* dL_dmeans, float* dL_dmean_offset,
                                  float* dL_dmean_offset_offset, float* dL_dscale, float* dL_dscale_offset,
                                  float* dL_djoint_offset, void* stream);

/* ---- Mesh terms of the fitting loss (reference fitting/common/nets/loss.py:73-87, 125-167, fitting/main/model.py:235-237)
 * EdgeLengthLoss, FaceOffsetSymmetricReg, PoseLoss and the centred vertex-to-vertex term.  Every operation is rounded in
 * fp32 and never contracted; every sum runs in the order stated here.  No atomics, no memset: every output element is
 * written by the launch that owns it.  sign(x) = (x > 0) - (x < 0), so sign(0) = 0.  Each backward gathers: the reference's
 * index_put_(accumulate = True) scatters are replaced by per-element sums over a transposed table built once on the host.
 *
 * EDGE LENGTH.  coord_out [B, V, 3]; coord_gt [Bt, V, 3], Bt == B or 1; valid [Bv, V], Bv == B or 1; faces [F, 3] int32.
 * Edge k of face f joins corners (a, b) = (0, 1), (0, 2), (1, 2) for k = 0, 1, 2.  For x = coord_out and x = coord_gt:
 *     dx = x[a,0] - x[b,0], dy = x[a,1] - x[b,1], dz = x[a,2] - x[b,2];   d = sqrtf((dx * dx + dy * dy) + dz * dz)
 *     loss[b, k F + f] = |d_out - d_gt| * (valid[a] * valid[b])                       ([B, 3 F]: the reference's cat order)
 *   A face may repeat a vertex: that edge has d = 0.  A face index outside [0, V) reads nothing and gives NaN (the host
 *   plan, exa_mesh_vertex_faces, refuses such a table first).
 *   Backward, one sum per (b, v, c): acc = +0.0; for every slot (f, corner) of exa_mesh_vertex_faces' CSR that names v,
 *   ascending f then corner, the two edges of that corner in ascending k (corner 0: k = 0, 1; corner 1: k = 0, 2; corner
 *   2: k = 1, 2):
 *     m = valid[a] * valid[b];   t = ((g[b, k F + f] * m) * sign(d_out - d_gt)) / d_out;   q = t * (x[a,c] - x[b,c])
 *     acc = acc + q  where v is the edge's a,   acc = acc + (-q)  where it is the edge's b
 *   AN EDGE WITH d_out == 0 CONTRIBUTES q = +0.0 (the reference divides 0 by 0 there and returns NaN: the one deliberate
 *   deviation).  A vertex in no face gets +0.0.  coord_gt and valid get no gradient.
 *
 * FLIP SYMMETRY.  p = face_offset [B, Vf, 3].  The plan (exa_mesh_flip_symmetry_plan) holds for face row i, with
 * v = face_vertex_idx[i]: tap[i,k] = the face row of vertex closest_faces[v,k], or -1 when that vertex carries no offset,
 * and w[i,k] = bc[v,k].  r_k = p[b, tap[i,k], :], or (+0.0, +0.0, +0.0) for a tap of -1 (multiplied and added like any
 * other); a tap outside [-1, Vf) reads nothing and gives NaN.
 *     f_c = (r_0[c] * w[i,0] + r_1[c] * w[i,1]) + r_2[c] * w[i,2]
 *     loss[b,i] = (|p[b,i,0] + f_0| + |p[b,i,1] - f_1|) + |p[b,i,2] - f_2|
 *   Backward, one sum per (b, i, c), with s_0(j) = sign(p[b,j,0] + f_0(j)) * g[b,j], s_c(j) = sign(p[b,j,c] - f_c(j)) * g[b,j]
 *   for c = 1, 2:  acc = s_c(i) first;  then for every (j, k) with tap[j,k] == i, ascending j then k (the plan's CSR, entry
 *   3 j + k):  acc = acc + u_c(j) * w[j,k],  u_0 = s_0(j), u_c = -s_c(j) for c = 1, 2.
 *
 * POSE.  One thread per rotation n of N: R_out = matrix(quaternion(pose_out[n])), R_gt likewise, by steps 1 of the forward
 * kinematics above (the small-angle branch below 1e-6 included); loss[n, q] = |R_out[q] - R_gt[q]|, q = 0 .. 8.  Backward:
 * G[q] = g[n, q] * sign(R_out[q] - R_gt[q]), then the analytic Jacobian of step 1 (d angle / d x := 0 at a zero row).
 * pose_gt gets no gradient.
 *
 * CENTRED V2V.  a = out, t = target [B, V, 3], w = weight [V], scale by value.  SUM2(x) over the V values of one (b, c):
 * the vertices are cut into exa_mesh_centered_v2v_blocks(V) = ceil(V / 256) workgroups of EXA_MESH_FIT_ROWS = 256
 * consecutive vertices, one per thread (+0.0 past the last), partial[g] = WG(values) of workgroup g (WG as defined for the
 * offset regularisers above); then thread j of a workgroup: s = +0.0, s = s + partial[j], partial[j + 256], ..; SUM2 = WG(s).
 *     ma[b,c] = SUM2(a[b,:,c]) / (float)V,  mt[b,c] = SUM2(t[b,:,c]) / (float)V        (means [B, 6]: ma, then mt)
 *     e = (a - ma) - (t - mt);   loss[b,v,c] = (|e| * w[v]) * scale
 *   Backward:  s = ((g * w[v]) * scale) * sign(e);   S[b,c] = SUM2(s[b,:,c]);   dL_dout = s - (S / (float)V).
 *   target and weight get no gradient.
 * B == 0 (and V, F, Vf, N == 0 where nothing is left to write) is a successful no-op in every call. */
#define EXA_MESH_FIT_ROWS 256           /* threads per workgroup = vertices per partial of the centred term */

/* One launch.  All [dev]; loss [B, 3 F], fully written. */
int exa_mesh_edge_length_forward(int32_t B, int32_t Bt, int32_t Bv, int32_t V, int32_t F, const float* coord_out,
                                 const float* coord_gt, const float* valid, const int32_t* faces, float* loss,
                                 void* stream);

/* One launch.  vert_offsets [dev] [V + 1], vert_entries [dev] [3 F]: exa_mesh_vertex_faces' CSR of `faces`; grad_loss
 * [dev] [B, 3 F]; dL_dcoord_out [dev] [B, V, 3], fully written. */
int exa_mesh_edge_length_backward(int32_t B, int32_t Bt, int32_t Bv, int32_t V, int32_t F, const float* coord_out,
                                  const float* coord_gt, const float* valid, const int32_t* faces,
                                  const int32_t* vert_offsets, const int32_t* vert_entries, const float* grad_loss,
                                  float* dL_dcoord_out, void* stream);

/* Host only, every array HOST memory.  face_vertex_idx [Vf]: the vertices of [0, V_full) that carry an offset, each named
 * once; closest_faces [V_full, 3] int32 and bc [V_full, 3]: the reference's flip_corr.  Writes vertex_row [V_full] (the
 * face row of every vertex, -1 for the others), taps [Vf, 3], weights [Vf, 3] and the taps' transpose offsets [Vf + 1],
 * entries [3 Vf] (entry 3 j + k, ascending; offsets[Vf] of them are written).  EXA_MESH_E_INVALID, with a message naming
 * it, for an index outside [0, V_full) in either table and for a vertex named twice in face_vertex_idx. */
int exa_mesh_flip_symmetry_plan(int32_t V_full, int32_t Vf, const int32_t* face_vertex_idx, const int32_t* closest_faces,
                                const float* bc, int32_t* vertex_row, int32_t* taps, float* weights, int32_t* offsets,
                                int32_t* entries);

/* One launch.  face_offset [dev] [B, Vf, 3]; taps, weights [dev] [Vf, 3]; loss [dev] [B, Vf], fully written. */
int exa_mesh_flip_symmetry_forward(int32_t B, int32_t Vf, const float* face_offset, const int32_t* taps,
                                   const float* weights, float* loss, void* stream);

/* One launch.  offsets, entries [dev]: the plan's CSR; grad_loss [dev] [B, Vf]; dL_dface_offset [dev] [B, Vf, 3], fully
 * written. */
int exa_mesh_flip_symmetry_backward(int32_t B, int32_t Vf, const float* face_offset, const int32_t* taps,
                                    const float* weights, const int32_t* offsets, const int32_t* entries,
                                    const float* grad_loss, float* dL_dface_offset, void* stream);

/* One launch each.  pose_out, pose_gt [dev] [N, 3]; loss, grad_loss [dev] [N, 9]; dL_dpose_out [dev] [N, 3]; fully written. */
int exa_mesh_pose_loss_forward(int64_t N, const float* pose_out, const float* pose_gt, float* loss, void* stream);
int exa_mesh_pose_loss_backward(int64_t N, const float* pose_out, const float* pose_gt, const float* grad_loss,
                                float* dL_dpose_out, void* stream);

/* The partials per (b, c) of the centred term: ceil(V / 256); 0 for V <= 0. */
int64_t exa_mesh_centered_v2v_blocks(int32_t V);

/* Two launches.  out, target [dev] [B, V, 3]; weight [dev] [V]; partials [dev] workspace of B * 6 * blocks floats, written
 * before it is read; means [dev] [B, 6] and loss [dev] [B, V, 3], fully written. */
int exa_mesh_centered_v2v_forward(int32_t B, int32_t V, const float* out, const float* target, const float* weight,
                                  float scale, float* partials, float* means, float* loss, void* stream);

/* Two launches.  means [dev] the forward's; grad_loss [dev] [B, V, 3]; partials [dev] workspace of B * 3 * blocks floats;
 * dL_dout [dev] [B, V, 3], fully written (the first launch leaves s there, the second subtracts S / V in place). */
int exa_mesh_centered_v2v_backward(int32_t B, int32_t V, const float* out, const float* target, const float* weight,
                                   float scale, const float* means, const float* grad_loss, float* partials,
                                   float* dL_dout, void* stream);

/* ---- Keypoints of the fitting (reference smplx/body_models.py:1257-1283, lbs.py:30-153, vertex_joint_selector.py:73-80;
 * fitting/main/model.py:97-117, 140-157; CoordLoss, fitting/common/nets/loss.py:9-71).  Every operation is rounded in fp32 and
 * never contracted (a landmark row's two fmaf are stated as such); every sum runs in the order stated here.  No atomics, no
 * memset: every output element is written by the
 * launch that owns it, so the same inputs give the same bits on every call.
 *
 * KEYPOINTS.  vertices [B, V, 3], joints [B, J, 3], rot [B, J, 3, 3], trans [B, 3] or NULL, focal, princpt [B, 2].  The host
 * compiles the selection into K + 1 records rec [K + 1, 4] int32 = (kind, i0, i1, i2), record K being the root:
 *     EXA_MESH_KPT_JOINT    raw = joints[b, i0]                                              (a copy)
 *     EXA_MESH_KPT_VERTEX   raw = vertices[b, i0]                                            (a copy)
 *     EXA_MESH_KPT_STATIC   raw[c] = fmaf(x[i2,c], w2, fmaf(x[i1,c], w1, x[i0,c] * w0)),  x = vertices[b], w = rec_w[k, 0..2]:
 *                           one rounded product and two FUSED multiply-adds, the only fused operations of this stage.  It is
 *                           the order in which the reference's einsum('blfi,blf->bli') sums over f on the device (a dot
 *                           product with a fused accumulator, measured at seven shapes from 12 to 13 056 coordinates without
 *                           one differing bit), so that the rows equal the reference's expressions in torch bit for bit
 *     EXA_MESH_KPT_DYNAMIC  the same with (i0, i1, i2) = dyn_vtx[bin, slot], w = dyn_w[bin, slot], slot = rec's i0, bin = the
 *                           item's yaw bin; dyn_vtx, dyn_w are [EXA_MESH_KPT_BINS, Ld, 3]
 *   An index outside its table reads nothing and gives NaN (the host refuses such a table first).
 *   Yaw bin (only with Ld > 0, else 0; rot takes no gradient).  rel = identity; for i = 0 .. C - 1: rel = rot[b, chain[i]] . rel,
 *   each element (R[r,0] * rel[0,c] + R[r,1] * rel[1,c]) + R[r,2] * rel[2,c].  sy = sqrtf(rel00 * rel00 + rel10 * rel10),
 *   a = atan2f(-rel20, sy), deg = ((-a) * 180.0f) / (float)pi.  A deg that is not finite gives bin 0.  y = rintf(min(deg, 39))
 *   (half to even); bin = y for y >= 0, 39 - y for -39 <= y < 0, 78 for y < -39; clamped into [0, 78] before any table read.
 *   root = raw(record K);  cam = (raw - root) + trans  (trans NULL: no addition);
 *   kpt_proj = ((cam_x / cam_z) * focal_x) + princpt_x, likewise y: IEEE division, cam_z == 0 included;
 *   kpt_cam = cam, or cam - trans with root_rel;  mesh_cam = (vertices - root) + trans, then - trans with root_rel.
 *   Backward.  Cotangents g_cam [B, K, 3], g_proj [B, K, 2], g_root [B, 3], g_mesh [B, V, 3], each possibly NULL (= zeros).
 *   Per keypoint, with cam recomputed as above: tx = g_proj_x * focal_x, ty = g_proj_y * focal_y, qx = cam_x / cam_z,
 *   qy = cam_y / cam_z;  p = (tx / cam_z, ty / cam_z, -((tx * qx + ty * qy) / cam_z)), or +0 without g_proj;
 *   c_k = g_cam + p (just g_cam, or just p, when the other is NULL).  S_c = sum of c_k, S_p = sum of p_k: s = +0.0, s = s + x_k
 *   for k = 0 .. K - 1.  S_m[c] = SUM2 of g_mesh[b, :, c] exactly as the centred term above (workgroups of EXA_MESH_KPT_ROWS
 *   = 256 vertices, exa_mesh_keypoints_blocks(V) partials), +0.0 without g_mesh.
 *     r_K (the root's raw cotangent) = (g_root - S_c) - S_m;   r_k = c_k for k < K
 *     d_trans = S_c + S_m, or S_p with root_rel (the camera coordinates' own + trans - trans cancels exactly)
 *     d_joints[b, j] = +0.0, then + r_k for the records k = 0 .. K that name joint j, ascending (joff / jent)
 *     d_vertices[b, v] = g_mesh[b, v] (+0.0 without), then acc = acc + w * r_k for the entries (k, corner, bin) of v in
 *       ascending (k, corner, bin) (vrow / voff / vent_*): those with bin == -1 (static; a vertex record has w = 1) and those
 *       whose bin is the item's yaw bin.
 *   No gradient to rot, focal or princpt.
 *
 * COORD LOSS.  kpt_proj, kpt_proj_gt [B, K, 2], kpt_valid [B, K] (assumed >= 0), kpt_cam [B, K, 3], weight [B, K, 2] or NULL.
 * Per item and hand (index list idx [n]): sum = +0.0, sum = sum + valid[idx[i]] for i = 0 .. n - 1; z likewise over
 * cam[idx[i], 2], depth = z / (float)n; over the entries with valid > 0, in order, min and max of x and of y (as torch.minimum
 * / torch.maximum: NaN once an operand is).  The item is skipped (hand_w = 1 everywhere) when either sum == 0 or either hand
 * has no entry > 0.  Else per axis: centre = (min + max) / 2, width = max - min, lo = centre - (0.5f * width) * 1.2f,
 * hi = centre + (0.5f * width) * 1.2f, w = hi - lo; x2 = w + lo (the reference's xywh -> xyxy); with (x1, y1, x2, y2) per hand:
 *     inter = max(0, min(lx2, rx2) - max(lx1, rx1)) * max(0, min(ly2, ry2) - max(ly1, ry1))
 *     area = (x2 - x1) * (y2 - y1);   iou = inter / (((area_l + area_r) - inter) + 1e-5f)
 * If iou > 0.5f the hand with the larger depth loses (the right one on a tie): hand_w = 0 for the keypoints whose part[k] has
 * that hand's bit (1 left, 2 right; the hand's rows and its wrist), 1 elsewhere.
 *     loss = ((|proj - gt| * valid) * hand_w) * weight                     (the last product only with weight)
 *     dL_dproj = (((g * weight) * hand_w) * valid) * sign(proj - gt),  sign(0) = 0
 * B == 0 is a successful no-op in every call. */
#define EXA_MESH_KPT_ROWS 256           /* threads per workgroup = vertices per partial of the g_mesh sum */
#define EXA_MESH_KPT_BINS 79            /* rows of the dynamic landmark tables */
#define EXA_MESH_KPT_JOINT 0
#define EXA_MESH_KPT_VERTEX 1
#define EXA_MESH_KPT_STATIC 2
#define EXA_MESH_KPT_DYNAMIC 3

/* The tables of one keypoint selection; every pointer is a device pointer. */
typedef struct ExaMeshKeypoints {
    int32_t V, J, K, Ld, C, T;           /* vertices, joints, keypoints, dynamic slots, chain length, touched vertices */
    const int32_t* rec;                  /* [K + 1, 4] */
    const float* rec_w;                  /* [K + 1, 3] */
    const int32_t* dyn_vtx;              /* [79, Ld, 3] */
    const float* dyn_w;                  /* [79, Ld, 3] */
    const int32_t* chain;                /* [C] */
    const int32_t* vrow;                 /* [V]: the vertex's row of voff, -1 when no record touches it */
    const int32_t* voff;                 /* [T + 1] */
    const int32_t* vent_k;               /* per entry: the record, */
    const int32_t* vent_bin;             /* its bin (-1: static) */
    const float* vent_w;                 /* and its weight */
    const int32_t* joff;                 /* [J + 1] */
    const int32_t* jent;                 /* the records naming each joint, ascending */
} ExaMeshKeypoints;

/* The partials per (b, c) of the g_mesh sum: ceil(V / 256); 0 for V <= 0. */
int64_t exa_mesh_keypoints_blocks(int32_t V);

/* Host only: the bytes of the backward's workspace (the rows [B, 2 K + 1, 3] and the partials [B, 3, blocks]). */
int exa_mesh_keypoints_workspace_size(int32_t B, int32_t V, int32_t K, uint64_t* out_bytes);

/* One launch, two with mesh_cam.  kpt_cam [B, K, 3], root_cam [B, 3], yaw_bin [B] int32: fully written; kpt_proj [B, K, 2]
 * (NULL: not wanted; else focal and princpt are required) and mesh_cam [B, V, 3] (NULL: not wanted) likewise.  rot is
 * required with Ld > 0 and unread otherwise. */
int exa_mesh_keypoints_forward(const ExaMeshKeypoints* tables, int32_t B, const float* vertices, const float* joints,
                               const float* rot, const float* trans, const float* focal, const float* princpt,
                               int32_t root_rel, float* kpt_cam, float* root_cam, float* kpt_proj, float* mesh_cam,
                               int32_t* yaw_bin, void* stream);

/* Two launches, three with g_mesh_cam.  yaw_bin: the forward's.  workspace [dev]: exa_mesh_keypoints_workspace_size bytes,
 * every section written before it is read.  d_vertices [B, V, 3] and d_joints [B, J, 3] fully written; d_trans [B, 3]
 * written when trans is given (NULL: not wanted). */
int exa_mesh_keypoints_backward(const ExaMeshKeypoints* tables, int32_t B, const float* vertices, const float* joints,
                                const float* trans, const float* focal, const float* princpt, int32_t root_rel,
                                const int32_t* yaw_bin, const float* g_kpt_cam, const float* g_kpt_proj,
                                const float* g_root_cam, const float* g_mesh_cam, void* workspace, uint64_t workspace_bytes,
                                float* d_vertices, float* d_joints, float* d_trans, void* stream);

/* One launch, one wave per item.  lhand_idx [n_lhand], rhand_idx [n_rhand], part [K] int32 [dev]; hand_w [B, K] and loss
 * [B, K, 2] fully written. */
int exa_mesh_coord_loss_forward(int32_t B, int32_t K, int32_t n_lhand, int32_t n_rhand, const int32_t* lhand_idx,
                                const int32_t* rhand_idx, const int32_t* part, const float* kpt_proj,
                                const float* kpt_proj_gt, const float* kpt_valid, const float* kpt_cam, const float* weight,
                                float* hand_w, float* loss, void* stream);

/* One launch, one thread per element.  hand_w: the forward's; dL_dkpt_proj [B, K, 2] fully written. */
int exa_mesh_coord_loss_backward(int32_t B, int32_t K, const float* kpt_proj, const float* kpt_proj_gt,
                                 const float* kpt_valid, const float* weight, const float* hand_w, const float* grad_loss,
                                 float* dL_dkpt_proj, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EXA_MESH_H */
