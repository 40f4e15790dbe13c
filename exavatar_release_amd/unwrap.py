"""HIP face-texture unwrap: drop-ins for the UV side of the reference's ``fitting/`` code.

* ``get_face_index_map_uv(vertex_uv, face_uv, uvmap_shape)`` -- reference ``fitting/common/nets/layer.py:9-23`` and its
  copy ``avatar/common/utils/flame.py:13-27`` (pytorch3d ``MeshRasterizer`` under ``OrthographicCameras``): a
  ``Fragments`` namedtuple over the UV atlas.
* ``XY2UV(vertex_uv, face_uv, uvmap_shape)`` -- reference ``layer.py:41-102``: ``forward(img, mesh_cam, face, cam_param)``
  -> ``(uvmap [B,C,Hu,Wu] float32, mask [B,C,Hu,Wu] bool)``.
* ``TextureUnwrap(xy2uv, uv_weight)`` -- the accumulation of ``fitting/main/unwrap.py:76-91``: ``add(...)`` per batch of
  frames, ``result()`` at the end; nothing of the size [B,C,Hu,Wu] is written and nothing is copied to the host.
* ``uv_region_mask(pix_to_face_uv, face, vertex_keep)`` -- the two face loops of ``fitting/common/utils/flame.py:53-72``
  as one gather (plain torch: it needs no kernel).

The kernels are ``csrc/unwrap.hip`` and the orthographic mode of ``csrc/mesh_raster.hip`` behind ``include/exa_mesh.h``;
ROCm device tensors only, no CPU path.  Forward only: nothing in the reference differentiates through the unwrap, and a
tensor that requires grad is refused by name.  The CPU restatement that pins them is ``tests/unwrap_oracle.py``.  No
stream capture of these calls has been run.

The UV raster's convention (pytorch3d 0.7's behaviour for the reference's settings, restated)
---------------------------------------------------------------------------------------------
The reference scales u by ``uvmap_shape[1]`` = Wu and v by ``uvmap_shape[0]`` = Hu, appends the dummy depth 1, negates x
and y and uses ``OrthographicCameras(in_ndc=False, image_size=(Hu, Wu))`` with the defaults focal 1 and principal point
0.  pytorch3d converts a screen-space camera to NDC with s = min(Hu, Wu) / 2 exactly as for the pinhole of
``mesh.py``: ``fx_ndc = 1 / s``, ``px_ndc = -(0 - Wu / 2) / s = Wu / (2 s)``; an orthographic camera projects a view-space
point (X', Y', Z) to ``x_ndc = fx_ndc X' + px_ndc`` (no division by Z).  With X' = -u Wu: ``x_ndc = (Wu / 2 - u Wu) / s``.
The rasterizer puts the centre of texel (row i, col j) at ``x_ndc = (Wu - 2 j - 1) / min(Hu, Wu) = (Wu / 2 - j - 1/2) / s``;
equating the two gives ``u Wu = j + 1/2``, and the same in y with Hu: the centre of texel (i, j) lies at
``(u Wu, v Hu) = (j + 0.5, i + 0.5)``, also for a non-square map (s cancels).  So the UV raster is the image raster of
``mesh.py`` on the screen points ``(u Wu, v Hu)`` at depth 1, without a projection: ``exa_mesh_forward_ortho``.

Coverage, the degenerate-face rule (|A| < 1e-8 square texels) and the tie rule are the image raster's.  pytorch3d applies
the perspective correction only under a perspective camera, so ``bary_coords`` are the plain screen barycentrics
``b_k = E_k / A`` and ``zbuf = (b_0 + b_1) + b_2`` (each times the depth 1): 1 up to rounding.  All depths being equal,
where UV faces overlap the lower face index wins wherever the two sums round alike (they do when the barycentrics are
dyadic; a real atlas has no overlap).  Background is -1 in all three outputs.

``XY2UV.forward`` (reference ``layer.py:53-102``, restated)
-----------------------------------------------------------
Visible faces.  ``pix_to_face_xy`` is the image raster of ``mesh_cam`` at the image's size (``exa_mesh_forward``, no zbuf,
no barycentrics).  Face f of item n is visible when some pixel of ``pix_to_face_xy[n]`` holds it.  The reference's
wrap-around is reproduced: ``torch.unique`` keeps the -1 of background pixels and ``valid_face_mask[-1] = 1`` then marks
the LAST face, so when item n has at least one background pixel, face F - 1 is visible whether it was hit or not.

Texels.  A texel whose ``pix_to_face_uv`` is -1, or whose face is not visible, gets ``uvmap = 0`` and ``mask = False`` in
every channel (+0.0 where the reference's ``-1 * False`` gives -0.0: the one place where the bits differ).  Any other
texel, with b its ``bary_coords_uv`` and k the three vertices of its face, in float32, in this order, never contracted:
``x_k = X_k / Z_k * fx + cx``, ``y_k = Y_k / Z_k * fy + cy``; ``px = (x_0 b_0 + x_1 b_1) + x_2 b_2`` and ``py`` likewise;
``gx = px / (W - 1) * 2 - 1``, ``gy = py / (H - 1) * 2 - 1``; then ``F.grid_sample(img, ., 'bilinear', 'zeros',
align_corners=True)``: ``ix = ((gx + 1) / 2) * (W - 1)``, the four taps with the weights and the order ``mesh.py`` states
for the texture sampler (``0 + v_nw nw + v_ne ne + v_sw sw + v_se se``, weights from ``ix_se - ix`` etc.), a tap outside
the image contributing nothing.  ``mask = (value != -1)`` per channel and ``uvmap = value`` where it holds, else 0.  (The
division by ``W - 1`` is a division, as PyTorch's CPU kernel evaluates it.)  A position that is not finite -- an image of
one row or column -- has no tap: value 0, mask True.

The one deliberate difference: a last face that only the wrap-around marks may have been culled by the raster; where one
of its corners has Z <= 1e-6 the reference samples the image through a mirrored (Z < 0) or non-finite (Z = 0) projection,
and this module writes ``uvmap = 0``, ``mask = False`` there instead.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._device import _ptr, _workspace, check_no_grad, launch, need_rocm
from .mesh import Fragments, _camera, _forward, _topology

MAX_CHANNELS = 8          # EXA_MESH_MAX_CHANNELS


def _shape2(uvmap_shape, what):
    try:
        Hu, Wu = int(uvmap_shape[0]), int(uvmap_shape[1])
    except (TypeError, ValueError, IndexError):
        raise ValueError('%s: uvmap_shape must be (rows, columns)' % what)
    if len(uvmap_shape) != 2 or Hu < 1 or Wu < 1:
        raise ValueError('%s: uvmap_shape must be (rows, columns), each at least 1' % what)
    return Hu, Wu


def get_face_index_map_uv(vertex_uv, face_uv, uvmap_shape):
    """Drop-in for reference ``layer.py:9-23`` / ``flame.py:13-27``: rasterize the UV atlas ``vertex_uv`` [N,U,2] (u, v in
    [0, 1], on a ROCm device) with faces ``face_uv`` [N,F,3] or [F,3] (tensor or numpy; one topology for all N, so the N
    rows of a [N,F,3] tensor must agree and the first is used) at ``uvmap_shape`` = (Hu, Wu).  Returns
    ``Fragments(pix_to_face [N,Hu,Wu,1] int64 (packed n * F + f, -1), zbuf [N,Hu,Wu,1], bary_coords [N,Hu,Wu,1,3],
    dists=None)``; the convention is derived in the module docstring.  Forward only."""
    what = 'get_face_index_map_uv'
    if not isinstance(vertex_uv, torch.Tensor) or vertex_uv.dim() != 3 or vertex_uv.shape[2] != 2:
        raise ValueError('%s: vertex_uv must be a [N, U, 2] tensor' % what)
    need_rocm(vertex_uv.device, what)
    if torch.is_grad_enabled() and vertex_uv.requires_grad:
        raise NotImplementedError('%s: vertex_uv requires grad, and the unwrap is forward only; detach it' % what)
    Hu, Wu = _shape2(uvmap_shape, what)
    device = vertex_uv.device
    if isinstance(face_uv, torch.Tensor) and face_uv.dim() == 3:
        face_uv = face_uv[0]
    elif not isinstance(face_uv, torch.Tensor) and np.asarray(face_uv).ndim == 3:
        face_uv = np.asarray(face_uv)[0]
    N, U = vertex_uv.shape[0], vertex_uv.shape[1]
    faces = _topology(face_uv, U, device)[0]
    uv = vertex_uv.detach().to(torch.float32)
    # the reference's own float32 scaling (layer.py:11-12); its negation of x and y is pytorch3d's axis convention
    verts = torch.stack((uv[:, :, 0] * Wu, uv[:, :, 1] * Hu, torch.ones_like(uv[:, :, 0])), 2).contiguous()
    F = faces.shape[0]
    ws = _lib.mesh_workspace_sizes(N, F, Hu, Wu)
    face_ws, bin_ws = _workspace(ws.face_bytes, device), _workspace(ws.bin_bytes, device)
    pix_to_face = torch.empty((N, Hu, Wu), dtype=torch.int64, device=device)
    zbuf = torch.empty((N, Hu, Wu), dtype=torch.float32, device=device)
    bary = torch.empty((N, Hu, Wu, 3), dtype=torch.float32, device=device)
    g = _lib.ExaMeshGeometry(N, U, F, Hu, Wu, verts.data_ptr(), faces.data_ptr(), None, None)
    launch(_lib.MESH, 'exa_mesh_forward_ortho', device, ctypes.byref(g), _ptr(face_ws), _ptr(bin_ws), _ptr(pix_to_face),
           _ptr(zbuf), _ptr(bary))
    return Fragments(pix_to_face[..., None], zbuf[..., None], bary[:, :, :, None, :], None)


def _unwrap(pix_to_face_uv, bary_uv, img, mesh_cam, faces, focal, princpt, pix_to_face_xy, uvmap, mask, tex_sum, mask_sum,
            uv_weight, face_valid):
    """One ``exa_mesh_unwrap`` call over checked, contiguous device tensors."""
    device = img.device
    B, C, H, W = img.shape
    Hu, Wu = pix_to_face_uv.shape
    F = faces.shape[0]
    flag_ws = _workspace(_lib.unwrap_workspace_size(B, F), device)
    u = _lib.ExaMeshUnwrap(B, mesh_cam.shape[1], F, C, H, W, Hu, Wu, img.data_ptr(), mesh_cam.data_ptr(), faces.data_ptr(),
                           focal.data_ptr(), princpt.data_ptr(), pix_to_face_xy.data_ptr(), pix_to_face_uv.data_ptr(),
                           bary_uv.data_ptr(), uv_weight.data_ptr() if uv_weight is not None else None,
                           face_valid.data_ptr() if face_valid is not None else None)
    launch(_lib.MESH, 'exa_mesh_unwrap', device, ctypes.byref(u), _ptr(flag_ws), flag_ws.numel(), _ptr(uvmap), _ptr(mask),
           _ptr(tex_sum), _ptr(mask_sum))


class XY2UV(nn.Module):
    """Drop-in for reference ``layer.py:41-102``: the same constructor arguments (``vertex_uv`` [U,2] and ``face_uv``
    [F,3] numpy arrays, ``uvmap_shape`` = (Hu, Wu)), the same ``forward`` signature and result (module docstring).  The
    constructor runs ``get_face_index_map_uv`` once on the current ROCm device and keeps ``pix_to_face_uv`` [Hu,Wu] int64
    and ``bary_coords_uv`` [Hu,Wu,3] under the reference's attribute names, as non-persistent buffers."""

    def __init__(self, vertex_uv, face_uv, uvmap_shape):
        super(XY2UV, self).__init__()
        vertex_uv = torch.as_tensor(np.asarray(vertex_uv)).float().cuda()[None, :, :]
        face_uv = np.ascontiguousarray(np.asarray(face_uv).reshape(-1, 3))
        self.uvmap_shape = _shape2(uvmap_shape, 'XY2UV')
        outputs = get_face_index_map_uv(vertex_uv, face_uv, self.uvmap_shape)
        self.face_num = int(face_uv.shape[0])
        self.register_buffer('pix_to_face_uv', outputs.pix_to_face[0, :, :, 0].contiguous(), persistent=False)
        self.register_buffer('bary_coords_uv', outputs.bary_coords[0, :, :, 0, :].contiguous(), persistent=False)

    def _inputs(self, what, img, mesh_cam, face, cam_param):
        """The checked, contiguous device tensors of one call and the image raster's ``pix_to_face_xy`` [B,H,W]."""
        for name, x in (('img', img), ('mesh_cam', mesh_cam)):
            if not isinstance(x, torch.Tensor):
                raise TypeError('%s: %s must be a tensor' % (what, name))
            if x.device.type != 'cuda':
                raise RuntimeError('%s: %s must be on a ROCm device (it is on %s; there is no CPU path)' % (what, name, x.device))
        if torch.is_grad_enabled():
            for name, x in (('img', img), ('mesh_cam', mesh_cam), ('focal', cam_param['focal']),
                            ('princpt', cam_param['princpt'])):
                if isinstance(x, torch.Tensor) and x.requires_grad:
                    raise NotImplementedError('%s: %s requires grad, and the unwrap is forward only (nothing in the '
                                              'reference differentiates through it); detach it' % (what, name))
        if img.dim() != 4 or not 1 <= img.shape[1] <= MAX_CHANNELS:
            raise ValueError('%s: img must be [B, C, H, W] with 1 <= C <= %d (it has %s)' % (what, MAX_CHANNELS,
                                                                                               tuple(img.shape)))
        B, C, H, W = img.shape
        if mesh_cam.dim() != 3 or mesh_cam.shape[0] != B or mesh_cam.shape[2] != 3:
            raise ValueError('%s: mesh_cam must be [%d, V, 3] (it has %s)' % (what, B, tuple(mesh_cam.shape)))
        device = img.device
        if mesh_cam.device != device or self.pix_to_face_uv.device != device:
            raise ValueError('%s: img, mesh_cam and the module must be on one device' % what)
        topo = _topology(face, mesh_cam.shape[1], device)
        if topo[0].shape[0] != self.face_num:
            raise ValueError('%s: face has %d faces, face_uv has %d' % (what, topo[0].shape[0], self.face_num))
        focal, princpt = _camera(cam_param, B, device)
        img = img.detach().to(torch.float32).contiguous()
        verts = mesh_cam.detach().to(torch.float32).contiguous()
        # the image raster: the existing call, no zbuf and no barycentrics
        pix_to_face_xy = _forward(verts, topo, focal, princpt, H, W, None, None, False)[1]
        return img, verts, topo[0], focal, princpt, pix_to_face_xy

    def forward(self, img, mesh_cam, face, cam_param):
        """``img`` [B,C,H,W] (C = 1 .. 8), ``mesh_cam`` [B,V,3] camera space, ``face`` [F,3] (numpy or tensor, one topology
        for the batch), ``cam_param['focal']`` / ``['princpt']`` [B,2] or [2].  Returns ``(uvmap, mask)``: float32 and
        ``torch.bool`` [B,C,Hu,Wu], as the module docstring states them."""
        img, verts, faces, focal, princpt, p2f = self._inputs('XY2UV', img, mesh_cam, face, cam_param)
        B, C = img.shape[0], img.shape[1]
        Hu, Wu = self.uvmap_shape
        uvmap = torch.empty((B, C, Hu, Wu), dtype=torch.float32, device=img.device)
        mask = torch.empty((B, C, Hu, Wu), dtype=torch.bool, device=img.device)
        _unwrap(self.pix_to_face_uv, self.bary_coords_uv, img, verts, faces, focal, princpt, p2f, uvmap, mask, None, None,
                None, None)
        return uvmap, mask


class TextureUnwrap:
    """The accumulation of reference ``fitting/main/unwrap.py:76-91`` over an ``XY2UV``: ``add`` runs the unwrap's
    launches on one batch of frames and the texel kernel adds ``sum_b value * uv_weight * valid_b`` and ``sum_b mask *
    uv_weight * valid_b`` into two persistent [C,Hu,Wu] float32 buffers, in place and in index order (no atomics: the same
    calls give the same bits); ``result()`` is ``(texture_sum / (mask_sum + 1e-4), mask_sum > 0)``.  ``uv_weight`` [Hu,Wu]
    is the reference's ``flame.uv_mask`` (``uv_region_mask(...).float()``)."""

    def __init__(self, xy2uv, uv_weight):
        if not isinstance(xy2uv, XY2UV):
            raise TypeError('TextureUnwrap: xy2uv must be an XY2UV')
        if not isinstance(uv_weight, torch.Tensor) or tuple(uv_weight.shape) != tuple(xy2uv.uvmap_shape):
            raise ValueError('TextureUnwrap: uv_weight must be a [%d, %d] tensor' % tuple(xy2uv.uvmap_shape))
        check_no_grad('TextureUnwrap', 'uv_weight', uv_weight, 'a buffer')
        self.xy2uv = xy2uv
        self.uv_weight = uv_weight.detach().to(device=xy2uv.pix_to_face_uv.device, dtype=torch.float32).contiguous()
        self.texture_sum = None
        self.mask_sum = None

    def add(self, img, mesh_cam, face, cam_param, face_valid=None):
        """One batch: ``img``, ``mesh_cam``, ``face``, ``cam_param`` as ``XY2UV.forward``; ``face_valid`` [B] (bool or
        float, device) or None (every frame counts).  Returns nothing; the sums are ``texture_sum`` and ``mask_sum``."""
        what = 'TextureUnwrap.add'
        img, verts, faces, focal, princpt, p2f = self.xy2uv._inputs(what, img, mesh_cam, face, cam_param)
        B, C = img.shape[0], img.shape[1]
        if face_valid is not None:
            if not isinstance(face_valid, torch.Tensor) or face_valid.numel() != B:
                raise ValueError('%s: face_valid must be a tensor of %d values' % (what, B))
            check_no_grad(what, 'face_valid', face_valid)
            face_valid = face_valid.detach().to(device=img.device, dtype=torch.float32).reshape(B).contiguous()
        Hu, Wu = self.xy2uv.uvmap_shape
        if self.texture_sum is None:
            self.texture_sum = torch.zeros((C, Hu, Wu), dtype=torch.float32, device=img.device)
            self.mask_sum = torch.zeros((C, Hu, Wu), dtype=torch.float32, device=img.device)
        elif self.texture_sum.shape[0] != C:
            raise ValueError('%s: img has %d channels, the sums hold %d' % (what, C, self.texture_sum.shape[0]))
        _unwrap(self.xy2uv.pix_to_face_uv, self.xy2uv.bary_coords_uv, img, verts, faces, focal, princpt, p2f, None, None,
                self.texture_sum, self.mask_sum, self.uv_weight, face_valid)

    def result(self):
        """``(face_texture [C,Hu,Wu] float32, face_texture_mask [C,Hu,Wu] bool)`` of reference ``unwrap.py:88-89``."""
        if self.texture_sum is None:
            raise RuntimeError('TextureUnwrap.result: nothing has been added')
        return self.texture_sum / (self.mask_sum + 1e-4), self.mask_sum > 0


def uv_region_mask(pix_to_face_uv, face, vertex_keep):
    """The texels whose face keeps all three vertices: ``(p2f >= 0) & vertex_keep[face].all(1)[p2f.clamp_min(0)]``.  This
    is what the loops of reference ``flame.py:53-72`` leave of ``uv_mask`` when ``vertex_keep`` is False at the excluded
    vertices (``~is_neck & expr_vertex_mask``).  ``pix_to_face_uv`` [Hu,Wu] int64 (-1: no face), ``face`` [F,3] (tensor or
    numpy), ``vertex_keep`` [V] bool; plain torch on ``pix_to_face_uv``'s device.  Returns a bool [Hu,Wu] tensor."""
    if not isinstance(pix_to_face_uv, torch.Tensor) or pix_to_face_uv.dim() != 2:
        raise ValueError('uv_region_mask: pix_to_face_uv must be a [Hu, Wu] tensor')
    device = pix_to_face_uv.device
    face = torch.as_tensor(np.asarray(face) if not isinstance(face, torch.Tensor) else face).to(device).long().reshape(-1, 3)
    vertex_keep = torch.as_tensor(vertex_keep).to(device)
    if vertex_keep.dtype != torch.bool or vertex_keep.dim() != 1:
        raise ValueError('uv_region_mask: vertex_keep must be a bool [V] tensor')
    p2f = pix_to_face_uv.long()
    if face.shape[0] == 0:
        return torch.zeros_like(p2f, dtype=torch.bool)
    if int(p2f.max()) >= face.shape[0]:
        raise ValueError('uv_region_mask: pix_to_face_uv names a face outside [0, %d)' % face.shape[0])
    return (p2f >= 0) & vertex_keep[face].all(1)[p2f.clamp_min(0)]
