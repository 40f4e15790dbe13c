"""HIP triangle rasterizer + UV texture sample: drop-ins for the face render of the reference.

* ``MeshRenderer(vertex_uv, face_uv)`` -- reference ``avatar/common/nets/layer.py:40-68`` (pytorch3d ``MeshRasterizer`` +
  ``TexturesUV``).  ``forward(uvmap, mesh, face, cam_param, render_shape)`` -> ``[N, C, H, W]``, -1 in every channel of a
  background pixel; differentiable in ``mesh`` (and through the PyTorch world->camera ``bmm`` in ``R`` / ``t``).
* ``render_mesh(mesh, face, cam_param, bkg, blend_ratio=1.0)`` -- reference ``avatar/common/utils/vis.py:73-109`` and
  ``fitting/common/utils/vis.py:18-53`` (pytorch3d ``SoftPhongShader``): the Phong-shaded mesh over ``bkg``, a numpy
  [H,W,3] array.  Forward only, like ``shade_mesh`` (the device part) and ``vertex_normals`` under it.
* ``get_face_index_map_xy(mesh, face, cam_param, render_shape)`` -- reference ``layer.py:23-38``: a ``Fragments``
  namedtuple.  ``pix_to_face`` [N,H,W,1] int64 holds packed ``n * F + f`` (-1: no face); ``zbuf`` [N,H,W,1] and
  ``bary_coords`` [N,H,W,1,3] are differentiable in ``mesh`` (-1 at background pixels); ``dists`` is ``None`` (the
  reference never reads it, and its pytorch3d value needs the blur machinery this rasterizer does not have).

The kernels are ``csrc/mesh_raster.hip`` behind ``include/exa_mesh.h``; ROCm device tensors only, no CPU path.  The CPU
restatement that pins them is ``tests/mesh_oracle.py``.

Conventions (pytorch3d 0.7's behaviour for the reference's settings, restated)
------------------------------------------------------------------------------
Projection.  The reference negates x and y of the camera-space mesh (layer.py:26) and uses ``PerspectiveCameras(
in_ndc=False, image_size=(H, W))``.  pytorch3d converts a screen-space camera to NDC with s = min(H, W) / 2:
``fx_ndc = fx / s``, ``px_ndc = -(px - W / 2) / s`` (same for y with H), and projects a view-space point (X', Y', Z)
to ``x_ndc = fx_ndc X' / Z + px_ndc``.  Its NDC has +x left and +y up, and its rasterizer puts the centre of pixel
(row i, col j) at ``x_ndc = (W - 2 j - 1) / min(H, W)``, ``y_ndc = (H - 2 i - 1) / min(H, W)``.  With X' = -X:
``x_ndc = -(fx X / Z + px - W / 2) / s``; setting it equal to the centre of column j gives
``fx X / Z + px - W / 2 = j + 1/2 - W / 2``, i.e. the OpenCV pinhole ``u = fx X / Z + cx`` with column j's centre at
u = j + 0.5 (and ``v = fy Y / Z + cy``, row i's centre at v = i + 0.5).  Barycentrics are invariant under the affine
map between NDC and pixels, so everything below is computed in pixels.

Coverage.  ``blur_radius = 0``, ``faces_per_pixel = 1``, ``cull_backfaces = False``.  With screen corners s_k and
pixel centre p, ``E_k = cross(s_{k+1} - p, s_{k+2} - p)``, ``A = cross(s_1 - s_0, s_2 - s_0)``, ``b_k = E_k / A``; the
pixel is inside when all three b_k > 0 (either winding).  A face whose |A| < 1e-8 square pixels is degenerate and
skipped.  A face with any corner at Z <= 1e-6 is culled outright: pytorch3d, without ``z_clip_value``, rasterizes a
face that crosses the camera plane through the projective wrap-around, which is not worth imitating, and ExAvatar's
face mesh never comes near that plane.

Depth test.  The nearest face by interpolated view-space z (below) wins; on equal z the lower face index wins, so the
result does not depend on the order in which faces are walked.

Perspective-correct barycentrics (pytorch3d's default for perspective cameras): ``b'_k = (b_k / z_k) / sum_i(b_i /
z_i)``, ``zbuf = sum_k b'_k z_k``.  No clipping of b' (pytorch3d clips only when blur_radius > 0).

TexturesUV.  ``face_uv`` indexes ``vertex_uv`` (a different index set from ``face``); the pixel's uv is
``sum_k b'_k uv_k``; the map is sampled as ``F.grid_sample(flip(map, rows), 2 uv - 1, 'bilinear', padding_mode='border',
align_corners=True)`` -- the kernel reads row ``H_t - 1 - y`` instead of flipping.  The reference flips ``vertex_uv``'s
v once at load (flame.py) and once more in ``MeshRenderer.forward`` (layer.py:53); the constructor here keeps the
reference's signature and ``forward`` repeats the second flip, so both compose as they do there.  The blend is
evaluated as F.grid_sample does (``0 + v_nw nw + v_ne ne + v_sw sw + v_se se``, weights from ``ix_se - ix`` etc.)
without fused multiply-adds, so ``render[:, 3:] == 1`` (the reference's face mask, model.py:200) agrees with what
PyTorch computes from the same uv.  1 .. 8 channels; the texture is a fixed buffer (no texture gradient).

Phong-shaded render (reference ``render_mesh``, ``avatar/common/utils/vis.py:73-109`` and its numpy twin in
``fitting/common/utils/vis.py:18-53``: pytorch3d ``SoftPhongShader`` + ``PointLights()`` + ``Materials(specular_color=0,
shininess=0)`` + ``TexturesVertex`` of ones).  Rasterization is the one above, unchanged.  Negating x and y is a
rotation, so every dot product of the shader is evaluated in the caller's camera frame: pytorch3d's default light at
(0, 1, 0) is (0, -1, 0) here, and the camera centre is the origin.
  * Vertex normals (pytorch3d ``_compute_vertex_normals``): corner k of every face -- culled and hidden faces included --
    adds ``cross(v_{k+1} - v_k, v_{k+2} - v_k)``; each sum is normalised as ``x / max(|x|, 1e-6)`` (a vertex whose faces
    are all degenerate keeps a zero normal).
  * At a covered pixel, with the nearest face's corners k and its perspective-correct barycentrics b':
    ``p = sum b'_k v_k``, ``n = sum b'_k n_k``, ``l^ = normalize(L - p)``, ``n^ = normalize(n)``, ``cos = n^ . l^``,
    ``v^ = normalize(-p)``, ``r = -l^ + 2 cos n^``;
    ``colour = La Ma + Ld Md relu(cos) + Ls Ms (relu(v^ . r) [cos > 0]) ** shininess`` per channel (``0 ** 0 = 1``,
    as ``torch.pow``).  There is no flip of the normal towards the viewer: the winding decides which side is lit.  The
    reference's constants give ``0.5 + 0.3 relu(cos)``, grey.
  * Blend: for one face per pixel pytorch3d's ``softmax_rgb_blend`` (sigma = gamma = 1e-4, znear 1, zfar 100) returns
    the shaded colour to ~1e-10 wherever 0 < z < 100, and the background colour (1, 1, 1) at empty pixels; that is what
    the kernel writes.  At z >= zfar pytorch3d mixes in the background with a weight that depends on its ``dists``, which
    this rasterizer does not compute: not reproduced (an avatar is a few metres from the camera).  The alpha channel is
    not produced (the reference keeps ``images[..., :3]``).
  * ``render_mesh`` then applies the reference's composite in numpy as written: ``is_bkg = zbuf <= 0`` (the same pixels
    as ``pix_to_face == -1``), ``fg = render * blend_ratio + bkg / 255 * (1 - blend_ratio)``, ``fg * (1 - is_bkg) * 255
    + bkg * is_bkg``.
"""
import collections
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._device import _ptr, grad_in, launch, need_rocm
from ._tables import Cache, face_tables

Fragments = collections.namedtuple('Fragments', ['pix_to_face', 'zbuf', 'bary_coords', 'dists'])
Fragments.__doc__ = """pytorch3d ``Fragments`` of one face per pixel: ``pix_to_face`` [N,H,W,1] int64 (packed n * F + f, -1 for
background), ``zbuf`` [N,H,W,1], ``bary_coords`` [N,H,W,1,3] (-1 for background), ``dists`` None (not computed)."""

_topologies = Cache()     # (id(face), V, device) -> (host copy of face, (faces [F,3] int32, CSR offsets, CSR entries))


def _topology(face, V, device):
    """``face`` as a device int32 [F,3] tensor plus the vertex -> (face, corner) CSR of the backward, built once per
    topology: the cache is keyed on the object and checked against a host copy of its contents (numpy has no ``_version``)."""
    host = face.detach().cpu().numpy() if isinstance(face, torch.Tensor) else np.asarray(face)
    host = np.ascontiguousarray(host.reshape(-1, 3), dtype=np.int32)
    key = (id(face), int(V), str(device))
    hit = _topologies.find(key)
    if hit is not None and hit[0].shape == host.shape and np.array_equal(hit[0], host):
        return hit[1]
    return _topologies.keep(key, (host, face_tables(host, V, device)), face)[1]


def _camera(cam_param, N, device):
    focal = torch.as_tensor(cam_param['focal']).to(device=device, dtype=torch.float32).reshape(-1, 2).expand(N, 2)
    princpt = torch.as_tensor(cam_param['princpt']).to(device=device, dtype=torch.float32).reshape(-1, 2).expand(N, 2)
    return focal.contiguous(), princpt.contiguous()


def _geometry(verts, faces, focal, princpt, H, W):
    N, V = verts.shape[0], verts.shape[1]
    return _lib.ExaMeshGeometry(N, V, faces.shape[0], H, W, verts.data_ptr(), faces.data_ptr(), focal.data_ptr(),
                                princpt.data_ptr())


def _texture(texture, face_uvs):
    if texture is None:
        return None
    return _lib.ExaMeshTexture(texture.shape[1], texture.shape[2], texture.shape[3], texture.shape[0],
                               texture.data_ptr(), face_uvs.data_ptr())


def _forward(verts, topo, focal, princpt, H, W, texture, face_uvs, want_zbary):
    device = verts.device
    N = verts.shape[0]
    faces = topo[0]
    F = faces.shape[0]
    ws = _lib.mesh_workspace_sizes(N, F, H, W)
    face_ws = torch.empty(int(ws.face_bytes), dtype=torch.uint8, device=device)
    bin_ws = torch.empty(int(ws.bin_bytes), dtype=torch.uint8, device=device)
    pix_to_face = torch.empty((N, H, W), dtype=torch.int64, device=device)
    zbuf = torch.empty((N, H, W), dtype=torch.float32, device=device) if want_zbary else None
    bary = torch.empty((N, H, W, 3), dtype=torch.float32, device=device) if want_zbary else None
    render = torch.empty((N, texture.shape[1], H, W), dtype=torch.float32, device=device) if texture is not None else None
    g = _geometry(verts, faces, focal, princpt, H, W)
    t = _texture(texture, face_uvs)
    launch(_lib.MESH, 'exa_mesh_forward', device, ctypes.byref(g), ctypes.byref(t) if t is not None else None,
           _ptr(face_ws), _ptr(bin_ws), _ptr(pix_to_face), _ptr(zbuf), _ptr(bary), _ptr(render))
    return face_ws, pix_to_face, zbuf, bary, render


def _backward(ctx, dzbuf, dbary, drender):
    verts, focal, princpt, face_ws, pix_to_face = ctx.saved_tensors[:5]
    texture, face_uvs = (ctx.saved_tensors[5], ctx.saved_tensors[6]) if ctx.textured else (None, None)
    faces, offsets, entries = ctx.topo
    device = verts.device
    N = verts.shape[0]
    ws = _lib.mesh_workspace_sizes(N, faces.shape[0], ctx.H, ctx.W)
    grad_ws = torch.empty(int(ws.grad_bytes), dtype=torch.uint8, device=device)
    dverts = torch.empty_like(verts)
    g = _geometry(verts, faces, focal, princpt, ctx.H, ctx.W)
    t = _texture(texture, face_uvs)
    dzbuf, dbary, drender = grad_in(dzbuf), grad_in(dbary), grad_in(drender)
    launch(_lib.MESH, 'exa_mesh_backward', device, ctypes.byref(g), ctypes.byref(t) if t is not None else None,
           _ptr(face_ws), _ptr(pix_to_face), _ptr(dzbuf), _ptr(dbary), _ptr(drender), _ptr(offsets), _ptr(entries),
           _ptr(grad_ws), _ptr(dverts))
    return dverts


class _RasterizeMesh(torch.autograd.Function):
    """verts [N,V,3] camera space -> (pix_to_face [N,H,W], zbuf [N,H,W], bary [N,H,W,3])."""

    @staticmethod
    def forward(ctx, verts, topo, focal, princpt, H, W):
        v = verts.detach().to(torch.float32).contiguous()
        face_ws, pix_to_face, zbuf, bary, _ = _forward(v, topo, focal, princpt, H, W, None, None, True)
        ctx.topo, ctx.H, ctx.W, ctx.textured = topo, H, W, False
        ctx.save_for_backward(v, focal, princpt, face_ws, pix_to_face)
        ctx.mark_non_differentiable(pix_to_face)
        return pix_to_face, zbuf, bary

    @staticmethod
    def backward(ctx, _dp2f, dzbuf, dbary):
        if dzbuf is None and dbary is None:
            return None, None, None, None, None, None
        return _backward(ctx, dzbuf, dbary, None), None, None, None, None, None


class _RenderMesh(torch.autograd.Function):
    """verts [N,V,3] camera space -> (render [N,C,H,W] with -1 at background, pix_to_face [N,H,W])."""

    @staticmethod
    def forward(ctx, verts, topo, focal, princpt, H, W, texture, face_uvs):
        v = verts.detach().to(torch.float32).contiguous()
        face_ws, pix_to_face, _, _, render = _forward(v, topo, focal, princpt, H, W, texture, face_uvs, False)
        ctx.topo, ctx.H, ctx.W, ctx.textured = topo, H, W, True
        ctx.save_for_backward(v, focal, princpt, face_ws, pix_to_face, texture, face_uvs)
        ctx.mark_non_differentiable(pix_to_face)
        return render, pix_to_face

    @staticmethod
    def backward(ctx, drender, _dp2f):
        if drender is None:
            return (None,) * 8
        return (_backward(ctx, None, None, drender),) + (None,) * 7


def _check_mesh(mesh, what):
    if not isinstance(mesh, torch.Tensor) or mesh.dim() != 3 or mesh.shape[2] != 3:
        raise ValueError('%s: mesh must be a [N, V, 3] tensor' % what)
    need_rocm(mesh.device, what)


def get_face_index_map_xy(mesh, face, cam_param, render_shape):
    """Drop-in for reference ``layer.py:23-38``: rasterize the camera-space ``mesh`` [N,V,3] (faces ``face`` [F,3], numpy
    or tensor, one topology for all N) with the pinhole cameras ``cam_param['focal']`` / ``['princpt']`` ([N,2] or [2])
    at ``render_shape`` = (H, W).  Returns ``Fragments(pix_to_face, zbuf, bary_coords, dists=None)``; ``zbuf`` and
    ``bary_coords`` are differentiable in ``mesh``.  For pytorch3d's ``fitting/`` callers this replaces
    ``MeshRasterizer(cameras, RasterizationSettings(blur_radius=0, faces_per_pixel=1))(Meshes(...))``."""
    _check_mesh(mesh, 'get_face_index_map_xy')
    H, W = int(render_shape[0]), int(render_shape[1])
    N, V = mesh.shape[0], mesh.shape[1]
    topo = _topology(face, V, mesh.device)
    focal, princpt = _camera(cam_param, N, mesh.device)
    pix_to_face, zbuf, bary = _RasterizeMesh.apply(mesh, topo, focal, princpt, H, W)
    return Fragments(pix_to_face[..., None], zbuf[..., None], bary[:, :, :, None, :], None)


class MeshRenderer(nn.Module):
    """Drop-in for reference ``layer.py:40-68`` (same constructor, same ``forward`` signature and result)."""

    def __init__(self, vertex_uv, face_uv):
        super(MeshRenderer, self).__init__()
        self.vertex_uv = torch.as_tensor(np.asarray(vertex_uv), dtype=torch.float32).cuda()
        self.face_uv = torch.as_tensor(np.asarray(face_uv), dtype=torch.int64).cuda()

    def forward(self, uvmap, mesh, face, cam_param, render_shape):
        if uvmap.requires_grad:
            raise NotImplementedError('MeshRenderer: texture gradients are not implemented (the reference texture is a '
                                      'fixed buffer); pass uvmap.detach()')
        if uvmap.dim() != 4 or uvmap.shape[1] > 8:
            raise ValueError('MeshRenderer: uvmap must be [N, C, H, W] with C <= 8')
        render_height, render_width = int(render_shape[0]), int(render_shape[1])
        mesh = torch.bmm(cam_param['R'], mesh.permute(0, 2, 1)).permute(0, 2, 1) + cam_param['t'].view(-1, 1, 3)
        _check_mesh(mesh, 'MeshRenderer')
        N, V = mesh.shape[0], mesh.shape[1]
        if uvmap.shape[0] not in (1, N):
            raise ValueError('MeshRenderer: uvmap holds %d maps for %d meshes' % (uvmap.shape[0], N))
        topo = _topology(face, V, mesh.device)
        if self.face_uv.shape[0] != topo[0].shape[0]:
            raise ValueError('MeshRenderer: face_uv has %d faces, face has %d' % (self.face_uv.shape[0], topo[0].shape[0]))
        # flip y-axis following PyTorch3D convention (layer.py:53); corner uvs per face, [F, 3, 2]
        vertex_uv = torch.stack((self.vertex_uv[:, 0], 1 - self.vertex_uv[:, 1]), 1)
        face_uvs = vertex_uv.to(mesh.device)[self.face_uv.to(mesh.device)].contiguous()
        texture = uvmap.detach().to(device=mesh.device, dtype=torch.float32).contiguous()
        focal, princpt = _camera(cam_param, N, mesh.device)
        render, _ = _RenderMesh.apply(mesh, topo, focal, princpt, render_height, render_width, texture, face_uvs)
        return render


# ---- Phong-shaded render (reference render_mesh) -------------------------------------------------------------------------
def _forward_only(mesh, what):
    if torch.is_grad_enabled() and mesh.requires_grad:
        raise NotImplementedError('%s is forward only (the reference renders under torch.no_grad()); pass mesh.detach() '
                                  'or call it under torch.no_grad()' % what)


def _vertex_normals(verts, topo):
    faces, offsets, entries = topo
    normals = torch.empty_like(verts)
    g = _lib.ExaMeshGeometry(verts.shape[0], verts.shape[1], faces.shape[0], 0, 0, verts.data_ptr(), faces.data_ptr(),
                             None, None)
    launch(_lib.MESH, 'exa_mesh_vertex_normals', verts.device, ctypes.byref(g), _ptr(offsets), _ptr(entries), _ptr(normals))
    return normals


def _verts(mesh, what):
    if isinstance(mesh, torch.Tensor) and mesh.dim() == 2:
        mesh = mesh[None]
    _check_mesh(mesh, what)
    _forward_only(mesh, what)
    return mesh.detach().to(torch.float32).contiguous()


def vertex_normals(mesh, face):
    """Area-weighted vertex normals of ``mesh`` [N,V,3] (or [V,3]) with faces ``face`` [F,3] (numpy or tensor): pytorch3d
    ``Meshes.verts_normals_packed`` per mesh, [N,V,3] on the mesh's device.  Forward only."""
    verts = _verts(mesh, 'vertex_normals')
    return _vertex_normals(verts, _topology(face, verts.shape[1], verts.device))


def _rgb(x, what):
    v = np.asarray(x, dtype=np.float64)
    if v.shape not in ((), (3,)) or not np.isfinite(v).all():
        raise ValueError('shade_mesh: %s must be a finite scalar or RGB triple' % what)
    return np.broadcast_to(v, (3,)).tolist()


def _shading(light_location, lights, materials, shininess, background):
    loc = np.asarray(light_location, dtype=np.float64)
    if loc.shape != (3,) or not np.isfinite(loc).all():
        raise ValueError('shade_mesh: light_location must be a finite (x, y, z)')
    if len(lights) != 3 or len(materials) != 3:
        raise ValueError('shade_mesh: lights and materials are (ambient, diffuse, specular)')
    sh = _lib.ExaMeshShading()
    sh.light_location[:] = loc.tolist()
    sh.light_ambient[:], sh.light_diffuse[:], sh.light_specular[:] = [_rgb(c, 'lights[%d]' % i) for i, c in enumerate(lights)]
    sh.material_ambient[:], sh.material_diffuse[:], sh.material_specular[:] = \
        [_rgb(c, 'materials[%d]' % i) for i, c in enumerate(materials)]
    sh.shininess = float(shininess)
    sh.background[:] = _rgb(background, 'background')
    return sh


def shade_mesh(mesh, face, cam_param, render_shape, *, light_location=(0.0, -1.0, 0.0), lights=(0.5, 0.3, 0.2),
               materials=(1.0, 1.0, 0.0), shininess=0.0, background=(1.0, 1.0, 1.0)):
    """Phong-shaded render of the camera-space ``mesh`` [N,V,3] or [V,3] (faces ``face`` [F,3], one topology for all N)
    seen by the pinhole cameras ``cam_param['focal']`` / ``['princpt']`` ([N,2] or [2]) at ``render_shape`` = (H, W):
    the device half of the reference's ``render_mesh`` (module docstring).  ``light_location`` is in the caller's camera
    frame; ``lights`` = (ambient, diffuse, specular) light colours and ``materials`` = (ambient, diffuse, specular)
    material colours, each a scalar or an RGB triple; ``shininess`` >= 0.  The defaults are the reference's
    ``PointLights()`` and ``Materials(specular_color=0, shininess=0)``.  N meshes go in one launch.

    Returns ``(image [N,H,W,3] float32, background colour at empty pixels; pix_to_face [N,H,W] int64, packed n * F + f,
    -1 at empty pixels)``.  Forward only: raises NotImplementedError for a ``mesh`` that requires grad under grad mode."""
    verts = _verts(mesh, 'shade_mesh')
    sh = _shading(light_location, lights, materials, shininess, background)
    H, W = int(render_shape[0]), int(render_shape[1])
    N, V = verts.shape[0], verts.shape[1]
    device = verts.device
    topo = _topology(face, V, device)
    faces = topo[0]
    focal, princpt = _camera(cam_param, N, device)
    ws = _lib.mesh_workspace_sizes(N, faces.shape[0], H, W)
    face_ws = torch.empty(int(ws.face_bytes), dtype=torch.uint8, device=device)
    bin_ws = torch.empty(int(ws.bin_bytes), dtype=torch.uint8, device=device)
    normals = _vertex_normals(verts, topo)
    image = torch.empty((N, H, W, 3), dtype=torch.float32, device=device)
    pix_to_face = torch.empty((N, H, W), dtype=torch.int64, device=device)
    g = _geometry(verts, faces, focal, princpt, H, W)
    launch(_lib.MESH, 'exa_mesh_forward_shaded', device, ctypes.byref(g), ctypes.byref(sh), _ptr(normals), _ptr(face_ws),
           _ptr(bin_ws), _ptr(pix_to_face), None, _ptr(image))
    return image, pix_to_face


def _composite(render, is_bkg, bkg, blend_ratio):
    """The last lines of the reference's ``render_mesh``, as written: numpy's dtype promotion is the reference's."""
    fg = render * blend_ratio + bkg / 255 * (1 - blend_ratio)
    return fg * (1 - is_bkg) * 255 + bkg * is_bkg


def _host_array(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x))


def render_mesh(mesh, face, cam_param, bkg, blend_ratio=1.0):
    """Drop-in for the reference's ``render_mesh`` (``avatar/common/utils/vis.py:73-109``, and the numpy-input copy in
    ``fitting/common/utils/vis.py:18-53``): the camera-space ``mesh`` [V,3] (torch on any device, or numpy), ``face``
    [F,3], ``cam_param['focal']`` / ``['princpt']`` [2] (torch or numpy; other keys are ignored), ``bkg`` a numpy
    [H,W,3] image on a 0-255 scale that sets the render's size.  Shades on the current ROCm device, copies the image
    and the background mask to the host and composites as the reference does; returns the numpy image (the callers
    apply ``.astype(np.uint8)``)."""
    device = torch.device('cuda', torch.cuda.current_device())
    mesh = torch.as_tensor(_host_array(mesh) if not isinstance(mesh, torch.Tensor) else mesh)
    mesh = mesh.to(device=device, dtype=torch.float32)
    cam = {k: torch.as_tensor(_host_array(cam_param[k])) for k in ('focal', 'princpt')}
    with torch.no_grad():
        image, pix_to_face = shade_mesh(mesh[None], face, cam, (bkg.shape[0], bkg.shape[1]))
    render = image[0].cpu().numpy()
    is_bkg = (pix_to_face[0] == -1)[..., None].float().cpu().numpy()     # the reference's (zbuf <= 0): [H, W, 1]
    return _composite(render, is_bkg, bkg, blend_ratio)
