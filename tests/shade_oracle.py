"""Float64 restatement of the Phong-shaded mesh render (``exavatar_release_amd.mesh.shade_mesh`` / ``render_mesh``).

Test infrastructure only: the package never imports it.  The semantics are those of the docstring of
``exavatar_release_amd/mesh.py`` (pytorch3d's ``_compute_vertex_normals``, ``phong_shading`` and ``softmax_rgb_blend`` for
one face per pixel, in the caller's camera frame) on top of ``tests/mesh_oracle.rasterize``.  The normals come from an
explicit loop over the faces, not from the package's ``p3d_standins``.  ``shade`` takes the per-pixel face and
barycentrics as inputs, so a GPU test can evaluate it at the kernel's own decisions.
"""
import math

import numpy as np
import torch

from tests import mesh_oracle as mo

EPS = 1e-6
# the reference's configuration: PointLights() (its (0, 1, 0) is (0, -1, 0) in the camera frame), Materials(
# specular_color=0, shininess=0), TexturesVertex of ones, background (1, 1, 1)
REFERENCE = {'light_location': (0.0, -1.0, 0.0), 'lights': (0.5, 0.3, 0.2), 'materials': (1.0, 1.0, 0.0),
             'shininess': 0.0, 'background': (1.0, 1.0, 1.0)}


def vertex_normals(verts, faces):
    """verts [N,V,3], faces [F,3] -> (normals [N,V,3], unnormalised sums [N,V,3]), float64 numpy.  Every face adds, at
    each corner k, cross(v_{k+1} - v_k, v_{k+2} - v_k); the sums are normalised as x / max(|x|, 1e-6)."""
    v = (verts.detach().double().cpu().numpy() if isinstance(verts, torch.Tensor) else np.asarray(verts, np.float64))
    f = (faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)).astype(np.int64)
    if v.ndim == 2:
        v = v[None]
    corners = v[:, f]                                               # [N, F, 3 corners, 3]
    cross = np.stack([np.cross(corners[:, :, (k + 1) % 3] - corners[:, :, k], corners[:, :, (k + 2) % 3] - corners[:, :, k])
                      for k in range(3)], 2)                        # [N, F, 3 corners, 3]
    acc = np.zeros_like(v)
    for i in range(f.shape[0]):
        for k in range(3):
            acc[:, f[i, k]] += cross[:, i, k]
    norm = np.linalg.norm(acc, axis=-1, keepdims=True)
    return acc / np.maximum(norm, EPS), acc


def _rgb(x, dev):
    return torch.as_tensor(np.broadcast_to(np.asarray(x, dtype=np.float64), (3,)).copy(), device=dev)


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True).clamp_min(EPS)


def shade(verts, faces, normals, face, bary, light_location=REFERENCE['light_location'], lights=REFERENCE['lights'],
          materials=REFERENCE['materials'], shininess=REFERENCE['shininess'], background=REFERENCE['background']):
    """Phong colour of every pixel.  verts / normals [N,V,3], faces [F,3], face [N,H,W] (UNPACKED face index, -1 for
    background), bary [N,H,W,3] perspective-correct barycentrics.  Returns (image [N,H,W,3] float64, cos [N,H,W]: n^ . l^,
    0 at background)."""
    dev = face.device
    verts = torch.as_tensor(verts).double().to(dev)
    normals = torch.as_tensor(normals).double().to(dev)
    faces = torch.as_tensor(faces).long().to(dev)
    bary = bary.double().to(dev)
    N = verts.shape[0]
    cov = face >= 0
    fv = faces[face.clamp_min(0)]                                   # [N,H,W,3]
    nidx = torch.arange(N, device=dev)[:, None, None, None]
    w = torch.where(cov[..., None], bary, torch.zeros_like(bary))[..., None]
    p = (w * verts[nidx, fv]).sum(-2)
    n = (w * normals[nidx, fv]).sum(-2)
    L = _rgb(light_location, dev)
    l, nh, v = _unit(L - p), _unit(n), _unit(-p)
    cos = (nh * l).sum(-1)
    r = -l + 2 * cos[..., None] * nh
    a = (v * r).sum(-1).clamp_min(0) * (cos > 0)
    spec = torch.pow(a, float(shininess))
    La, Ld, Ls = (_rgb(c, dev) for c in lights)
    Ma, Md, Ms = (_rgb(c, dev) for c in materials)
    col = La * Ma + Ld * Md * cos.clamp_min(0)[..., None] + Ls * Ms * spec[..., None]
    image = torch.where(cov[..., None], col, _rgb(background, dev).expand_as(col))
    return image, torch.where(cov, cos, torch.zeros_like(cos))


def render(verts, faces, focal, princpt, H, W, frags=None, **shading):
    """The whole render in float64: mesh_oracle.rasterize, vertex_normals, shade.  verts [N,V,3], focal / princpt [N,2]
    or [2].  Returns (image [N,H,W,3], cos [N,H,W], fragments dict of mesh_oracle.rasterize)."""
    if frags is None:
        frags = mo.rasterize(verts, faces, focal, princpt, H, W)
    normals, _ = vertex_normals(verts, faces)
    image, cos = shade(verts, faces, torch.from_numpy(normals), frags['face'], frags['bary'], **shading)
    return image, cos, frags


def reference_composite(images, zbuf, bkg, blend_ratio):
    """The last four lines of the reference's render_mesh (vis.py:105-109), as written: images [1,H,W,C>=3] and zbuf
    [1,H,W,1] torch tensors (pytorch3d's layout), bkg a numpy [H,W,3] image on a 0-255 scale."""
    is_bkg = (zbuf <= 0).float().cpu().numpy()[0]
    render = images[0, :, :, :3].cpu().numpy()
    fg = render * blend_ratio + bkg / 255 * (1 - blend_ratio)
    render = fg * (1 - is_bkg) * 255 + bkg * is_bkg
    return render


# ---- test scenes -------------------------------------------------------------------------------------------------------
def smplx_sized_scene(H, W, seed=0, N=1):
    """~SMPL-X-sized body mesh (10 242 vertices, 20 480 faces; SMPL-X has 10 475 / 20 908): a perturbed level-5
    icosphere stretched into a standing ellipsoid 2.5 m from a pinhole camera that frames it at H x W.  Returns a dict
    of float32 CPU tensors: verts [N,V,3] (camera space), faces [F,3], focal / princpt [N,2]; mesh n > 0 is shifted a
    little and turned about the vertical axis."""
    g = torch.Generator().manual_seed(seed)
    v, f = mo.icosphere(5)
    bump = 1 + 0.02 * torch.randn(v.shape[0], 1, generator=g, dtype=torch.float64)
    body = v * bump * torch.tensor([0.35, 0.85, 0.25], dtype=torch.float64)
    verts = []
    for n in range(N):
        a = 0.4 * n
        R = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], dtype=torch.float64)
        verts.append(body @ R.T + torch.tensor([0.03 * n, 0.1 - 0.02 * n, 2.5 + 0.1 * n], dtype=torch.float64))
    verts = torch.stack(verts)
    focal = torch.tensor([[0.8 * H, 0.8 * H]], dtype=torch.float64).repeat(N, 1)
    princpt = torch.tensor([[W / 2 - 0.31, H / 2 + 0.17]], dtype=torch.float64).repeat(N, 1)
    return {'verts': verts.float(), 'faces': f, 'focal': focal.float(), 'princpt': princpt.float()}
