"""Generates tests/golden/ref_unwrap.npz by EXECUTING the reference's own ``XY2UV``.

``/root/reference/fitting/common/nets/layer.py`` cannot be imported here (it imports pytorch3d and the fitting config at
the top), so the source text of ``class XY2UV`` is cut out of the file with ``ast`` and exec'd unchanged in a namespace
holding torch / nn / F / np, with ``get_face_index_map_uv`` and ``get_face_index_map_xy`` bound to adaptors over
``tests/mesh_oracle.rasterize`` that return pytorch3d-shaped fragments.  pytorch3d is not installed, so this golden pins
everything in ``XY2UV.forward`` EXCEPT pytorch3d's own rasterizer; that part stays pinned by ``tests/mesh_oracle.py``, as
for the face render.  ``Tensor.cuda()`` returns a copy for the duration (this container has no GPU; a copy, not the tensor
itself, because the reference writes -1 into ``torch.from_numpy(face).cuda()`` and on a GPU that is a copy of ``face``).
The float64 run is the same source on the same numbers with ``Tensor.float()`` widened to ``.double()``.
Run from the repo root:  python tests/golden/make_golden_unwrap.py
Nothing here is read at test time on the GPU box -- only the .npz travels.

Scenes (``tests/unwrap_oracle.unwrap_scene``; B = 2 with a camera per item, image 40 x 56, UV map 48 x 40, C = 3):
  a   patch 1 leaves background pixels; the last face lies off the image, hidden, and the reference's wrap-around
      (``valid_face_mask[-1] = 1``) makes it visible.  Asserted below on the reference's output.
  b   patch 1 overhangs the image on every side: no background pixel, and the hidden last face stays invisible.  Asserted.
Both: the float64 oracle reports ZERO ambiguous pixels in the image raster and zero ambiguous texels in the UV raster
(``unwrap_oracle.clean_scene`` searches seeds for it); the flags are stored and the tests re-assert them.
  behind   scene a pushed wholly behind the camera (Z < 0): what the reference's float32 run gives where only the
      wrap-around marks the (culled) last face.  Recorded as ``behind_*``; the package writes 0 / False there.
"""
import ast
import collections
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import mesh_oracle as mo          # noqa: E402
from tests import unwrap_oracle as uo        # noqa: E402

REF = '/root/reference/fitting/common/nets/layer.py'
src = open(REF).read()
Fragments = collections.namedtuple('Fragments', ['pix_to_face', 'zbuf', 'bary_coords', 'dists'])


def get_face_index_map_uv(vertex_uv, face_uv, uvmap_shape):
    """[1,U,2] in the run's dtype -> pytorch3d-shaped fragments; the scaling is the reference's, in that dtype."""
    fr = uo.rasterize_uv(vertex_uv[0], face_uv[0], uvmap_shape[0], uvmap_shape[1], dtype=vertex_uv.dtype)
    dt = vertex_uv.dtype
    return Fragments(fr['pix_to_face'][None, :, :, None], fr['zbuf'].to(dt)[None, :, :, None],
                     fr['bary'].to(dt)[None, :, :, None, :], None)


def get_face_index_map_xy(mesh, face, cam_param, render_shape):
    fr = mo.rasterize(mesh, torch.from_numpy(face), cam_param['focal'], cam_param['princpt'], render_shape[0], render_shape[1])
    return Fragments(fr['pix_to_face'][..., None], fr['zbuf'].to(mesh.dtype)[..., None],
                     fr['bary'].to(mesh.dtype)[:, :, :, None, :], None)


ns = {'torch': torch, 'nn': nn, 'F': F, 'np': np, 'get_face_index_map_uv': get_face_index_map_uv,
      'get_face_index_map_xy': get_face_index_map_xy}
lines = src.splitlines()
for node in ast.parse(src).body:
    if isinstance(node, ast.ClassDef) and node.name == 'XY2UV':
        exec('\n'.join(lines[node.lineno - 1: node.end_lineno]), ns)


def run_reference(sc, dtype):
    """The reference's XY2UV on a scene, in float32 or -- ``.float()`` widened -- float64."""
    _float = torch.Tensor.float
    if dtype == torch.float64:
        torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        m = ns['XY2UV'](sc['vertex_uv'].copy(), sc['face_uv'].copy(), uo.UVMAP)
        cam = {'focal': torch.from_numpy(sc['focal']).to(dtype), 'princpt': torch.from_numpy(sc['princpt']).to(dtype)}
        face = sc['face'].copy()
        uvmap, mask = m(torch.from_numpy(sc['img']).to(dtype), torch.from_numpy(sc['verts']).to(dtype), face, cam)
        assert np.array_equal(face, sc['face']), 'the reference must not write into the caller\'s face'
    finally:
        torch.Tensor.float = _float
    assert uvmap.dtype == dtype and m.bary_coords_uv.dtype == dtype
    return uvmap.numpy(), mask.numpy(), m.pix_to_face_uv.numpy(), m.bary_coords_uv.numpy()


_cuda = torch.Tensor.cuda
torch.Tensor.cuda = lambda self, *a, **k: self.clone()
try:
    rec = {}
    for name, fill in (('a', False), ('b', True)):
        sc, xy, uv = uo.clean_scene(fill)
        nF = sc['face'].shape[0]
        u32, m32, p2f_uv, bary32 = run_reference(sc, torch.float32)
        u64, m64, p2f_uv64, bary64 = run_reference(sc, torch.float64)
        assert np.array_equal(p2f_uv, p2f_uv64) and np.array_equal(m32, m64)
        assert np.array_equal(p2f_uv, uv['pix_to_face'].numpy())
        p2f_xy = xy['pix_to_face'].numpy()
        amb_xy = (xy['edge_amb'] | xy['z_amb']).numpy()
        amb_uv = (uv['edge_amb'] | uv['z_amb']).numpy()
        assert not amb_xy.any() and not amb_uv.any()
        # the last face is hidden in both scenes; the wrap-around shows it in a, and only there
        last = nF - 1
        has_bg = [(p2f_xy[n] == -1).any() for n in range(2)]
        hit_last = [(p2f_xy[n] == n * nF + last).any() for n in range(2)]
        last_texels = p2f_uv == last
        assert last_texels.sum() > 0 and not any(hit_last)
        if fill:
            assert not any(has_bg) and not m32[:, :, last_texels].any(), 'b: no background pixel, the last face stays invisible'
        else:
            assert all(has_bg) and m32[:, :, last_texels].all(), 'a: the wrap-around makes the hidden last face visible'
        assert (sc['verts'][..., 2] > 1.0).all()
        # the oracle agrees with the reference (tests/test_unwrap_oracle.py repeats this from the file)
        o32, om32 = uo.unwrap(sc['img'], sc['verts'], sc['face'], sc['focal'], sc['princpt'], p2f_xy, p2f_uv, bary32)
        e_ref, e = np.abs(u32 - u64).max(), np.abs(o32 - u64).max()
        assert np.array_equal(om32, m32) and e <= 4 * e_ref, (name, e, e_ref)
        # sample positions outside the image occur among the sampled texels (a tap is dropped, or all four)
        vis = uo.visible_faces(p2f_xy, nF)
        n_sampled = int(m32[:, 0].sum())
        rec.update({name + '_' + k: v for k, v in sc.items() if k != 'seed'})
        rec.update({name + '_seed': np.int64(sc['seed']), name + '_pix_to_face_xy': p2f_xy, name + '_pix_to_face_uv': p2f_uv,
                    name + '_amb_xy': amb_xy, name + '_amb_uv': amb_uv, name + '_bary32': bary32, name + '_bary64': bary64,
                    name + '_uvmap32': u32, name + '_uvmap64': u64, name + '_mask32': m32})
        print('%s: seed %d, %d of %d faces visible (item 0), %d sampled texels, e_ref %.3e, oracle32 e %.3e, bit-equal %s, '
              'max |oracle32 - ref32| %.3e' % (name, sc['seed'], vis[0].sum(), nF, n_sampled, e_ref, e,
                                               np.array_equal(o32, np.where(m32, u32, 0)), np.abs(o32 - u32).max()))

    # behind: what the reference's float32 run gives when every Z is negative (nothing is rasterized, every pixel is
    # background, and the wrap-around marks the culled last face)
    sc = {k[2:]: v for k, v in rec.items() if k.startswith('a_')}
    sc['verts'] = sc['verts'] * np.array([1, 1, -1], dtype=np.float32)
    u32, m32, p2f_uv, _ = run_reference(sc, torch.float32)
    last_texels = p2f_uv == sc['face'].shape[0] - 1
    rec['behind_ref32_finite'] = np.bool_(np.isfinite(u32).all())
    rec['behind_ref32_last_mask_all'] = np.bool_(m32[:, :, last_texels].all())
    rec['behind_ref32_last_nonzero'] = np.int64((u32[:, :, last_texels] != 0).sum())
    assert not m32[:, :, ~last_texels].any()
    print('behind: reference float32 finite %s, mask on the last face\'s texels all True %s, %d of %d values nonzero' % (
        rec['behind_ref32_finite'], rec['behind_ref32_last_mask_all'], rec['behind_ref32_last_nonzero'],
        u32[:, :, last_texels].size))
finally:
    torch.Tensor.cuda = _cuda
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ref_unwrap.npz')
np.savez_compressed(path, **rec)
print('wrote', path, os.path.getsize(path), 'bytes')
assert os.path.getsize(path) < 1_000_000
