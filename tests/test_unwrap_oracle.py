"""CPU tests of the face-texture unwrap: the oracle (tests/unwrap_oracle.py) against the golden file that the reference's
own ``XY2UV`` wrote (tests/golden/make_golden_unwrap.py), ``uv_region_mask`` against the reference's loops, and the host
side of the new C entry points: declared, bound, and every argument error reported before any GPU work."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import _lib, build
from exavatar_release_amd import unwrap as module
from tests import unwrap_oracle as uo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 4                 # the project's bar: another float32 evaluation stays within 4 x the reference's own float32 error
BAD = ctypes.c_void_p(0x1000)      # never dereferenced: every call below fails validation first, or has nothing to do
INVALID, NULLPTR = -1, -2
SCENES = ('a', 'b')


@functools.lru_cache(maxsize=None)
def golden():
    path = os.path.join(ROOT, 'tests', 'golden', 'ref_unwrap.npz')
    assert os.path.getsize(path) < 1_000_000
    return dict(np.load(path))


def scene(name):
    g = golden()
    return {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + '_')}


@functools.lru_cache(maxsize=None)
def oracle32(name):
    sc = scene(name)
    return uo.unwrap(sc['img'], sc['verts'], sc['face'], sc['focal'], sc['princpt'], sc['pix_to_face_xy'],
                     sc['pix_to_face_uv'], sc['bary32'])


@pytest.mark.parametrize('name', SCENES)
def test_the_fixtures_have_no_ambiguous_pixel_or_texel(name):
    sc = scene(name)
    assert sc['amb_xy'].shape == (2, 40, 56) and sc['amb_uv'].shape == (48, 40)
    assert not sc['amb_xy'].any() and not sc['amb_uv'].any()
    assert sc['img'].shape == (2, 3, 40, 56) and sc['verts'].shape == (2, 2 * 13 * 17, 3)
    assert not np.array_equal(sc['face_uv'], sc['face']), 'the atlas is stored under an index set of its own'
    # the stored rasters are the oracle's on the stored numbers
    xy, uv = uo.scene_rasters(sc)
    assert np.array_equal(xy['pix_to_face'].numpy(), sc['pix_to_face_xy'])
    assert np.array_equal(uv['pix_to_face'].numpy(), sc['pix_to_face_uv'])
    assert np.array_equal(uv['bary'].numpy().astype(np.float32), sc['bary32'])
    assert np.abs(sc['bary64'] - sc['bary32']).max() < 1e-5       # the float64 run scales u Wu, v Hu in float64


def test_the_wrap_around_is_on_both_sides():
    """Scene a: background pixels, the hidden last face is visible; scene b: no background pixel, it stays invisible."""
    for name, shown in (('a', True), ('b', False)):
        sc = scene(name)
        F = sc['face'].shape[0]
        p = sc['pix_to_face_xy']
        assert not any((p[n] == n * F + F - 1).any() for n in range(2)), 'the last face is hit by no pixel'
        assert all((p[n] == -1).any() == shown for n in range(2))
        vis = uo.visible_faces(p, F)
        assert vis[:, F - 1].all() == shown and vis[:, F - 1].any() == shown
        last = sc['pix_to_face_uv'] == F - 1
        assert last.sum() >= 2
        assert sc['mask32'][:, :, last].all() == shown and sc['mask32'][:, :, last].any() == shown
        assert oracle32(name)[1][:, :, last].all() == shown
    p = np.array([[[0, 1], [1, 1]], [[-1, 5], [9, 3]]])          # item 1: 5 -> face 2, 3 -> face 0, 9 is out of range
    assert uo.visible_faces(p, 3).tolist() == [[True, True, False], [True, False, True]]


@pytest.mark.parametrize('name', SCENES)
def test_oracle_against_the_reference(name):
    sc = scene(name)
    u32, m32 = oracle32(name)
    assert np.array_equal(m32, sc['mask32']), 'mask must equal the reference\'s float32 run exactly'
    e_ref = np.abs(sc['uvmap32'].astype(np.float64) - sc['uvmap64']).max()
    e = np.abs(u32.astype(np.float64) - sc['uvmap64']).max()
    ref32 = np.where(sc['mask32'], sc['uvmap32'], np.float32(0))            # the reference's -0.0 at empty texels
    bit_equal = np.array_equal(u32.view(np.int32), ref32.view(np.int32))
    print('%s: e_ref %.3e, oracle32 e %.3e, bit-equal to the reference\'s CPU float32 run: %s (max diff %.3e)' % (
        name, e_ref, e, bit_equal, np.abs(u32 - ref32).max()))
    assert e_ref > 0 and e <= FACTOR * e_ref
    assert (u32[~m32] == 0).all() and not np.signbit(u32[~m32]).any()
    # sample positions outside the image occur among the sampled texels
    assert (u32[m32] == 0).any()
    # the float64 oracle on the float64 barycentrics is the reference's float64 run to rounding
    u64, m64 = uo.unwrap(sc['img'], sc['verts'], sc['face'], sc['focal'], sc['princpt'], sc['pix_to_face_xy'],
                         sc['pix_to_face_uv'], sc['bary64'], dtype=np.float64)
    assert np.array_equal(m64, sc['mask32']) and np.abs(u64 - sc['uvmap64']).max() <= 1e-12


def test_the_reference_samples_a_culled_last_face_and_the_oracle_does_not():
    """A mesh wholly behind the camera: every pixel is background, the wrap-around marks the (culled) last face, and the
    reference's float32 run samples the image through the mirrored projection -- finite values, recorded by the golden
    script.  The package writes 0 / False there (the one deliberate difference, include/exa_mesh.h)."""
    g = golden()
    assert bool(g['behind_ref32_finite']) and bool(g['behind_ref32_last_mask_all'])
    sc = scene('a')
    verts = sc['verts'] * np.array([1, 1, -1], dtype=np.float32)
    p = np.full((2, 40, 56), -1, dtype=np.int64)
    assert uo.visible_faces(p, sc['face'].shape[0])[:, -1].all()
    u, m = uo.unwrap(sc['img'], verts, sc['face'], sc['focal'], sc['princpt'], p, sc['pix_to_face_uv'], sc['bary32'])
    assert not m.any() and (u == 0).all()


def test_uv_region_mask_is_the_references_loops():
    sc = scene('a')
    rng = np.random.RandomState(5)
    V = sc['verts'].shape[1]
    keep = rng.uniform(size=V) > 0.15
    p2f = torch.from_numpy(sc['pix_to_face_uv'])
    want = uo.uv_region_mask_loop(sc['pix_to_face_uv'], sc['face'], keep)
    got = exa.uv_region_mask(p2f, sc['face'], torch.from_numpy(keep))
    assert got.dtype == torch.bool and np.array_equal(got.numpy(), want)
    assert 0 < want.sum() < (sc['pix_to_face_uv'] >= 0).sum()
    assert np.array_equal(exa.uv_region_mask(p2f, torch.from_numpy(sc['face']), torch.ones(V, dtype=torch.bool)).numpy(),
                          sc['pix_to_face_uv'] >= 0)
    with pytest.raises(ValueError, match='uv_region_mask: vertex_keep must be a bool'):
        exa.uv_region_mask(p2f, sc['face'], torch.ones(V))
    with pytest.raises(ValueError, match=r'uv_region_mask: pix_to_face_uv names a face outside \[0, 10\)'):
        exa.uv_region_mask(p2f, sc['face'][:10], torch.from_numpy(keep))


# ---- the host side of the C entry points --------------------------------------------------------------------------------
ENTRY_POINTS = (('exa_mesh_forward_ortho', 7), ('exa_mesh_unwrap_workspace_size', 3), ('exa_mesh_unwrap', 8))


def test_the_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'exa_mesh.h')).read()
    lib = _lib.load()
    for name, n_args in ENTRY_POINTS:
        assert re.search(r'\bint %s\(' % name, header), name
        assert name in _lib.MESH.signatures and len(getattr(lib, name).argtypes) == n_args
    assert 'ExaMeshUnwrap' in _lib.MESH.structs and 'typedef struct ExaMeshUnwrap' in header
    assert lib.exa_mesh_version() == 100 and _lib.MESH.version == 100 and len(_lib.ABIS) == 6
    assert build.SOURCES['unwrap.hip'] == ['-ffp-contract=off']
    for name in ('XY2UV', 'get_face_index_map_uv', 'TextureUnwrap', 'uv_region_mask'):
        assert name in exa.__all__ and getattr(exa, name) is getattr(module, name)
    assert 'XY2UV' in exa.__doc__ and module.MAX_CHANNELS == 8


def test_the_flag_workspace_size():
    lib = _lib.load()
    err = lib.exa_mesh_last_error
    for B, F, want in ((1, 1, 256), (2, 128, 256), (2, 129, 512), (8, 9976, 79872), (0, 5, 0), (5, 0, 0)):
        assert _lib.unwrap_workspace_size(B, F) == want, (B, F)
    out = ctypes.c_uint64()
    assert lib.exa_mesh_unwrap_workspace_size(-1, 1, ctypes.byref(out)) == INVALID and err() == b'exa_mesh: negative size'
    assert lib.exa_mesh_unwrap_workspace_size(1 << 13, 1 << 12, ctypes.byref(out)) == INVALID and b'2^24 faces' in err()
    assert lib.exa_mesh_unwrap_workspace_size(1, 1, None) == NULLPTR and b'out_bytes is NULL' in err()


def _unwrap(lib, ws=BAD, ws_bytes=1 << 20, maps=(1, 1), sums=(0, 0), desc=True, **over):
    f = dict(B=2, V=10, F=6, C=3, H=8, W=9, Hu=5, Wu=7)
    f.update({k: v for k, v in over.items() if k in f})
    ptrs = ['img', 'verts', 'faces', 'focal', 'princpt', 'pix_to_face_xy', 'pix_to_face_uv', 'bary_uv', 'uv_weight',
            'face_valid']
    u = _lib.ExaMeshUnwrap(*[f[k] for k in ('B', 'V', 'F', 'C', 'H', 'W', 'Hu', 'Wu')],
                           *[None if over.get(k) == 'null' else BAD for k in ptrs])
    return lib.exa_mesh_unwrap(ctypes.byref(u) if desc else None, ws, ws_bytes, *[BAD if x else None for x in maps + sums], None)


def test_exa_mesh_unwrap_checks_its_arguments():
    lib = _lib.load()
    err = lib.exa_mesh_last_error
    assert _unwrap(lib, desc=False) == NULLPTR and b'unwrap descriptor is NULL' in err()
    for size in ('B', 'V', 'F', 'H', 'W', 'Hu', 'Wu'):
        assert _unwrap(lib, **{size: -1}) == INVALID and err() == b'exa_mesh: negative size', size
    for C in (0, 9, -1):
        assert _unwrap(lib, C=C) == INVALID and b'unwrap: channels must be 1 .. 8' in err()
    assert _unwrap(lib, H=8193) == INVALID and b'larger than 8192 x 8192' in err()
    assert _unwrap(lib, Wu=8193) == INVALID and b'larger than 8192 x 8192' in err()
    assert _unwrap(lib, B=1 << 13, F=1 << 12) == INVALID and b'2^24 faces' in err()
    assert _unwrap(lib, maps=(1, 0)) == INVALID and b'pass uvmap and mask, or neither' in err()
    assert _unwrap(lib, sums=(0, 1)) == INVALID and b'pass tex_sum and mask_sum, or neither' in err()
    assert _unwrap(lib, maps=(0, 0)) == NULLPTR and b'unwrap: no output' in err()
    for name in ('pix_to_face_uv', 'bary_uv'):
        assert _unwrap(lib, **{name: 'null'}) == NULLPTR and b'pix_to_face_uv / bary_uv is NULL' in err()
    assert _unwrap(lib, sums=(1, 1), uv_weight='null') == NULLPTR and b'uv_weight is NULL' in err()
    for name in ('faces', 'verts', 'focal', 'princpt'):
        assert _unwrap(lib, **{name: 'null'}) == NULLPTR and b'faces / verts / focal / princpt is NULL' in err()
    for name in ('img', 'pix_to_face_xy'):
        assert _unwrap(lib, **{name: 'null'}) == NULLPTR and b'img / pix_to_face_xy is NULL' in err()
    assert _unwrap(lib, ws=None) == NULLPTR and b'flag_ws is NULL' in err()
    assert _unwrap(lib, ws_bytes=255) == INVALID and b'smaller than exa_mesh_unwrap_workspace_size' in err()
    assert _unwrap(lib, B=0) == 0 and _unwrap(lib, Hu=0) == 0 and _unwrap(lib, Wu=0, maps=(0, 0), sums=(1, 1)) == 0
    with pytest.raises(RuntimeError, match='exa_mesh: unwrap: channels must be 1 .. 8'):
        _lib.MESH.check(_unwrap(lib, C=9))


def test_exa_mesh_forward_ortho_checks_its_arguments():
    lib = _lib.load()
    err = lib.exa_mesh_last_error

    def call(g, ws=(BAD, BAD), p2f=BAD):
        return lib.exa_mesh_forward_ortho(ctypes.byref(g) if g is not None else None, ws[0], ws[1], p2f, None, None, None)
    G = _lib.ExaMeshGeometry
    assert call(None) == NULLPTR and b'geometry is NULL' in err()
    assert call(G(1, 3, 1, -1, 4, BAD, BAD, None, None)) == INVALID and b'negative size' in err()
    assert call(G(1, 3, 1, 4, 4, None, BAD, None, None)) == NULLPTR and b'verts is NULL' in err()
    assert call(G(1, 3, 1, 4, 4, BAD, None, None, None)) == NULLPTR and b'faces' in err()
    assert call(G(1, 3, 1, 4, 4, BAD, BAD, None, None), p2f=None) == NULLPTR and b'pix_to_face is NULL' in err()
    assert call(G(1, 3, 1, 4, 4, BAD, BAD, None, None), ws=(None, BAD)) == NULLPTR and b'workspace is NULL' in err()
    assert call(G(0, 3, 1, 4, 4, None, None, None, None)) == 0 and call(G(1, 3, 1, 0, 4, BAD, BAD, None, None)) == 0
    # the perspective entry point still wants its cameras
    assert lib.exa_mesh_forward(ctypes.byref(G(1, 3, 1, 4, 4, BAD, BAD, None, None)), None, BAD, BAD, BAD, None, None, None,
                                None) == NULLPTR and b'faces / focal / princpt is NULL' in err()


def test_the_python_layer_refuses_by_name_without_a_device():
    with pytest.raises(ValueError, match=r'get_face_index_map_uv: vertex_uv must be a \[N, U, 2\] tensor'):
        exa.get_face_index_map_uv(torch.zeros(4, 2), np.zeros((1, 3), dtype=np.int64), (8, 8))
    with pytest.raises(RuntimeError, match='get_face_index_map_uv runs on a ROCm device only'):
        exa.get_face_index_map_uv(torch.zeros(1, 4, 2), np.zeros((1, 3), dtype=np.int64), (8, 8))
    with pytest.raises(TypeError, match='TextureUnwrap: xy2uv must be an XY2UV'):
        exa.TextureUnwrap(None, torch.zeros(4, 4))
