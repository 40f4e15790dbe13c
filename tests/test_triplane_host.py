"""CPU tests of the triplane lookup's host side: invalid arguments fail with a negative status before any GPU work, the
plan's pure-Python layout helpers keep their bounds, and the Python surface refuses what it does not support.  The ABI
itself (include/exa_triplane.h against its binding) is checked by tests/test_abi.py."""
import ctypes

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import _lib
from exavatar_release_amd import triplane as tp

BAD = ctypes.c_void_p(0x1000)      # never dereferenced: every call below fails validation first


def test_plan_keys_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()

    def keys(N=10, H=4, W=4, coords=BAD, face=BAD, out=BAD):
        return lib.exa_triplane_plan_keys(N, H, W, coords, face, out, None)

    assert keys(N=-1) < 0
    assert keys(N=(1 << 27) + 1) < 0
    assert keys(H=0) < 0
    assert keys(W=-3) < 0
    assert keys(H=1 << 14, W=1 << 14) < 0 and b'texels' in lib.exa_triplane_last_error()
    for k in ('coords', 'face', 'out'):
        assert keys(**{k: None}) == -2, k
    assert keys(N=0, coords=None, face=None, out=None) == 0      # nothing to do


def test_forward_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()

    def fwd(N=10, C=32, H=4, W=4, body=BAD, face=BAD, coords=BAD, sel=BAD, out=BAD):
        return lib.exa_triplane_forward(N, C, H, W, body, face, coords, sel, out, None)

    assert fwd(C=0) == -1 and b'C must be' in lib.exa_triplane_last_error()
    assert fwd(C=1025) < 0
    assert fwd(N=-2) < 0
    assert fwd(H=0) < 0
    for k in ('body', 'face', 'coords', 'sel', 'out'):
        assert fwd(**{k: None}) == -2, k
    assert b'NULL' in lib.exa_triplane_last_error()
    assert fwd(N=0, body=None, face=None, coords=None, sel=None, out=None) == 0


def test_backward_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()

    def bwd(N=10, C=32, H=4, W=4, coords=BAD, g=BAD, ent=BAD, seg=BAD, tex=BAD, wg=BAD, nwg=1, maxseg=8, gb=BAD, gf=BAD):
        return lib.exa_triplane_backward(N, C, H, W, coords, g, ent, seg, tex, wg, nwg, maxseg, gb, gf, None)

    assert bwd(C=0) < 0
    assert bwd(W=0) < 0
    assert bwd(nwg=0) < 0
    assert bwd(maxseg=0) < 0
    assert bwd(C=32, maxseg=513) < 0 and b'max_wg_segments' in lib.exa_triplane_last_error()
    assert bwd(C=1, maxseg=16384, gf=None) == -2      # within the LDS bound: fails only on the NULL
    for k in ('coords', 'g', 'ent', 'seg', 'tex', 'wg', 'gb', 'gf'):
        kw = {k: None}
        if k != 'gb':
            kw['gb'] = BAD
        assert bwd(**kw) == -2, k
    # N = 0 still writes the zero gradients: the planes and tables are needed, the row arrays are not
    assert bwd(N=0, coords=None, g=None, ent=None, gb=None) == -2
    assert bwd(N=0, coords=None, g=None, ent=None, seg=None) == -2


def test_segment_length_fits_the_longest_list_into_one_workgroup():
    assert tp.segment_length(0, 32) == 32
    assert tp.segment_length(3082, 32) == 32                 # 97 segments <= 512
    assert tp.segment_length(512 * 32, 32) == 32
    assert tp.segment_length(512 * 32 + 1, 32) == 64
    for C in (1, 3, 32, 33, 1024):
        for n in (0, 1, 100, 5000, 10 ** 6):
            S = tp.segment_length(n, C)
            assert S >= 32 and S & (S - 1) == 0
            assert -(-n // S) * C * 4 <= tp.MAX_LDS


def test_workgroup_packing_covers_every_texel_once_within_bounds():
    rng = np.random.default_rng(0)
    for C in (1, 3, 32, 33, 256):
        nseg = rng.integers(0, 6, size=5000)
        nseg[rng.integers(0, 5000, size=20)] = 300             # texels longer than a workgroup pass
        nseg[:700] = 0                                       # a long empty stretch
        wg, most = tp.pack_workgroups(nseg, C)
        assert wg.dtype == np.int32 and wg[0] == 0 and wg[-1] == nseg.size
        assert np.all(np.diff(wg) >= 1)
        G = C // 4 if C % 4 == 0 else C
        slots = max(1, tp.BWD_BLOCK // G)
        per = np.add.reduceat(nseg, wg[:-1])
        assert most == max(1, per.max())
        lone = np.diff(wg) == 1
        assert np.all((per <= slots) | lone), 'only a texel on its own may exceed one pass'
        assert np.all(np.diff(wg) <= max(1, 32768 // C))
    wg, most = tp.pack_workgroups(np.zeros(10, dtype=np.int64), 32)
    assert wg[0] == 0 and wg[-1] == 10 and most == 1


def test_python_surface_raises_as_specified():
    xyz = torch.randn(20, 3)
    face = torch.zeros(20, dtype=torch.bool)
    with pytest.raises(RuntimeError, match='no CPU path'):
        exa.TriplaneFeatures(xyz, face)
    with pytest.raises(ValueError, match='constants'):
        exa.TriplaneFeatures(xyz.clone().requires_grad_(True), face)
    with pytest.raises(ValueError, match='float32'):
        exa.TriplaneFeatures(xyz.double(), face)
    with pytest.raises(ValueError, match='bool'):
        exa.TriplaneFeatures(xyz, face.to(torch.uint8))
    with pytest.raises(ValueError, match=r'\[N, 3\]'):
        exa.TriplaneFeatures(torch.randn(20, 2), face)
    with pytest.raises(ValueError, match='triplane_shape'):
        exa.TriplaneFeatures(xyz, face, triplane_shape=(0, 4, 4))
    assert 'TriplaneFeatures' in exa.__all__
