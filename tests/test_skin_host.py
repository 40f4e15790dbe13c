"""CPU tests of the skinning's host side: invalid arguments fail with their negative status before any GPU work, and the
Python surface refuses what it does not support.  The ABI itself (include/exa_skin.h against its binding) is checked by
tests/test_abi.py."""
import ctypes

import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd.skinning import skin_points  # noqa: F401  (the feature under test)
from exavatar_release_amd import _lib

BAD = ctypes.c_void_p(0x1000)      # never dereferenced: every call below fails validation first
INVALID, NULLPTR = -1, -2


def test_workspace_size():
    assert _lib.skin_workspace_size(0, 55) == 0
    assert _lib.skin_workspace_size(1, 1) == 15 * 4
    assert _lib.skin_workspace_size(256, 64) == 771 * 4
    assert _lib.skin_workspace_size(167000, 55) == 653 * 663 * 4
    lib = _lib.load()
    out = ctypes.c_uint64()
    assert lib.exa_skin_workspace_size(-1, 55, ctypes.byref(out)) == INVALID
    assert lib.exa_skin_workspace_size(10, 65, ctypes.byref(out)) == INVALID
    assert lib.exa_skin_workspace_size(10, 0, ctypes.byref(out)) == INVALID
    assert lib.exa_skin_workspace_size(10, 55, None) == NULLPTR


def _arr(*ptrs):
    return (ctypes.c_void_p * len(ptrs))(*[p.value if isinstance(p, ctypes.c_void_p) else p for p in ptrs])


def test_forward_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()

    def fwd(V=10, S=2, J=55, Vw=10, pts=True, W=BAD, idx=BAD, T=BAD, trans=BAD, Rinv=BAD, t=BAD, out=True):
        p = _arr(*[BAD] * S) if pts is True else pts
        o = _arr(*[BAD] * S) if out is True else out
        return lib.exa_skin_forward(V, S, J, Vw, p, W, idx, T, trans, Rinv, t, o, None)

    assert fwd(V=-1) == INVALID
    assert fwd(V=(1 << 28) + 1) == INVALID
    assert fwd(S=0, pts=_arr(BAD), out=_arr(BAD)) == INVALID and b'S (point sets)' in lib.exa_skin_last_error()
    assert fwd(S=5, pts=_arr(*[BAD] * 5), out=_arr(*[BAD] * 5)) == INVALID
    assert fwd(J=65) == INVALID and b'J (joints)' in lib.exa_skin_last_error()
    assert fwd(J=0) == INVALID
    assert fwd(Vw=-1) == INVALID
    assert fwd(idx=None, Vw=9) == INVALID and b'V rows' in lib.exa_skin_last_error()
    assert fwd(Rinv=None) == INVALID and fwd(t=None) == INVALID
    for k in ('W', 'T', 'trans'):
        assert fwd(**{k: None}) == NULLPTR, k
    assert fwd(pts=None) == NULLPTR and fwd(out=None) == NULLPTR
    assert fwd(pts=_arr(BAD, None)) == NULLPTR and fwd(out=_arr(None, BAD)) == NULLPTR
    assert b'NULL' in lib.exa_skin_last_error()
    assert fwd(V=0, Vw=0, pts=None, W=None, T=None, trans=None, out=None) == 0      # nothing to do


def test_backward_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()
    need = _lib.skin_workspace_size(300, 55)

    def bwd(V=300, S=2, J=55, Vw=300, pts=True, W=BAD, idx=BAD, T=BAD, Rinv=BAD, gout=True, gpts=True, gT=BAD,
            gtr=BAD, ws=BAD, nbytes=need):
        p = _arr(*[BAD] * S) if pts is True else pts
        go = _arr(*[BAD] * S) if gout is True else gout
        gp = _arr(*[BAD] * S) if gpts is True else gpts
        return lib.exa_skin_backward(V, S, J, Vw, p, W, idx, T, Rinv, go, gp, gT, gtr, ws, nbytes, None)

    assert bwd(V=-3) == INVALID
    assert bwd(S=0) == INVALID and bwd(S=5) == INVALID
    assert bwd(J=65) == INVALID
    assert bwd(idx=None, Vw=299) == INVALID
    assert bwd(nbytes=need - 1) == INVALID and b'workspace' in lib.exa_skin_last_error()
    assert bwd(ws=None) == NULLPTR
    for k in ('W', 'T'):
        assert bwd(**{k: None}) == NULLPTR, k
    assert bwd(pts=None) == NULLPTR and bwd(gout=None) == NULLPTR and bwd(gout=_arr(BAD, None)) == NULLPTR
    # J = 64 needs a bigger workspace than J = 55
    assert bwd(J=64, nbytes=need) == INVALID


def test_python_surface_raises_as_specified():
    assert 'skin_points' in exa.__all__ and exa.skin_points is not None
    V, J = 20, 55
    x = torch.randn(V, 3)
    T = torch.eye(4).repeat(J, 1, 1)
    W = torch.rand(V, J)
    R, t = torch.eye(3), torch.zeros(3)
    with pytest.raises(RuntimeError, match='no CPU path'):
        exa.skin_points(x, T, W)
    with pytest.raises(ValueError, match='buffer'):
        exa.skin_points(x, T, W.clone().requires_grad_(True))
    with pytest.raises(ValueError, match='camera data'):
        exa.skin_points(x, T, W, R=R.clone().requires_grad_(True), t=t)
    with pytest.raises(ValueError, match='camera data'):
        exa.skin_points(x, T, W, R=R, t=t.clone().requires_grad_(True))
    with pytest.raises(ValueError, match='together'):
        exa.skin_points(x, T, W, R=R)
    with pytest.raises(ValueError, match='float32'):
        exa.skin_points(x.double(), T, W)
    with pytest.raises(ValueError, match='float32'):
        exa.skin_points(x, T.double(), W)
    with pytest.raises(ValueError, match=r'\[J, 4, 4\]'):
        exa.skin_points(x, torch.eye(4).repeat(65, 1, 1), torch.rand(V, 65))
    with pytest.raises(ValueError, match=r'\[J, 4, 4\]'):
        exa.skin_points(x, T[:, :3], W)
    with pytest.raises(ValueError, match=r'\[Vw, J\]'):
        exa.skin_points(x, T, W[:, :54])
    with pytest.raises(ValueError, match=r'\[V, 3\]'):
        exa.skin_points((x, x[:10]), T, W)
    with pytest.raises(ValueError, match='point sets'):
        exa.skin_points([x] * 5, T, W)
    with pytest.raises(ValueError, match='int64'):
        exa.skin_points(x, T, W, idx=torch.zeros(V, dtype=torch.int32))
    with pytest.raises(ValueError, match='V = 20 rows'):
        exa.skin_points(x, T, W[:10])
    with pytest.raises(ValueError, match='trans'):
        exa.skin_points(x, T, W, trans=torch.zeros(2))
