"""CPU tests of the knn_points host side: invalid arguments fail with a negative status before any GPU work, and the
Python surface refuses CPU tensors and the unsupported options.  The ABI itself (include/exa_knn.h against its binding)
is checked by tests/test_abi.py."""
import ctypes

import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import _lib

BAD = ctypes.c_void_p(0x1000)      # never dereferenced: every call below fails validation first


def _size(N, P1, P2, K):
    out = ctypes.c_uint64(123)
    rc = _lib.load().exa_knn_workspace_size(N, P1, P2, K, ctypes.byref(out))
    return rc, out.value


def _forward(N=1, P1=10, P2=10, K=1, p1=BAD, p2=BAD, flags=0, ws=BAD, nbytes=1 << 40, dists=BAD, idx=BAD):
    return _lib.load().exa_knn_forward(N, P1, P2, K, p1, p2, flags, ws, nbytes, dists, idx, None, None)


def test_workspace_size_is_zero_for_empty_inputs_and_grows_with_the_points():
    for shape in ((0, 10, 10), (3, 0, 10), (3, 10, 0), (0, 0, 0)):
        assert _size(*shape, 1) == (0, 0)
    rc, a = _size(1, 1000, 1000, 1)
    rc2, b = _size(1, 100000, 100000, 1)
    assert rc == 0 and rc2 == 0 and 0 < a < b
    assert _size(2, 1000, 1000, 4)[1] >= 2 * _size(1, 1000, 1000, 4)[1] - 4096


def test_workspace_size_rejects_bad_arguments():
    assert _size(1, 10, 10, 0)[0] < 0
    assert _size(1, 10, 10, 33)[0] < 0
    assert _size(-1, 10, 10, 1)[0] < 0
    assert _size(1, -10, 10, 1)[0] < 0
    assert _size(1, 10, -10, 1)[0] < 0
    assert _lib.load().exa_knn_workspace_size(1, 10, 10, 1, None) < 0


def test_forward_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert _forward(K=0) < 0
    assert _forward(K=33) < 0
    assert _forward(N=-1) < 0
    assert _forward(P1=-1) < 0
    assert _forward(P2=-5) < 0
    assert _forward(K=11) < 0                       # K > P2
    assert _forward(flags=2) < 0
    assert _forward(p1=None) < 0
    assert _forward(p2=None) < 0
    assert _forward(dists=None) < 0
    assert _forward(idx=None) < 0
    assert _forward(ws=None) < 0
    need = _size(1, 10, 10, 1)[1]
    assert _forward(nbytes=need - 1) < 0
    assert b'workspace' in lib.exa_knn_last_error()
    assert _forward(K=0) == -1 and b'K must be' in lib.exa_knn_last_error()
    # nothing to search: ok without touching anything
    assert _forward(N=0, p1=None, p2=None, ws=None, dists=None, idx=None) == 0
    assert _forward(P1=0, p1=None, p2=None, ws=None, dists=None, idx=None) == 0


def test_backward_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()

    def bwd(N=1, P1=10, P2=10, K=1, p1=BAD, p2=BAD, idx=BAD, si=BAD, order=BAD, g1=BAD, g2=BAD):
        return lib.exa_knn_backward(N, P1, P2, K, p1, p2, idx, None, None, si, order, g1, g2, None)

    assert bwd(K=0) < 0
    assert bwd(K=33) < 0
    assert bwd(N=-1) < 0
    assert bwd(P2=0) < 0
    for k in ('p1', 'p2', 'idx', 'si', 'order', 'g1', 'g2'):
        assert bwd(**{k: None}) < 0, k


def test_cpu_tensors_have_no_cpu_path():
    a = torch.randn(1, 20, 3)
    with pytest.raises(RuntimeError, match='no CPU path'):
        exa.knn_points(a, a, K=2)


def test_unsupported_options_raise():
    a = torch.randn(1, 20, 3)
    with pytest.raises(NotImplementedError, match='padded batches'):
        exa.knn_points(a, a, lengths1=torch.tensor([20]))
    with pytest.raises(NotImplementedError, match='padded batches'):
        exa.knn_points(a, a, lengths2=torch.tensor([20]))
    with pytest.raises(NotImplementedError, match='squared L2'):
        exa.knn_points(a, a, norm=1)
    with pytest.raises(ValueError):
        exa.knn_points(a, a, K=33)
    with pytest.raises(ValueError):
        exa.knn_points(a, a, K=0)
