"""CPU tests of the mesh Laplacian's host side: the neighbour table is the reference's element for element, invalid
arguments fail with their negative status and an ``exa_mesh: `` message before any GPU work, the transposed table of a
hand-written example is the hand-written answer, and the Python surface refuses what it does not support.  The ABI
itself (include/exa_mesh.h against its binding) is checked by tests/test_abi.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import _lib
from exavatar_release_amd.mesh_reg import LaplacianReg, mesh_laplacian_loss, neighbor_table
from tests import lap_oracle as lo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_lap.npz')
BAD = ctypes.c_void_p(0x1000)      # never dereferenced: every call below fails validation first
INVALID, NULLPTR = -1, -2


def _failed(lib, rc, status, word=b''):
    msg = lib.exa_mesh_last_error()
    return rc == status and msg.startswith(b'exa_mesh: ') and word in msg


def test_table_equals_the_reference_golden_element_for_element():
    z = np.load(GOLDEN)
    V = z['neighbor_idxs'].shape[0]
    reg = LaplacianReg(V, z['face'])
    assert reg.neighbor_idxs.dtype == torch.int64 and reg.neighbor_weights.dtype == torch.float32
    assert np.array_equal(reg.neighbor_idxs.cpu().numpy(), z['neighbor_idxs'])
    assert np.array_equal(reg.neighbor_weights.cpu().numpy(), z['neighbor_weights'])
    hub = int(z['hub'])
    assert reg.neighbor_idxs[hub].tolist() == z['neighbor_idxs'][hub].tolist() != sorted(z['rim'].tolist())[:10]
    # a tensor of faces and another slot count go the same way
    idxs, weights = neighbor_table(V, torch.from_numpy(z['face']), 10)
    assert np.array_equal(idxs, z['neighbor_idxs']) and np.array_equal(weights, z['neighbor_weights'])
    idx4, w4 = neighbor_table(V, z['face'], 4)
    assert np.array_equal(idx4[hub], z['neighbor_idxs'][hub, :4]) and (w4[hub] == np.float32(-0.25)).all()


def test_an_unused_vertex_and_a_bad_face_are_value_errors():
    face = lo.grid_faces(3, 3)
    with pytest.raises(ValueError, match='vertex 9 belongs to no face'):
        LaplacianReg(10, face)
    with pytest.raises(ValueError, match=r'outside \[0, 8\)'):
        LaplacianReg(8, face)
    with pytest.raises(ValueError, match='neighbor_max_num'):
        LaplacianReg(9, face, 17)


def test_neighbor_transpose_of_a_hand_written_table():
    lib = _lib.load()
    # slots:        0  1   2  3   4  5   6  7
    idx = np.array([[1, 2], [0, 0], [3, 2], [1, 3]], dtype=np.int32)
    off = np.zeros(5, dtype=np.int32)
    ent = np.zeros(8, dtype=np.int32)
    assert lib.exa_mesh_neighbor_transpose(4, 2, idx.ctypes.data, off.ctypes.data, ent.ctypes.data) == 0
    assert off.tolist() == [0, 2, 4, 6, 8]
    assert ent.tolist() == [2, 3, 0, 6, 1, 5, 4, 7]
    o2, e2 = lo.transpose(idx)
    assert o2.tolist() == off.tolist() and e2.tolist() == ent.tolist()
    # the golden's table, against the oracle's independent construction
    z = np.load(GOLDEN)
    g = np.ascontiguousarray(z['neighbor_idxs'], dtype=np.int32)
    V, K = g.shape
    off, ent = np.zeros(V + 1, dtype=np.int32), np.zeros(V * K, dtype=np.int32)
    assert lib.exa_mesh_neighbor_transpose(V, K, g.ctypes.data, off.ctypes.data, ent.ctypes.data) == 0
    o2, e2 = lo.transpose(g)
    assert np.array_equal(off, o2) and np.array_equal(ent, e2)
    # an index >= V (and a negative one) is refused by name
    idx[2, 0] = 4
    rc = lib.exa_mesh_neighbor_transpose(4, 2, idx.ctypes.data, off.ctypes.data, ent.ctypes.data)
    assert _failed(lib, rc, INVALID, b'index 4 of vertex 2, slot 0')
    idx[2, 0] = -1
    rc = lib.exa_mesh_neighbor_transpose(4, 2, idx.ctypes.data, off.ctypes.data, ent.ctypes.data)
    assert _failed(lib, rc, INVALID, b'index -1 of vertex 2')


def test_neighbor_transpose_rejects_bad_arguments():
    lib = _lib.load()
    assert _failed(lib, lib.exa_mesh_neighbor_transpose(-1, 10, BAD, BAD, BAD), INVALID, b'negative size')
    assert _failed(lib, lib.exa_mesh_neighbor_transpose(4, 0, BAD, BAD, BAD), INVALID, b'K (neighbours')
    assert _failed(lib, lib.exa_mesh_neighbor_transpose(4, 17, BAD, BAD, BAD), INVALID, b'K (neighbours')
    assert _failed(lib, lib.exa_mesh_neighbor_transpose(4, 10, None, BAD, BAD), NULLPTR, b'NULL')
    assert _failed(lib, lib.exa_mesh_neighbor_transpose(4, 10, BAD, None, BAD), NULLPTR, b'NULL')
    assert _failed(lib, lib.exa_mesh_neighbor_transpose(4, 10, BAD, BAD, None), NULLPTR, b'NULL')
    off = np.full(1, 7, dtype=np.int32)
    assert lib.exa_mesh_neighbor_transpose(0, 10, None, off.ctypes.data, None) == 0 and off[0] == 0


def test_forward_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()

    def fwd(B=2, Bt=2, V=100, C=3, K=10, out=BAD, target=BAD, idx=BAD, w=BAD, weight=BAD, loss=BAD, d=BAD):
        return lib.exa_mesh_laplacian_forward(B, Bt, V, C, K, out, target, idx, w, weight, loss, d, None)

    assert _failed(lib, fwd(B=-1), INVALID, b'negative size')
    assert _failed(lib, fwd(V=-1), INVALID, b'negative size')
    assert _failed(lib, fwd(C=0), INVALID, b'C (channels)') and _failed(lib, fwd(C=9), INVALID, b'C (channels)')
    assert _failed(lib, fwd(K=0), INVALID, b'K (neighbours') and _failed(lib, fwd(K=17), INVALID, b'K (neighbours')
    assert _failed(lib, fwd(Bt=3), INVALID, b'Bt') and _failed(lib, fwd(Bt=0), INVALID, b'Bt')
    assert _failed(lib, fwd(B=3, Bt=2), INVALID, b'Bt')
    for k in ('out', 'idx', 'w', 'loss', 'd'):
        assert _failed(lib, fwd(**{k: None}), NULLPTR, b'NULL'), k
    assert fwd(V=0, out=None, idx=None, w=None, loss=None, d=None) == 0       # nothing to do
    assert fwd(B=0, Bt=1, out=None, loss=None, d=None) == 0


def test_backward_and_workspace_size_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert _lib.laplacian_workspace_size(0, 100, 3) == 0 and _lib.laplacian_workspace_size(2, 0, 3) == 0
    assert _lib.laplacian_workspace_size(1, 1, 1) == 256
    assert _lib.laplacian_workspace_size(2, 167281, 3) == (2 * 167281 * 3 * 4 + 255) // 256 * 256
    out = ctypes.c_uint64()
    assert _failed(lib, lib.exa_mesh_laplacian_workspace_size(-1, 10, 3, ctypes.byref(out)), INVALID, b'negative size')
    assert _failed(lib, lib.exa_mesh_laplacian_workspace_size(1, -10, 3, ctypes.byref(out)), INVALID, b'negative size')
    assert _failed(lib, lib.exa_mesh_laplacian_workspace_size(1, 10, 9, ctypes.byref(out)), INVALID, b'C (channels)')
    assert _failed(lib, lib.exa_mesh_laplacian_workspace_size(1, 10, 0, ctypes.byref(out)), INVALID, b'C (channels)')
    assert _failed(lib, lib.exa_mesh_laplacian_workspace_size(1, 10, 3, None), NULLPTR, b'NULL')
    need = _lib.laplacian_workspace_size(2, 100, 3)

    def bwd(B=2, V=100, C=3, K=10, d=BAD, gl=BAD, w=BAD, weight=BAD, off=BAD, ent=BAD, ws=BAD, nbytes=need, gout=BAD):
        return lib.exa_mesh_laplacian_backward(B, V, C, K, d, gl, w, weight, off, ent, ws, nbytes, gout, None)

    assert _failed(lib, bwd(B=-2), INVALID, b'negative size') and _failed(lib, bwd(V=-2), INVALID, b'negative size')
    assert _failed(lib, bwd(C=0), INVALID, b'C (channels)') and _failed(lib, bwd(C=9), INVALID, b'C (channels)')
    assert _failed(lib, bwd(K=0), INVALID, b'K (neighbours') and _failed(lib, bwd(K=17), INVALID, b'K (neighbours')
    for k in ('d', 'gl', 'w', 'off', 'ent', 'ws', 'gout'):
        assert _failed(lib, bwd(**{k: None}), NULLPTR, b'NULL'), k
    assert _failed(lib, bwd(nbytes=need - 1), INVALID, b'workspace')
    assert _failed(lib, bwd(B=3), INVALID, b'workspace')                     # a bigger batch needs a bigger workspace
    assert bwd(V=0, d=None, gl=None, w=None, off=None, ent=None, ws=None, nbytes=0, gout=None) == 0


def test_python_surface_raises_as_specified():
    assert 'LaplacianReg' in exa.__all__ and exa.LaplacianReg is LaplacianReg
    assert 'mesh_laplacian_loss' in exa.__all__ and exa.mesh_laplacian_loss is mesh_laplacian_loss
    face = lo.grid_faces(4, 5)
    V = 20
    reg = LaplacianReg(V, face)
    assert tuple(reg.neighbor_idxs.shape) == (V, 10) and not list(reg.parameters()) and not reg.state_dict()
    x = torch.randn(1, V, 3)
    with pytest.raises(RuntimeError, match='no CPU path'):
        reg(x, None)
    with pytest.raises(RuntimeError, match='no CPU path'):
        reg(x, x.clone())
    with pytest.raises(RuntimeError, match='no CPU path'):
        mesh_laplacian_loss(x, None, reg.neighbor_idxs.cpu(), reg.neighbor_weights.cpu())
    with pytest.raises(TypeError, match='tensor'):
        reg(x.numpy(), None)
    with pytest.raises(ValueError, match='K <= 16'):
        mesh_laplacian_loss(x, None, torch.zeros(V, 17, dtype=torch.int64), torch.zeros(V, 17))
    with pytest.raises(ValueError, match='K <= 16'):
        mesh_laplacian_loss(x, None, torch.zeros(V, 10), torch.zeros(V, 10))
