"""CPU tests of the blend-shape offsets' host side: the exports, the workspace-size query, invalid arguments failing with
their negative status and an ``exa_mesh: `` message before any GPU work, the module's plan against the oracle's, and the
Python surface refusing what it does not support.  The ABI itself (include/exa_mesh.h against its binding) is checked
by tests/test_abi.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import _lib, build
from exavatar_release_amd.blend_shapes import BlendShapes, BlendTable, blend_offsets, make_table
from tests import blend_oracle as bo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_blend.npz')
BAD = ctypes.c_void_p(0x1000)      # never dereferenced: every call below fails validation first
INVALID, NULLPTR = -1, -2


def _failed(lib, rc, status, word=b''):
    msg = lib.exa_mesh_last_error()
    return rc == status and msg.startswith(b'exa_mesh: ') and word in msg


def test_exports_and_build_list():
    for name in ('BlendShapes', 'BlendTable', 'blend_offsets'):
        assert name in exa.__all__ and getattr(exa, name) is getattr(exa.blend_shapes, name)
    assert build.SOURCES['blend_shapes.hip'] == ['-ffp-contract=off']
    for name in ('exa_mesh_blend_forward', 'exa_mesh_blend_workspace_size', 'exa_mesh_blend_backward'):
        assert name in _lib.MESH.signatures
    assert _lib.MESH.version == 100 and _lib.load().exa_mesh_version() == 100
    assert len(_lib.ABIS) == 6


def test_workspace_size_runs_on_the_host():
    lib = _lib.load()
    assert _lib.blend_workspace_size(50, 0) == 0
    assert _lib.blend_workspace_size(1, 1) == 256
    assert _lib.blend_workspace_size(50, 1024) == 256                       # one chunk: 50 floats
    assert _lib.blend_workspace_size(486, 1025) == (2 * 486 * 4 + 255) // 256 * 256
    assert _lib.blend_workspace_size(486, 200736) == (197 * 486 * 4 + 255) // 256 * 256
    out = ctypes.c_uint64()
    assert _failed(lib, lib.exa_mesh_blend_workspace_size(0, 10, ctypes.byref(out)), INVALID, b'K (blend')
    assert _failed(lib, lib.exa_mesh_blend_workspace_size(513, 10, ctypes.byref(out)), INVALID, b'K (blend')
    assert _failed(lib, lib.exa_mesh_blend_workspace_size(5, -1, ctypes.byref(out)), INVALID, b'negative size')
    assert _failed(lib, lib.exa_mesh_blend_workspace_size(5, 10, None), NULLPTR, b'NULL')
    with pytest.raises(RuntimeError, match='exa_mesh: K'):
        _lib.blend_workspace_size(0, 10)


def test_forward_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()

    def fwd(K=50, N=10, ld=12, M=30, coef=BAD, table=BAD, cols=BAD, inv=BAD, base=BAD, out=BAD, masked=BAD):
        return lib.exa_mesh_blend_forward(K, N, ld, M, coef, table, cols, inv, base, out, masked, None)

    assert _failed(lib, fwd(N=-1), INVALID, b'negative size') and _failed(lib, fwd(M=-1), INVALID, b'negative size')
    assert _failed(lib, fwd(K=0), INVALID, b'K (blend') and _failed(lib, fwd(K=513), INVALID, b'K (blend')
    assert _failed(lib, fwd(M=(1 << 30) + 1), INVALID, b'exceeds 2^30')
    assert _failed(lib, fwd(N=31, ld=32), INVALID, b'exceeds M')
    assert _failed(lib, fwd(ld=8), INVALID, b'ld must be') and _failed(lib, fwd(ld=13), INVALID, b'ld must be')
    for k in ('coef', 'table', 'cols', 'inv', 'out'):
        assert _failed(lib, fwd(**{k: None}), NULLPTR, b'NULL'), k
    assert _failed(lib, fwd(table=ctypes.c_void_p(0x1004)), INVALID, b'16-byte aligned')
    assert fwd(N=0, ld=0, M=0, coef=None, table=None, cols=None, inv=None, out=None) == 0        # nothing to do
    assert lib.exa_mesh_last_error().startswith(b'exa_mesh: ')
    with pytest.raises(RuntimeError, match='exa_mesh: ld must be'):
        _lib.MESH.check(fwd(ld=13))


def test_backward_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()
    need = _lib.blend_workspace_size(50, 2000)

    def bwd(K=50, N=2000, ld=2000, M=6000, table=BAD, cols=BAD, inv=BAD, g_out=BAD, g_masked=BAD, ws=BAD, nbytes=need,
            dcoef=BAD, dbase=BAD):
        return lib.exa_mesh_blend_backward(K, N, ld, M, table, cols, inv, g_out, g_masked, ws, nbytes, dcoef, dbase, None)

    assert _failed(lib, bwd(N=-2), INVALID, b'negative size') and _failed(lib, bwd(M=-2), INVALID, b'negative size')
    assert _failed(lib, bwd(K=0), INVALID, b'K (blend') and _failed(lib, bwd(K=513), INVALID, b'K (blend')
    assert _failed(lib, bwd(ld=1999), INVALID, b'ld must be') and _failed(lib, bwd(ld=2002), INVALID, b'ld must be')
    assert _failed(lib, bwd(N=6001, ld=6004), INVALID, b'exceeds M')
    for k in ('table', 'cols', 'inv', 'g_out', 'ws'):
        assert _failed(lib, bwd(**{k: None}), NULLPTR, b'NULL'), k
    assert _failed(lib, bwd(nbytes=need - 1), INVALID, b'workspace')
    assert _failed(lib, bwd(N=3000, ld=3000), INVALID, b'workspace')         # more chunks need a bigger workspace
    assert _failed(lib, bwd(table=ctypes.c_void_p(0x1008)), INVALID, b'16-byte aligned')
    assert bwd(dcoef=None, dbase=None) == 0                                  # no gradient wanted: nothing to do


def _model(V=40, Kp=18, Ke=5, seed=1):
    rng = np.random.RandomState(seed)
    pose_dirs = rng.standard_normal((Kp, 3 * V)).astype(np.float32)
    expr_dirs = rng.standard_normal((V, 3, Ke)).astype(np.float32)
    expr_dirs[rng.rand(V) < 0.6] = 0
    mask = rng.rand(V) < 0.4
    return pose_dirs, expr_dirs, mask


def test_module_plan_equals_the_oracle_plan_and_state_dict_is_empty():
    pose_dirs, expr_dirs, mask = _model()
    m = BlendShapes(torch.from_numpy(pose_dirs), torch.from_numpy(expr_dirs), torch.from_numpy(mask))
    assert not m.state_dict() and not list(m.parameters())
    assert sorted(n for n, _ in m.named_buffers()) == ['expr_cols', 'expr_inv', 'expr_table', 'pose_cols', 'pose_inv',
                                                       'pose_table']
    want = bo.plan(pose_dirs, bo.pose_keep(mask))
    for got, w in zip(m.pose_plan, want):
        assert got.numpy().dtype == w.dtype and np.array_equal(got.numpy(), w)
    want = bo.plan(*bo.expr_full(expr_dirs))
    for got, w in zip(m.expr_plan, want):
        assert got.numpy().dtype == w.dtype and np.array_equal(got.numpy(), w)
    assert isinstance(m.pose_plan, BlendTable) and m.vertex_num == 40
    # .to() moves the buffers (here: nowhere) and keeps them out of the state
    assert not m.to('cpu').state_dict()
    # an all-false and an all-true mask both work
    for mk in (np.zeros(40, bool), np.ones(40, bool)):
        m2 = BlendShapes(torch.from_numpy(pose_dirs), torch.from_numpy(expr_dirs), torch.from_numpy(mk))
        assert m2.pose_cols.numel() == 3 * int(mk.sum()) and m2.pose_table.shape == (18, 3 * int(mk.sum()))
    z = np.load(GOLDEN)
    m3 = BlendShapes(torch.from_numpy(z['smplx_pose_dirs']), torch.from_numpy(z['expr_expr_dirs'][:96]),
                     torch.from_numpy(z['smplx_pose_mask']))
    assert m3.pose_table.shape[0] == 486 and m3.pose_cols.numel() == 3 * int(z['smplx_pose_mask'].sum())


def test_constructor_raises_as_specified():
    pose_dirs, expr_dirs, mask = [torch.from_numpy(a) for a in _model()]
    with pytest.raises(TypeError, match='pose_dirs must be a tensor'):
        BlendShapes(pose_dirs.numpy(), expr_dirs, mask)
    with pytest.raises(ValueError, match='pose_dirs is data in the reference and gets no gradient'):
        BlendShapes(pose_dirs.clone().requires_grad_(True), expr_dirs, mask)
    with pytest.raises(ValueError, match='expr_dirs is data in the reference and gets no gradient'):
        BlendShapes(pose_dirs, expr_dirs.clone().requires_grad_(True), mask)
    with pytest.raises(ValueError, match='pose_mask must be a bool tensor'):
        BlendShapes(pose_dirs, expr_dirs, mask.float())
    with pytest.raises(ValueError, match='pose_dirs must be float32'):
        BlendShapes(pose_dirs.double(), expr_dirs, mask)
    with pytest.raises(ValueError, match=r'pose_dirs must be \[Kp, 3 V\]'):
        BlendShapes(pose_dirs[:, :-3], expr_dirs, mask)
    with pytest.raises(ValueError, match=r'pose_dirs must be \[Kp, 3 V\]'):
        BlendShapes(torch.zeros(513, 120), expr_dirs, mask)
    with pytest.raises(ValueError, match=r'expr_dirs must be \[V, 3, Ke\]'):
        BlendShapes(pose_dirs, expr_dirs[:-1], mask)
    with pytest.raises(ValueError, match=r'expr_dirs must be \[V, 3, Ke\]'):
        BlendShapes(pose_dirs, expr_dirs.reshape(40, 15), mask)


def test_python_surface_raises_as_specified():
    pose_dirs, expr_dirs, mask = [torch.from_numpy(a) for a in _model()]
    m = BlendShapes(pose_dirs, expr_dirs, mask)
    feat, moo, expr = torch.randn(1, 18), torch.randn(40, 3), torch.randn(5)
    with pytest.raises(RuntimeError, match='no CPU path'):
        m.pose_offsets(feat, moo)
    with pytest.raises(RuntimeError, match='no CPU path'):
        m.expr_offsets(expr)
    with pytest.raises(RuntimeError, match='no CPU path'):
        blend_offsets(expr, m.expr_plan)
    with pytest.raises(TypeError, match='tensors'):
        m.pose_offsets(feat.numpy(), moo)
    with pytest.raises(TypeError, match='expr must be a tensor'):
        m.expr_offsets(expr.numpy())
    with pytest.raises(ValueError, match=r'mean_offset_offset must be \[V, 3\]'):
        m.pose_offsets(feat, moo[:-1])
    with pytest.raises(TypeError, match='BlendTable'):
        blend_offsets(expr, tuple(m.expr_plan))
    t = m.expr_plan
    with pytest.raises(ValueError, match='table is data in the reference and gets no gradient'):
        blend_offsets(expr, BlendTable(t.table.clone().requires_grad_(True), t.cols, t.inv))
    with pytest.raises(ValueError, match='cols, inv int32'):
        blend_offsets(expr, BlendTable(t.table, t.cols.long(), t.inv))
    with pytest.raises(ValueError, match=r'table must be \[K, N_pad\]'):
        blend_offsets(expr, BlendTable(t.table[:, :-1], t.cols, t.inv))
    with pytest.raises(ValueError, match=r'table must be \[K, N_pad\]'):
        blend_offsets(torch.randn(513), BlendTable(torch.zeros(513, 4), torch.zeros(4, dtype=torch.int32),
                                                   torch.zeros(9, dtype=torch.int32)))
    with pytest.raises(TypeError, match='dirs and keep must be tensors'):
        make_table(pose_dirs.numpy(), mask)
    with pytest.raises(ValueError, match='keep must be a bool tensor'):
        make_table(pose_dirs, mask)
    with pytest.raises(ValueError, match=r'dirs must be \[K, M\]'):
        make_table(pose_dirs[0], mask)
