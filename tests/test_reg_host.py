"""Host side of the arm and hand regularisers (exavatar_release_amd/vertex_regs.py, csrc/vertex_regs.hip) without a GPU:
every argument check raises ValueError naming the argument (dtype and shape before the device, so that they can be
reached here), the C calls refuse bad sizes before they touch the device, the hands' index and rank tables, and the
memoisation of ArmRGBReg's plan."""
import ctypes

import numpy as np
import pytest
import torch

from exavatar_release_amd import _lib
from exavatar_release_amd import vertex_regs as vr
from exavatar_release_amd.vertex_regs import (ArmRGBReg, HandMeanReg, HandRGBReg, arm_neighbors, arm_rgb_loss, get_arm,
                                              index_tables)
from tests import reg_oracle as ro

V = 12


def _mesh():
    return torch.zeros(V, 3)


def _mask(*on):
    m = torch.zeros(V, dtype=torch.bool)
    m[list(on)] = True
    return m


def test_arm_neighbors_refuses_bad_arguments_by_name():
    up, lo = _mask(0, 1), _mask(2, 3)
    with pytest.raises(ValueError, match='mesh_neutral_pose must be float32'):
        arm_neighbors(_mesh().double(), up, lo)
    with pytest.raises(ValueError, match=r'mesh_neutral_pose must be \[V, 3\]'):
        arm_neighbors(torch.zeros(V, 4), up, lo)
    with pytest.raises(ValueError, match=r'mesh_neutral_pose must be \[V, 3\]'):
        arm_neighbors(torch.zeros(1, V, 3), up, lo)
    with pytest.raises(TypeError, match='mesh_neutral_pose must be a tensor'):
        arm_neighbors(np.zeros((V, 3), dtype=np.float32), up, lo)
    with pytest.raises(ValueError, match=r'is_upper_arm must be a bool \[V\]'):
        arm_neighbors(_mesh(), up.float(), lo)
    with pytest.raises(ValueError, match=r'is_lower_arm must be a bool \[V\]'):
        arm_neighbors(_mesh(), up, lo[:-1])
    with pytest.raises(ValueError, match=r'is_lower_arm must be a bool \[V\]'):
        arm_neighbors(_mesh(), up, lo[None])
    for bad in (0, 65, -1, 2.5, True):
        with pytest.raises(ValueError, match='top_k must be an integer 1 .. 64'):
            arm_neighbors(_mesh(), up, lo, top_k=bad)
    for bad in (0.0, -0.01, float('inf'), float('nan'), 1e-50, 1e39):     # the last two: 0 and inf as a float32
        with pytest.raises(ValueError, match='dist_x_thr must be finite and > 0'):
            arm_neighbors(_mesh(), up, lo, dist_x_thr=bad)
    with pytest.raises(ValueError, match='row_capacity must be 0 .. V'):
        arm_neighbors(_mesh(), up, lo, row_capacity=V + 1)
    # everything else in order: the device is checked last
    with pytest.raises(ValueError, match='mesh_neutral_pose must be on a ROCm device'):
        arm_neighbors(_mesh(), up, lo)
    with pytest.raises(ValueError, match='mesh_neutral_pose must be on a ROCm device'):
        ArmRGBReg()(_mesh().requires_grad_(True), up, lo, torch.zeros(1, V, 3))     # the mesh may require a gradient: it gets none


def test_arm_rgb_loss_refuses_bad_arguments_by_name():
    plan = vr.ArmPlan.__new__(vr.ArmPlan)
    plan.V, plan.device = V, torch.device('cpu')
    with pytest.raises(ValueError, match='plan must be an ArmPlan'):
        arm_rgb_loss(None, torch.zeros(1, V, 3))
    with pytest.raises(ValueError, match='rgb must be float32'):
        arm_rgb_loss(plan, torch.zeros(1, V, 3, dtype=torch.float16))
    for shape in ((1, V, 4), (V, 3), (1, V + 1, 3)):
        with pytest.raises(ValueError, match=r'rgb must be \[B, V, 3\]'):
            arm_rgb_loss(plan, torch.zeros(shape))
    plan.device = torch.device('meta')
    with pytest.raises(ValueError, match='rgb is not on the device of plan'):
        arm_rgb_loss(plan, torch.zeros(1, V, 3))


def test_get_arm_refuses_bad_arguments_by_name():
    face = ro.grid_faces(3, 4)
    w = torch.rand(V, 5)
    with pytest.raises(ValueError, match=r'mesh_neutral_pose must be \[V, 3\]'):
        get_arm(torch.zeros(V, 2), w, face, [1, 2])
    with pytest.raises(ValueError, match=r'skinning_weight must be \[V, J\]'):
        get_arm(_mesh(), torch.rand(V + 1, 5), face, [1, 2])
    with pytest.raises(ValueError, match='skinning_weight must be float32'):
        get_arm(_mesh(), w.double(), face, [1, 2])
    with pytest.raises(ValueError, match='skinning_weight is a buffer'):
        get_arm(_mesh(), w.clone().requires_grad_(True), face, [1, 2])
    with pytest.raises(ValueError, match='arm_joint_idx must name joints'):
        get_arm(_mesh(), w, face, [1, 5])
    with pytest.raises(ValueError, match=r'normal must be \[V, 3\] or \[1, V, 3\]'):
        get_arm(_mesh(), w, face, [1, 2], normal=torch.zeros(2, V, 3))
    with pytest.raises(ValueError, match='normal is data'):
        get_arm(_mesh(), w, face, [1, 2], normal=torch.zeros(V, 3, requires_grad=True))
    with pytest.raises(ValueError, match='mesh_neutral_pose must be on a ROCm device'):
        get_arm(_mesh(), w, face, [1, 2], normal=torch.zeros(1, V, 3))


def test_hand_rgb_refuses_bad_arguments_by_name():
    reg = HandRGBReg()
    r, l = _mask(0, 1, 2), _mask(3, 4, 5)
    with pytest.raises(ValueError, match='rgb must be float32'):
        reg(torch.zeros(1, V, 3).double(), r, l)
    with pytest.raises(ValueError, match=r'rgb must be \[B, V, 3\]'):
        reg(torch.zeros(1, V, 4), r, l)
    with pytest.raises(ValueError, match=r'rgb must be \[B, V, 3\]'):
        reg(torch.zeros(V, 3), r, l)
    with pytest.raises(ValueError, match=r'is_rhand must be a bool \[V\]'):
        reg(torch.zeros(1, V, 3), r.long(), l)
    with pytest.raises(ValueError, match=r'is_lhand must be a bool \[V\]'):
        reg(torch.zeros(1, V, 3), r, l[:5])
    with pytest.raises(ValueError, match=r'select equally many vertices \(they select 3 and 2\)'):
        reg(torch.zeros(1, V, 3), r, _mask(3, 4))
    with pytest.raises(ValueError, match='rgb must be on a ROCm device'):
        reg(torch.zeros(1, V, 3), r, l)


def test_hand_mean_refuses_bad_arguments_by_name():
    reg = HandMeanReg(ro.grid_faces(3, 4))
    r, l = _mask(0, 1, 2), _mask(3, 4, 5)
    off = torch.zeros(2, V, 3)
    with pytest.raises(ValueError, match=r'mesh_neutral_pose must be \[V, 3\]'):
        reg(torch.zeros(1, V, 3), off, r, l)
    with pytest.raises(ValueError, match='offset must be float32'):
        reg(_mesh(), off.double(), r, l)
    with pytest.raises(ValueError, match=r'offset must be \[B, V, 3\]'):
        reg(_mesh(), torch.zeros(2, V, 2), r, l)
    with pytest.raises(ValueError, match=r'offset must be \[B, V, 3\]'):
        reg(_mesh(), torch.zeros(2, V - 1, 3), r, l)
    with pytest.raises(ValueError, match=r'is_rhand must be a bool \[V\]'):
        reg(_mesh(), off, None, l)
    with pytest.raises(ValueError, match=r'is_lhand must be a bool \[V\]'):
        reg(_mesh(), off, r, l.int())
    with pytest.raises(ValueError, match='normal must be float32'):
        reg(_mesh(), off, r, l, normal=torch.zeros(V, 3).double())
    with pytest.raises(ValueError, match=r'normal must be \[V, 3\] or \[1, V, 3\]'):
        reg(_mesh(), off, r, l, normal=torch.zeros(V, 4))
    with pytest.raises(ValueError, match='normal is data'):
        reg(_mesh(), off, r, l, normal=torch.zeros(V, 3, requires_grad=True))
    with pytest.raises(ValueError, match='offset must be on a ROCm device'):
        reg(_mesh(), off.requires_grad_(True), r, l, normal=torch.zeros(V, 3))


def test_the_c_calls_refuse_bad_sizes_before_they_touch_the_device():
    lib = _lib.load()
    last = lib.exa_mesh_last_error
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.exa_mesh_arm_plan(-1, 0, 50, 0.01, p, p, p, p, p, p, p, p, p, p, None) == -1 and b'negative size' in last()
    assert lib.exa_mesh_arm_plan(8, 9, 50, 0.01, p, p, p, p, p, p, p, p, p, p, None) == -1 and b'rows' in last()
    for k in (0, 65):
        assert lib.exa_mesh_arm_plan(8, 8, k, 0.01, p, p, p, p, p, p, p, p, p, p, None) == -1 and b'K_max must be 1 .. 64' in last()
    for thr in (0.0, -1.0, float('inf'), float('nan')):
        assert lib.exa_mesh_arm_plan(8, 8, 50, thr, p, p, p, p, p, p, p, p, p, p, None) == -1 and b'dist_x_thr' in last()
    assert lib.exa_mesh_arm_plan(8, 8, 50, 0.01, p, p, p, p, p, p, p, p, p, None, None) == -2 and b'header is NULL' in last()
    assert lib.exa_mesh_arm_plan(8, 8, 50, 0.01, None, p, p, p, p, p, p, p, p, p, None) == -2
    assert lib.exa_mesh_arm_plan(8, 8, 50, 0.01, p, p, p, p, p, p, None, p, p, p, None) == -2 and b'nbr' in last()
    assert lib.exa_mesh_arm_loss_forward(1, 8, 8, 65, p, p, p, p, p, p, None) == -1
    assert lib.exa_mesh_arm_loss_forward(1, 8, 8, 50, p, p, p, p, None, p, None) == -2 and b'loss / d is NULL' in last()
    assert lib.exa_mesh_arm_loss_forward(0, 8, 8, 50, None, None, None, None, None, None, None) == 0       # B == 0: a no-op
    assert lib.exa_mesh_arm_loss_backward(65536, 8, p, p, p, p, None) == -1 and b'B exceeds 65535' in last()
    assert lib.exa_mesh_arm_loss_backward(1, 8, p, None, p, p, None) == -2
    size = ctypes.c_uint64(7)
    assert lib.exa_mesh_hand_rgb_workspace_size(2, 300, ctypes.byref(size)) == 0 and size.value == 256     # 2 * 2 * 2 * 3 * 4 = 96 -> 256
    assert _lib.hand_rgb_workspace_size(3, 12000) == 3584                                                  # 2 * 3 * 47 * 3 * 4 = 3384
    assert lib.exa_mesh_hand_rgb_workspace_size(2, -1, ctypes.byref(size)) == -1
    assert lib.exa_mesh_hand_rgb_workspace_size(2, 3, None) == -2
    assert lib.exa_mesh_hand_rgb_forward(1, 8, 9, p, p, p, p, 256, p, p, None) == -1 and b'N (vertices per hand)' in last()
    assert lib.exa_mesh_hand_rgb_forward(1, 800, 300, p, p, p, p, 64, p, p, None) == -1 and b'workspace is smaller' in last()
    assert lib.exa_mesh_hand_rgb_forward(1, 8, 3, p, p, p, None, 256, p, p, None) == -2
    assert lib.exa_mesh_hand_rgb_backward(1, 8, 3, p, None, p, p, p, p, None) == -2 and b'means / grad_loss' in last()
    assert lib.exa_mesh_hand_mean_forward(1, 8, 9, p, p, p, p, None) == -1 and b'H (hand vertices)' in last()
    assert lib.exa_mesh_hand_mean_forward(1, 8, 3, p, None, p, p, None) == -2
    assert lib.exa_mesh_hand_mean_forward(1, 8, 0, None, None, None, None, None) == 0                        # an empty list: a no-op
    assert lib.exa_mesh_hand_mean_backward(1, 8, 3, p, p, None, p, p, None) == -2 and b'grad_loss is NULL' in last()
    with pytest.raises(RuntimeError, match='exa_mesh: .*dL_doffset'):
        _lib.MESH.check(lib.exa_mesh_hand_mean_backward(1, 8, 3, p, p, p, p, None, None))


def test_index_and_rank_tables():
    mask = torch.tensor([0, 1, 1, 0, 0, 1, 0], dtype=torch.bool)
    idx, rank = index_tables(mask)
    assert idx.dtype == torch.int32 and rank.dtype == torch.int32
    assert idx.tolist() == [1, 2, 5] and rank.tolist() == [-1, 0, 1, -1, -1, 2, -1]
    rng = np.random.RandomState(0)
    big = rng.uniform(size=1000) < 0.3
    idx, rank = index_tables(torch.from_numpy(big))
    want_idx, want_rank = ro.index_tables(big)
    assert np.array_equal(idx.numpy(), want_idx) and np.array_equal(rank.numpy(), want_rank)
    idx, rank = index_tables(torch.zeros(5, dtype=torch.bool))
    assert idx.numel() == 0 and rank.tolist() == [-1] * 5
    # the cache: one entry per pair of mask objects, rebuilt after an in-place change; the union in ascending order
    r, l = _mask(0, 4, 7), _mask(4, 2, 9)
    t1 = vr._hands(r, l)
    assert vr._hands(r, l) is t1
    assert t1['r'][0].tolist() == [0, 4, 7] and t1['l'][0].tolist() == [2, 4, 9] and t1['h'][0].tolist() == [0, 2, 4, 7, 9]
    assert t1['h'][1].tolist() == [0, -1, 1, -1, 2, -1, -1, 3, -1, 4, -1, -1]
    r[1] = True
    t2 = vr._hands(r, l)
    assert t2 is not t1 and t2['r'][0].tolist() == [0, 1, 4, 7]


def test_arm_class_memoises_its_plan_on_the_identity_of_its_inputs(monkeypatch):
    built = []

    def fake_neighbors(mesh, up, lo, thr, top_k):
        built.append((mesh, up, lo, thr, top_k))
        return len(built)

    monkeypatch.setattr(vr, 'arm_neighbors', fake_neighbors)
    monkeypatch.setattr(vr, 'arm_rgb_loss', lambda plan, rgb: rgb * plan)
    reg = ArmRGBReg()
    mesh, up, lo, rgb = _mesh(), _mask(0, 1), _mask(2, 3, 4), torch.ones(2, V, 3)
    out = reg(mesh, up, lo, rgb)
    assert tuple(out.shape) == (2, 3, 3) and len(built) == 1 and built[0][3:] == (0.01, 50)
    reg(mesh, up, lo, rgb * 2)
    assert len(built) == 1 and reg.plan == 1, 'the same objects: the same plan'
    mesh.add_(1.0)
    reg(mesh, up, lo, rgb)
    assert len(built) == 2, 'an in-place change of the mesh rebuilds it'
    lo[5] = True
    assert tuple(reg(mesh, up, lo, rgb).shape) == (2, 4, 3) and len(built) == 3, 'and so does one of a mask'
    reg(mesh.clone(), up, lo, rgb)
    assert len(built) == 4, 'an equal tensor that is another object is not the same input'
    reg(mesh, up, lo, rgb)
    assert len(built) == 5
    assert tuple(reg(mesh, up, torch.zeros_like(lo), rgb).shape) == (2, 0, 3), 'an empty lower arm: an empty result'
