"""CPU checks of the kinematics oracle (tests/kin_oracle.py) -- the restatement the HIP forward kinematics are held to:
in float64 it equals the reference's own code (tests/golden/ref_kinematics.npz, cut from smplx/lbs.py and module.py and
executed) and the autograd of the restated expression to 1e-12; in float32 it stays within its first-order bound
K u sum|terms| of float64 with at least a factor of 2 to spare; and it gives the known answers."""
import os

import numpy as np
import pytest
import torch

from exavatar_release_amd import lbs, p3d_standins
from tests import kin_oracle as ko

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_kinematics.npz')
CHAIN64 = tuple(range(-1, 63))
STAR64 = (-1,) + (0,) * 63


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _random_tree(J, rng):
    return tuple([-1] + [int(rng.integers(0, j)) for j in range(1, J)])


def test_float64_oracle_equals_the_reference_code_golden():
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 1 << 16
    # SMPL-X tree through get_transform_mat_joint: pose -> transforms, with the big-pose transforms
    parents = [int(p) for p in z['smplx_parents']]
    assert tuple(parents) == lbs.SMPLX_PARENTS
    pose, joints, pre, G = z['smplx_pose'], z['smplx_joints'][None], z['smplx_pre'][None], z['smplx_G'][None]
    assert not pose[23].any() and not pose[24].any(), 'the eyes are the zero rows'
    rot = ko.axis_angle_to_matrix(pose, np.float64)[None]
    out, _ = ko.forward(rot, joints, parents, pre, np.float64)
    assert _rel(out[0], z['smplx_transforms']) <= 1e-12
    grot, gj, gpre = ko.backward(rot, joints, parents, pre, G, None, np.float64)
    gpose = ko.axis_angle_backward(pose, grot[0], np.float64)
    assert np.isfinite(gpose).all()
    assert _rel(gpose, z['smplx_grad_pose']) <= 1e-12
    assert np.abs(gpose[23] - z['smplx_grad_pose'][23]).max() <= 1e-12 * np.abs(z['smplx_grad_pose']).max()
    assert _rel(gj[0], z['smplx_grad_joints']) <= 1e-12
    assert _rel(gpre[0], z['smplx_grad_pre']) <= 1e-12
    # J = 7, B = 3 through batch_rigid_transform: rotations -> (posed_joints, rel_transforms)
    parents = [int(p) for p in z['tree7_parents']]
    out, posed = ko.forward(z['tree7_rot'], z['tree7_joints'], parents, None, np.float64)
    assert _rel(out, z['tree7_transforms']) <= 1e-12 and _rel(posed, z['tree7_posed']) <= 1e-12
    grot, gj, gpre = ko.backward(z['tree7_rot'], z['tree7_joints'], parents, None, z['tree7_G_transforms'],
                                 z['tree7_G_posed'], np.float64)
    assert gpre is None
    assert _rel(grot, z['tree7_grad_rot']) <= 1e-12 and _rel(gj, z['tree7_grad_joints']) <= 1e-12


@pytest.mark.parametrize('J,tree,use_pre', [(55, 'smplx', True), (64, 'chain', False), (64, 'star', True),
                                            (1, 'random', True), (20, 'random', False)])
def test_float64_backward_is_autograd_of_the_restated_expression(J, tree, use_pre):
    rng = np.random.default_rng(J + len(tree))
    parents = {'smplx': lbs.SMPLX_PARENTS, 'chain': CHAIN64, 'star': STAR64}.get(tree) or _random_tree(J, rng)
    pose = 0.5 * rng.standard_normal((J, 3))
    pose[J // 2] = 0.0
    joints = 0.3 * rng.standard_normal((J, 3))
    pre = rng.standard_normal((J, 4, 4)) if use_pre else None      # a general matrix: row 3 is not (0, 0, 0, 1)
    G, Gp = rng.standard_normal((J, 4, 4)), rng.standard_normal((J, 3))
    tt = lambda a: None if a is None else torch.tensor(a, dtype=torch.float64, requires_grad=True)      # noqa: E731
    tp, tj, tpre = tt(pose), tt(joints), tt(pre)
    T, posed, rot = ko.reference_expression(tp, tj, parents, tpre)
    inputs = [tp, tj] + ([tpre] if use_pre else [])
    grads = torch.autograd.grad([T, posed], inputs, [torch.tensor(G), torch.tensor(Gp)])
    R = ko.axis_angle_to_matrix(pose, np.float64)
    assert _rel(R, rot.detach().numpy()) <= 1e-12
    out, op = ko.forward(R[None], joints[None], parents, None if pre is None else pre[None], np.float64)
    assert _rel(out[0], T.detach().numpy()) <= 1e-12 and _rel(op[0], posed.detach().numpy()) <= 1e-12
    grot, gj, gpre = ko.backward(R[None], joints[None], parents, None if pre is None else pre[None], G[None], Gp[None],
                                 np.float64)
    assert _rel(ko.axis_angle_backward(pose, grot[0], np.float64), grads[0].numpy()) <= 1e-11
    assert _rel(gj[0], grads[1].numpy()) <= 1e-12
    if use_pre:
        assert _rel(gpre[0], grads[2].numpy()) <= 1e-12


def _depth(parents):
    return max(ko.depths(parents))


@pytest.mark.parametrize('J,tree,use_pre,B', [(55, 'smplx', True, 4), (64, 'chain', True, 2), (64, 'star', False, 2),
                                              (24, 'random', False, 8)])
def test_float32_oracle_is_within_its_bound_with_a_factor_two_to_spare(J, tree, use_pre, B):
    rng = np.random.default_rng(3 * J + B)
    parents = {'smplx': lbs.SMPLX_PARENTS, 'chain': CHAIN64, 'star': STAR64}.get(tree) or _random_tree(J, rng)
    f32 = lambda a: np.asarray(a, np.float32)      # noqa: E731
    rot = f32(ko.axis_angle_to_matrix(0.5 * rng.standard_normal((B, J, 3)), np.float64))
    joints = f32(0.3 * rng.standard_normal((B, J, 3)))
    pre = f32(rng.standard_normal((B, J, 4, 4))) if use_pre else None
    G, Gp = f32(rng.standard_normal((B, J, 4, 4))), f32(rng.standard_normal((B, J, 3)))
    a32 = ko.forward(rot, joints, parents, pre, np.float32) + ko.backward(rot, joints, parents, pre, G, Gp, np.float32)
    a64 = ko.forward(rot, joints, parents, pre, np.float64) + ko.backward(rot, joints, parents, pre, G, Gp, np.float64)
    mags = ko.magnitudes(rot, joints, parents, pre, G, Gp)
    D = _depth(parents)
    Ks = [ko.k_forward(D, use_pre)] * 2 + [ko.k_backward(D, J, use_pre)] * 3
    for x32, x64, m, K in zip(a32, a64, mags, Ks):
        if x32 is None:
            continue
        assert x32.dtype == np.float32 and x64.dtype == np.float64
        err = np.abs(x32.astype(np.float64) - x64)
        ratio = float((err / (ko.U * m + 1e-300)).max())
        assert ratio <= K / 2, (ratio, K)


def test_depths_and_invalid_trees():
    assert ko.depths(lbs.SMPLX_PARENTS)[:5] == [0, 1, 1, 1, 2] and max(ko.depths(lbs.SMPLX_PARENTS)) == 10
    assert ko.depths(CHAIN64) == list(range(64)) and ko.depths(STAR64) == [0] + [1] * 63
    for bad in ((0, 0), (-1, 1), (-1, -1), (-1, 0, 2), (), (-1,) + (0,) * 64):
        with pytest.raises(ValueError):
            ko.depths(bad)


def test_known_answers():
    rng = np.random.default_rng(5)
    J, parents = 55, lbs.SMPLX_PARENTS
    joints = rng.standard_normal((1, J, 3)).astype(np.float32)
    eye = np.tile(np.eye(3, dtype=np.float32), (1, J, 1, 1))
    # the identity pose: A is the identity up to the rounding of the rest-location step (1 u per level); the rotation
    # part and the posed joints of the root are exact
    assert np.array_equal(ko.axis_angle_to_matrix(np.zeros((J, 3), np.float32)), eye[0])
    A, posed = ko.forward(eye, joints, parents)
    assert np.array_equal(A[0, :, :3, :3], eye[0]) and np.array_equal(A[0, :, 3], np.tile([0, 0, 0, 1], (J, 1)))
    assert np.abs(A[0, :, :3, 3]).max() <= 16 * 2.0 ** -23 * np.abs(joints).max()
    assert np.abs(posed - joints).max() <= 16 * 2.0 ** -23 * np.abs(joints).max()
    A64, posed64 = ko.forward(eye, joints, parents, dtype=np.float64)
    assert np.abs(A64[0, :, :3, 3]).max() <= 1e-15 and np.abs(posed64 - joints).max() <= 1e-15
    # a root rotation is rigid: every joint's transform is the root's, the posed joints keep their distances
    pose = np.zeros((J, 3))
    pose[0] = [0.3, -0.5, 0.2]
    R = ko.axis_angle_to_matrix(pose, np.float64)[None]
    A, posed = ko.forward(R, joints, parents, dtype=np.float64)
    assert np.abs(A - A[:, :1]).max() <= 1e-14
    dist = lambda p: np.linalg.norm(p[0, :, None] - p[0, None, :], axis=-1)      # noqa: E731
    assert np.abs(dist(posed) - dist(joints.astype(np.float64))).max() <= 1e-14
    # a straight chain along x, every joint turned by a about z: joint k sits at the sum of the unit steps turned by
    # a, 2 a, .., k a
    n, a = 8, 0.3
    chain = tuple(range(-1, n - 1))
    jt = np.zeros((1, n, 3))
    jt[0, :, 0] = np.arange(n)
    pz = np.zeros((n, 3))
    pz[:, 2] = a
    _, posed = ko.forward(ko.axis_angle_to_matrix(pz, np.float64)[None], jt, chain, dtype=np.float64)
    want = np.zeros((n, 3))
    for k in range(1, n):
        want[k] = want[k - 1] + [np.cos(k * a), np.sin(k * a), 0]
    assert np.abs(posed[0] - want).max() <= 1e-14


def test_zero_pose_rows_take_the_half_identity_route():
    """At angle == 0, q = (1, x / 2, y / 2, z / 2) to first order and d angle / d x := 0: dR[2, 1] / dx = 1, and the
    gradient equals torch's autograd of the stand-in (whose ``norm`` has the zero subgradient), finite."""
    G = np.zeros((1, 3, 3))
    G[0, 2, 1] = 1.0
    g = ko.axis_angle_backward(np.zeros((1, 3)), G, np.float64)
    assert np.array_equal(g, [[1.0, 0.0, 0.0]])
    rng = np.random.default_rng(6)
    G = rng.standard_normal((4, 3, 3))
    for dtype, tdtype in ((np.float64, torch.float64), (np.float32, torch.float32)):
        p = torch.zeros(4, 3, dtype=tdtype, requires_grad=True)
        (want,) = torch.autograd.grad(p3d_standins.axis_angle_to_matrix(p), p, torch.tensor(G, dtype=tdtype))
        got = ko.axis_angle_backward(np.zeros((4, 3)), G, dtype)
        assert np.isfinite(got).all() and np.abs(got - want.numpy()).max() <= 1e-6
        # 0.5 I: the quaternion's vector part has gradient s = 0.5 per axis
        skew = np.stack([G[:, 2, 1] - G[:, 1, 2], G[:, 0, 2] - G[:, 2, 0], G[:, 1, 0] - G[:, 0, 1]], -1)
        assert np.abs(got - skew).max() <= 1e-6


@pytest.mark.parametrize('angle', [0.0, 0.5e-6, 0.99e-6, 1.01e-6, 2e-6, 1e-3, np.pi - 1e-4, np.pi, np.pi + 1e-4, 6.0])
def test_angles_at_the_small_angle_switch_and_near_pi(angle):
    rng = np.random.default_rng(7)
    axis = rng.standard_normal((6, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    pose = angle * axis
    G = rng.standard_normal((6, 3, 3))
    p = torch.tensor(pose, requires_grad=True)
    R = p3d_standins.axis_angle_to_matrix(p)
    (want,) = torch.autograd.grad(R, p, torch.tensor(G))
    got_R = ko.axis_angle_to_matrix(pose, np.float64)
    assert np.abs(got_R - R.detach().numpy()).max() <= 1e-14
    assert np.abs(got_R @ got_R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-12
    got = ko.axis_angle_backward(pose, G, np.float64)
    assert np.abs(got - want.numpy()).max() <= 1e-9 * max(1.0, np.abs(want.numpy()).max())
    # float32: the rotation stays a rotation to a few ulp on both sides of the switch
    R32 = ko.axis_angle_to_matrix(pose.astype(np.float32))
    assert np.abs(R32.astype(np.float64) - got_R).max() <= 8 * 2.0 ** -23
