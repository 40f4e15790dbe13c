"""CPU tests of the forward kinematics' host side: ``exa_mesh_kinematics_depths`` through ctypes, every invalid argument
fails with its negative status and its message before any GPU work, and the Python surface refuses what it does not
support.  The ABI itself (include/exa_mesh.h against its binding) is checked by tests/test_abi.py."""
import ctypes

import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import _lib, build, kinematics, lbs
from tests import kin_oracle as ko

BAD = ctypes.c_void_p(0x1000)      # never dereferenced: every call below fails validation first
INVALID, NULLPTR = -1, -2
CHAIN64 = tuple(range(-1, 63))


def _ints(values):
    return (ctypes.c_int32 * len(values))(*values)


def _depths(parents, J=None):
    lib = _lib.load()
    out = (ctypes.c_int32 * max(len(parents), 1))()
    rc = lib.exa_mesh_kinematics_depths(len(parents) if J is None else J, _ints(parents), out)
    return rc, list(out)[:len(parents)], lib.exa_mesh_last_error()


def test_depths_of_the_smplx_tree_and_of_a_chain():
    rc, d, _ = _depths(lbs.SMPLX_PARENTS)
    assert rc == 0 and d == ko.depths(lbs.SMPLX_PARENTS) and max(d) == 10
    rc, d, _ = _depths(CHAIN64)
    assert rc == 0 and d == list(range(64))
    rc, d, _ = _depths((-1,))
    assert rc == 0 and d == [0]


def test_depths_rejects_bad_trees_with_a_message():
    rc, _, msg = _depths((0, 0, 1))
    assert rc == INVALID and msg.startswith(b'exa_mesh: ') and b'parents[0] must be -1' in msg
    rc, _, msg = _depths((-1, 0, 2, 1))
    assert rc == INVALID and b'parents[2] = 2 must lie in [0, 2)' in msg
    rc, _, msg = _depths((-1, 0, -1))
    assert rc == INVALID and b'parents[2] = -1' in msg
    rc, _, msg = _depths((-1,), J=0)
    assert rc == INVALID and b'J (joints) must be 1 .. 64' in msg
    rc, _, msg = _depths((-1,) + (0,) * 64)
    assert rc == INVALID and b'J (joints) must be 1 .. 64' in msg
    lib = _lib.load()
    assert lib.exa_mesh_kinematics_depths(3, None, (ctypes.c_int32 * 3)()) == NULLPTR
    assert lib.exa_mesh_kinematics_depths(3, _ints((-1, 0, 0)), None) == NULLPTR
    assert b'depth_out is NULL' in lib.exa_mesh_last_error()


def test_forward_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()

    def fwd(B=2, J=3, parents=(-1, 0, 1), pose=BAD, rot_in=None, joints=BAD, pre=BAD, T=BAD, posed=BAD, rot=BAD):
        p = None if parents is None else _ints(parents)
        return lib.exa_mesh_kinematics_forward(B, J, p, pose, rot_in, joints, pre, T, posed, rot, None)

    err = lib.exa_mesh_last_error
    assert fwd(B=-1) == INVALID and b'negative size' in err()
    assert fwd(B=(1 << 20) + 1) == INVALID
    assert fwd(J=0) == INVALID and b'J (joints)' in err()
    assert fwd(J=65, parents=(-1,) + (0,) * 64) == INVALID and b'J (joints)' in err()
    assert fwd(parents=(0, 0, 1)) == INVALID and b'parents[0] must be -1' in err()
    assert fwd(parents=(-1, 1, 1)) == INVALID and b'parents[1] = 1' in err()
    assert fwd(parents=(-1, 0, 2)) == INVALID and b'parents[2] = 2' in err()
    assert fwd(parents=None) == NULLPTR and b'parents is NULL' in err()
    assert fwd(pose=BAD, rot_in=BAD) == INVALID and b'exactly one of pose / rot_in' in err()
    assert fwd(pose=None, rot_in=None) == INVALID and b'exactly one of pose / rot_in' in err()
    assert fwd(joints=None) == NULLPTR and b'joints is NULL' in err()
    for k in ('T', 'posed', 'rot'):
        assert fwd(**{k: None}) == NULLPTR and b'transforms / posed_joints / rot is NULL' in err(), k
    assert fwd(B=0, pose=None, joints=None, pre=None, T=None, posed=None, rot=None) == 0      # nothing to do
    assert fwd(B=0, parents=(-1, 0, 2)) == INVALID                                            # the tree is still checked


def test_backward_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()

    def bwd(B=2, J=3, parents=(-1, 0, 1), pose=BAD, rot=BAD, joints=BAD, pre=BAD, gT=BAD, gposed=BAD, gpose=BAD,
            grot=None, gjoints=BAD, gpre=BAD):
        p = None if parents is None else _ints(parents)
        return lib.exa_mesh_kinematics_backward(B, J, p, pose, rot, joints, pre, gT, gposed, gpose, grot, gjoints, gpre,
                                                None)

    err = lib.exa_mesh_last_error
    assert bwd(B=-2) == INVALID
    assert bwd(J=65, parents=(-1,) + (0,) * 64) == INVALID and bwd(J=0) == INVALID
    assert bwd(parents=(-1, 0, 3)) == INVALID and b'parents[2] = 3' in err()
    assert bwd(parents=(1, 0, 1)) == INVALID and b'parents[0]' in err()
    assert bwd(rot=None) == NULLPTR and bwd(joints=None) == NULLPTR and b'rot / joints is NULL' in err()
    assert bwd(pose=None) == NULLPTR and b'grad_pose needs pose' in err()
    assert bwd(pre=None) == NULLPTR and b'grad_pre needs pre' in err()
    # no output wanted, or no skeleton: a successful no-op
    assert bwd(gpose=None, grot=None, gjoints=None, gpre=None, rot=None, joints=None) == 0
    assert bwd(B=0, rot=None, joints=None) == 0


def test_python_surface_raises_as_specified():
    for name in ('joint_transforms', 'batch_rigid_transform'):
        assert name in exa.__all__ and getattr(exa, name) is getattr(kinematics, name)
    assert build.SOURCES['kinematics.hip'] == ['-ffp-contract=off']
    J = 55
    P = lbs.SMPLX_PARENTS
    pose, joints, pre = torch.zeros(J, 3), torch.zeros(J, 3), torch.eye(4).repeat(J, 1, 1)
    jt = exa.joint_transforms
    with pytest.raises(RuntimeError, match=r'joint_transforms runs on a ROCm device only \(no CPU path\)'):
        jt(pose, joints, P, pre)
    with pytest.raises(RuntimeError, match='batch_rigid_transform runs on a ROCm device only'):
        exa.batch_rigid_transform(torch.eye(3).repeat(1, J, 1, 1), joints[None], torch.tensor(P))
    with pytest.raises(TypeError, match='joint_transforms: pose must be a tensor'):
        jt(pose.numpy(), joints, P)
    with pytest.raises(ValueError, match=r'joint_transforms: joints must be float32 \(it is torch.float64\)'):
        jt(pose, joints.double(), P)
    with pytest.raises(ValueError, match=r'joint_transforms: pre must be float32'):
        jt(pose, joints, P, pre.half())
    with pytest.raises(ValueError, match=r'pose must be \[J, 3\] or \[B, J, 3\] with J = 55'):
        jt(pose[:54], joints, P)
    with pytest.raises(ValueError, match=r'pose must be \[J, 3, 3\] or \[B, J, 3, 3\]'):
        jt(pose, joints, P, rotations=True)
    with pytest.raises(ValueError, match=r'joints must be \[J, 3\] or \[B, J, 3\]'):
        jt(pose, joints[:, :2], P)
    with pytest.raises(ValueError, match=r'pre must be \[J, 4, 4\] or \[B, J, 4, 4\]'):
        jt(pose, joints, P, pre[:, :3])
    with pytest.raises(ValueError, match='disagree on the batch size'):
        jt(pose.repeat(2, 1, 1), joints.repeat(3, 1, 1), P)
    with pytest.raises(ValueError, match='parents must name 1 .. 64 joints'):
        jt(torch.zeros(65, 3), torch.zeros(65, 3), (-1,) + (0,) * 64)
    with pytest.raises(TypeError, match='parents must be a sequence'):
        jt(pose, joints, 55)
    with pytest.raises(RuntimeError, match=r'exa_mesh: parents\[2\] = 2 must lie in \[0, 2\)'):
        jt(torch.zeros(3, 3), torch.zeros(3, 3), (-1, 0, 2))
    with pytest.raises(RuntimeError, match=r'exa_mesh: parents\[0\] must be -1'):
        jt(torch.zeros(2, 3), torch.zeros(2, 3), [0, 0])
    with pytest.raises(ValueError, match='dtype must be float32'):
        exa.batch_rigid_transform(torch.eye(3).repeat(1, J, 1, 1), joints[None], P, dtype=torch.float64)
