"""HIP forward kinematics: a drop-in for ExAvatar's ``get_transform_mat_joint`` and smplx's ``batch_rigid_transform``.

* ``joint_transforms(pose, joints, parents, pre=None, *, rotations=False)`` -- reference
  ``avatar/common/nets/module.py:389-411``: ``axis_angle_to_matrix`` on the poses, the kinematic chain of
  ``batch_rigid_transform`` and the ``bmm`` with the big-pose transforms ``pre``, in ONE launch (the reference runs 54
  dependent 4x4 ``matmul`` s plus ``pad`` / ``cat`` / ``stack`` around them, and autograd replays them all).  Returns
  ``(transforms, posed_joints, rot)``; gradients reach ``pose``, ``joints`` and ``pre``, bit-reproducibly.
* ``batch_rigid_transform(rot_mats, joints, parents, dtype=torch.float32)`` -- the vendored function's signature and
  return order (``avatar/common/utils/smplx/smplx/lbs.py:361-417``), for a one-line swap there.

The kernels are ``csrc/kinematics.hip`` behind ``include/exa_mesh.h`` (``exa_mesh_kinematics_*``); ROCm device tensors
only, no CPU path.  The CPU restatement that pins them is ``tests/kin_oracle.py``.

Semantics
---------
Per skeleton, with ``p = parents[j]``: ``R_j`` from the axis-angle row by pytorch3d's quaternion route (or the given
rotation), ``L_j = [R_j | joints_j - joints_p]`` (``joints_0`` for the root), ``W_j = W_p L_j`` level by level,
``posed_joints_j = W_j[:, 3]``, ``A_j = W_j`` with ``W_j[:, :3] joints_j`` taken off its translation, and
``transforms_j = A_j pre_j`` (``A_j`` without ``pre``).  Every operation is rounded in fp32 without fused multiply-adds,
in the order the header writes out; the one step a CPU does not reproduce bit for bit is the device's ``sinf`` /
``cosf``.  ``rot`` is returned detached: it is what ``module.py:464,484,498`` take for the 6D
pose row and the pose-corrective feature, which the reference detaches too.

The backward is one launch without atomics: the children's contributions are added into their parent in ascending child
index, so the same inputs give the same bits.  A zero pose row (the eyes) gets the finite gradient that torch's ``norm``
gives (``d angle / d x := 0`` at ``angle == 0``), not NaN.

``parents`` is a sequence or a CPU tensor of ints -- ``smplx_layer.parents.tolist()``, taken once -- checked on the host
and handed to the kernel by value: no device buffer, no copy, no state.  Each call allocates its outputs and launches one
kernel each way without synchronising, so it can be captured into a hipGraph.
"""
import ctypes

import torch

from . import _lib
from ._device import _ptr, check_tensor, grad_in, launch
from ._tables import Cache

MAX_JOINTS = 64           # EXA_MESH_KIN_MAX_JOINTS

_trees = Cache()          # the parents as a tuple -> the validated host array


def _tree(what, parents):
    """``parents`` as the host int32 array the C ABI takes (cached per tree, validated once by the library)."""
    if isinstance(parents, torch.Tensor):
        if parents.device.type != 'cpu':
            raise ValueError('%s: parents must be a sequence or a CPU tensor of ints (smplx_layer.parents.tolist())' % what)
        parents = parents.tolist()
    try:
        key = tuple(int(p) for p in parents)
    except (TypeError, ValueError):
        raise TypeError('%s: parents must be a sequence or a CPU tensor of ints' % what) from None
    arr = _trees.find(key)
    if arr is None:
        if not 1 <= len(key) <= MAX_JOINTS:
            raise ValueError('%s: parents must name 1 .. %d joints (got %d)' % (what, MAX_JOINTS, len(key)))
        arr = (ctypes.c_int32 * len(key))(*key)
        depth = (ctypes.c_int32 * len(key))()
        _lib.MESH.check(_lib.load().exa_mesh_kinematics_depths(len(key), arr, depth))
        _trees.keep(key, arr)
    return arr


class _Kinematics(torch.autograd.Function):
    """x [B, J, 3] axis-angle or [B, J, 3, 3] rotations, joints [B, J, 3], pre [B, J, 4, 4] or None (all float32,
    contiguous), tree: the host parents array -> (transforms [B, J, 4, 4], posed_joints [B, J, 3], rot [B, J, 3, 3])."""

    @staticmethod
    def forward(ctx, x, joints, pre, tree, rotations):
        B, J = joints.shape[0], joints.shape[1]
        dev = joints.device
        transforms = torch.empty((B, J, 4, 4), dtype=torch.float32, device=dev)
        posed = torch.empty((B, J, 3), dtype=torch.float32, device=dev)
        rot = torch.empty((B, J, 3, 3), dtype=torch.float32, device=dev)
        launch(_lib.MESH, 'exa_mesh_kinematics_forward', dev, B, J, tree, None if rotations else _ptr(x),
               _ptr(x) if rotations else None, _ptr(joints), _ptr(pre), _ptr(transforms), _ptr(posed), _ptr(rot))
        ctx.save_for_backward(None if rotations else x, rot, joints, pre)
        ctx.tree, ctx.rotations = tree, rotations
        ctx.mark_non_differentiable(rot)
        ctx.set_materialize_grads(False)      # a missing cotangent arrives as None and travels as NULL
        return transforms, posed, rot

    @staticmethod
    def backward(ctx, g_transforms, g_posed, _g_rot):
        pose, rot, joints, pre = ctx.saved_tensors
        B, J = joints.shape[0], joints.shape[1]
        dev = joints.device
        need = ctx.needs_input_grad
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
        gx = (new(B, J, 3, 3) if ctx.rotations else new(B, J, 3)) if need[0] else None
        gjoints = new(B, J, 3) if need[1] else None
        gpre = new(B, J, 4, 4) if need[2] and pre is not None else None
        if gx is not None or gjoints is not None or gpre is not None:
            launch(_lib.MESH, 'exa_mesh_kinematics_backward', dev, B, J, ctx.tree, _ptr(pose), _ptr(rot), _ptr(joints),
                   _ptr(pre), _ptr(grad_in(g_transforms)), _ptr(grad_in(g_posed)),
                   None if ctx.rotations else _ptr(gx), _ptr(gx) if ctx.rotations else None, _ptr(gjoints), _ptr(gpre))
        return gx, gjoints, gpre, None, None


def _joint_transforms(what, pose, joints, parents, pre, rotations):
    tree = _tree(what, parents)
    J = len(tree)
    tail = (J, 3, 3) if rotations else (J, 3)
    name = 'rot_mats' if what == 'batch_rigid_transform' else 'pose'
    check_tensor(what, name, pose)
    check_tensor(what, 'joints', joints)
    if pre is not None:
        check_tensor(what, 'pre', pre)
    if pose.dim() not in (len(tail), len(tail) + 1) or tuple(pose.shape[-len(tail):]) != tail:
        raise ValueError('%s: %s must be [J, %s] or [B, J, %s] with J = %d (it has %s)' % (
            what, name, *(('3, 3',) * 2 if rotations else ('3',) * 2), J, tuple(pose.shape)))
    if joints.dim() not in (2, 3) or tuple(joints.shape[-2:]) != (J, 3):
        raise ValueError('%s: joints must be [J, 3] or [B, J, 3] with J = %d (it has %s)' % (what, J, tuple(joints.shape)))
    if pre is not None and (pre.dim() not in (3, 4) or tuple(pre.shape[-3:]) != (J, 4, 4)):
        raise ValueError('%s: pre must be [J, 4, 4] or [B, J, 4, 4] with J = %d (it has %s)' % (what, J, tuple(pre.shape)))
    batched = pose.dim() == len(tail) + 1 or joints.dim() == 3 or (pre is not None and pre.dim() == 4)
    sizes = {x.shape[0] for x, d in ((pose, len(tail) + 1), (joints, 3), (pre, 4)) if x is not None and x.dim() == d}
    if len(sizes) > 1:
        raise ValueError('%s: %s, joints and pre disagree on the batch size (%s)' % (what, name, sorted(sizes)))
    B = sizes.pop() if sizes else 1
    for n, x in ((name, pose), ('joints', joints), ('pre', pre)):
        if x is not None:
            check_tensor(what, n, x, f32=False, rocm=True, on=(pose, name))
    # a tensor without the batch axis is shared by every skeleton: expand's backward adds the B gradients up
    x = (pose if pose.dim() == len(tail) + 1 else pose.expand((B,) + tail)).contiguous()
    jt = (joints if joints.dim() == 3 else joints.expand(B, J, 3)).contiguous()
    pr = None if pre is None else (pre if pre.dim() == 4 else pre.expand(B, J, 4, 4)).contiguous()
    transforms, posed, rot = _Kinematics.apply(x, jt, pr, tree, rotations)
    if not batched:
        transforms, posed, rot = transforms[0], posed[0], rot[0]
    return transforms, posed, rot


def joint_transforms(pose, joints, parents, pre=None, *, rotations=False):
    """The joints' rest -> posed transforms (module docstring): ``(transforms, posed_joints, rot)``.

    ``pose`` [J, 3] or [B, J, 3] axis-angle, or with ``rotations=True`` [J, 3, 3] or [B, J, 3, 3] rotation matrices;
    ``joints`` [J, 3] or [B, J, 3] rest locations; ``parents`` a sequence or CPU tensor of J ints (J <= 64,
    ``parents[0] == -1``, ``0 <= parents[i] < i``); ``pre`` [J, 4, 4] or [B, J, 4, 4] or None: transforms applied first
    (``transforms = A pre``, the reference's big pose -> zero pose).  The results carry the batch axis when any argument
    does.  ``rot`` [.., J, 3, 3] is detached."""
    return _joint_transforms('joint_transforms', pose, joints, parents, pre, rotations)


def batch_rigid_transform(rot_mats, joints, parents, dtype=torch.float32):
    """smplx's ``batch_rigid_transform``: ``rot_mats`` [B, N, 3, 3], ``joints`` [B, N, 3] -> ``(posed_joints [B, N, 3],
    rel_transforms [B, N, 4, 4])``.  ``parents`` as in ``joint_transforms``; a device tensor (what ``smplx_layer.parents``
    is) is accepted here and read back with ``.tolist()``, which synchronises: hand over the list to avoid that.
    ``dtype`` must be float32."""
    what = 'batch_rigid_transform'
    if dtype != torch.float32:
        raise ValueError('batch_rigid_transform: dtype must be float32 (it is %s)' % dtype)
    if isinstance(parents, torch.Tensor) and parents.device.type != 'cpu':
        parents = parents.tolist()
    transforms, posed, _ = _joint_transforms(what, rot_mats, joints, parents, None, True)
    return posed, transforms
