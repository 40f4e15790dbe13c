"""HIP pose parameters: a drop-in for ExAvatar's ``SMPLXParamDict`` and the pose features ``HumanGaussian`` rebuilds.

* ``pose_params(d6, *, packed=False)`` -- ``matrix_to_axis_angle(rotation_6d_to_matrix(p))`` (reference
  ``avatar/common/nets/module.py:680``) for a whole sequence of 6D tensors in ONE launch, and one more for the gradients
  of them all.  The torch expression is 86 autograd nodes per tensor and indexes with a boolean mask nine times, each a
  read-back of the device: it cannot be captured into a hipGraph; this can.
* ``pose_features(rot, n_body)`` -- the two detached features of ``module.py:464,484,498`` from the kinematics' ``rot``:
  ``matrix_to_rotation_6d(rot[1:1 + n_body])`` flattened, and ``(rot[1:] - I).view(1, 9 (J - 1))``.
* ``SMPLXParamDict`` -- the reference's module (``module.py:649-684``): the same nested ``ParameterDict``, the same
  ``state_dict`` keys, shapes and values, the same optimizer groups; ``forward`` runs every frame of the call through
  ``pose_params`` at once.

The kernels are ``csrc/pose_params.hip`` behind ``include/exa_mesh.h`` (``exa_mesh_pose_*``), which writes out every
operation; ROCm device tensors only, no CPU path.  The CPU restatement that pins them is ``tests/pose_oracle.py``.

Semantics
---------
torch's, as ``p3d_standins`` states pytorch3d's functions: ``F.normalize``'s ``eps = 1e-12``; the lowest index wins a
tie of the four quaternion candidates; no gradient through the candidate index, the sign flip or the choice between
``sin(half) / angle`` and its series below ``|angle| < 1e-6``; ``norm``'s gradient is 0 at 0, so the identity row
``(1, 0, 0, 0, 1, 0)`` (the eyes) gets a finite gradient.  The quaternion is bit-equal to the float32 oracle; the
axis-angle passes the device's ``atan2f`` / ``sinf``.

The tensors stay where they are -- the seven ``nn.Parameter`` s of a frame are seven allocations -- and their addresses
travel to the kernel by value: no concatenation, no device buffer, no state.  Up to 64 tensors are one C call each way
(nine frames); more are issued as several.  Nothing is summed across rows, so the same inputs give the same bits.  A
missing cotangent travels as NULL, an input that needs no gradient gets none and none is computed for it, and each call
allocates its outputs and launches without synchronising: it can be captured.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib, p3d_standins
from ._device import _ptr, _ptrs, check_no_grad, check_tensor, grad_in, launch, need_rocm

MAX_SEGMENTS = 64         # EXA_MESH_POSE_MAX_SEGMENTS
MAX_JOINTS = 64           # EXA_MESH_KIN_MAX_JOINTS

PARAM_NAMES = ('root_pose', 'body_pose', 'jaw_pose', 'leye_pose', 'reye_pose', 'lhand_pose', 'rhand_pose', 'expr',
               'trans')


def _rows(tensors):
    return (ctypes.c_int32 * len(tensors))(*[t.numel() // 6 for t in tensors])


class _PoseParams(torch.autograd.Function):
    """packed: bool, d6: float32 contiguous [..., 6] tensors of one ROCm device -> the [..., 3] axis-angle tensors, then
    the packed [R, 3] when asked for."""

    @staticmethod
    def forward(ctx, packed, *d6):
        dev = d6[0].device
        outs = [torch.empty(t.shape[:-1] + (3,), dtype=torch.float32, device=dev) for t in d6]
        R = sum(t.numel() // 6 for t in d6)
        pk = torch.empty((R, 3), dtype=torch.float32, device=dev) if packed else None
        row = 0
        for i in range(0, len(d6), MAX_SEGMENTS):
            seg, out = d6[i:i + MAX_SEGMENTS], outs[i:i + MAX_SEGMENTS]
            launch(_lib.MESH, 'exa_mesh_pose_params_forward', dev, len(seg), _rows(seg), _ptrs(seg), _ptrs(out),
                   _ptr(pk[row:]) if packed else None, None)
            row += sum(t.numel() // 6 for t in seg)
        ctx.save_for_backward(*d6)
        ctx.packed = packed
        ctx.set_materialize_grads(False)      # a missing cotangent arrives as None and travels as NULL
        return (*outs, pk) if packed else tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        d6 = ctx.saved_tensors
        n = len(d6)
        need = ctx.needs_input_grad[1:]
        g_out = [grad_in(g) for g in grads[:n]]
        g_pk = grad_in(grads[n]) if ctx.packed else None
        if g_pk is None and all(g is None for g in g_out):
            return (None,) * (n + 1)
        dev = d6[0].device
        # a tensor whose rows have no cotangent from either side still gets its (zero) gradient from the kernel
        g_d6 = [torch.empty_like(t) if w else None for t, w in zip(d6, need)]
        row = 0
        for i in range(0, n, MAX_SEGMENTS):
            seg = d6[i:i + MAX_SEGMENTS]
            if any(g is not None for g in g_d6[i:i + MAX_SEGMENTS]):
                launch(_lib.MESH, 'exa_mesh_pose_params_backward', dev, len(seg), _rows(seg), _ptrs(seg),
                       _ptrs(g_out[i:i + MAX_SEGMENTS]), _ptr(g_pk[row:]) if g_pk is not None else None,
                       _ptrs(g_d6[i:i + MAX_SEGMENTS]))
            row += sum(t.numel() // 6 for t in seg)
        return (None, *g_d6)


def pose_params(d6, *, packed=False):
    """Axis-angle of 6D rotation tensors: ``d6`` a sequence of float32 ROCm tensors ``[..., 6]`` -> the tuple of
    ``[..., 3]`` tensors ``matrix_to_axis_angle(rotation_6d_to_matrix(t))``; with ``packed=True`` one more element, the
    ``[R, 3]`` tensor of all rows in the sequence's order (for the pose tensors of one frame: the ``[55, 3]`` pose
    ``joint_transforms`` takes, without a ``torch.cat``).  Gradients reach every tensor that requires one, from the
    separate outputs and the packed one alike."""
    what = 'pose_params'
    d6 = tuple(d6)
    for i, t in enumerate(d6):
        check_tensor(what, 'd6[%d]' % i, t)
    for i, t in enumerate(d6):
        if t.dim() < 1 or t.shape[-1] != 6:
            raise ValueError('%s: d6[%d] must be [..., 6] (it has %s)' % (what, i, tuple(t.shape)))
    for i, t in enumerate(d6):
        check_tensor(what, 'd6[%d]' % i, t, f32=False, rocm=True, on=(d6[0], 'd6[0]'))
    if not d6:
        return ()
    return _PoseParams.apply(bool(packed), *[t.contiguous() for t in d6])


def pose_features(rot, n_body):
    """``(pose6d [6 n_body], pose_feat [1, 9 (J - 1)])`` from the kinematics' ``rot`` [J, 3, 3] (float32, ROCm, J <= 64):
    the first two rows of ``rot[1 .. n_body]`` -- ``matrix_to_rotation_6d`` of the body joints without the root,
    ``module.py:464,498`` -- and ``rot[1:] - I`` (``module.py:484``), in one launch.  The reference detaches both: they
    carry no gradient, and a ``rot`` that requires one is refused."""
    what = 'pose_features'
    check_tensor(what, 'rot', rot)
    check_no_grad(what, 'rot', rot, 'detached')
    if rot.dim() != 3 or tuple(rot.shape[1:]) != (3, 3) or not 1 <= rot.shape[0] <= MAX_JOINTS:
        raise ValueError('%s: rot must be [J, 3, 3] with 1 <= J <= %d (it has %s)' % (what, MAX_JOINTS, tuple(rot.shape)))
    J, n_body = rot.shape[0], int(n_body)
    if not 0 <= n_body <= J - 1:
        raise ValueError('%s: n_body = %d asks for more rows than rot[1:] has (%d)' % (what, n_body, J - 1))
    need_rocm(rot.device, what)
    rot = rot.contiguous()
    pose6d = torch.empty(6 * n_body, dtype=torch.float32, device=rot.device)
    pose_feat = torch.empty((1, 9 * (J - 1)), dtype=torch.float32, device=rot.device)
    launch(_lib.MESH, 'exa_mesh_pose_features', rot.device, J, n_body, _ptr(rot), _ptr(pose6d), _ptr(pose_feat))
    return pose6d, pose_feat


class SMPLXParamDict(nn.Module):
    """The reference's per-frame SMPL-X parameters (``module.py:649-684``): ``smplx_params[str(frame)][name]`` for the
    nine names of a frame, the seven poses stored as 6D rotations.  ``state_dict`` keys, shapes and values are the
    reference's, so checkpoints load both ways."""

    def __init__(self):
        super(SMPLXParamDict, self).__init__()

    def init(self, smplx_params, device=None):
        """``smplx_params``: {frame index: {name: tensor}} with axis-angle poses, as the reference's datasets hand them
        over.  The parameters are created on the tensors' own device, or on ``device``; the 6D values are
        ``matrix_to_rotation_6d(axis_angle_to_matrix(x))`` by ``p3d_standins``, once."""
        _smplx_params = {}
        for frame_idx in smplx_params.keys():
            frame = nn.ParameterDict({})
            for param_name in PARAM_NAMES:
                x = smplx_params[frame_idx][param_name]
                if device is not None:
                    x = x.to(device)
                if 'pose' in param_name:
                    x = p3d_standins.matrix_to_rotation_6d(p3d_standins.axis_angle_to_matrix(x))
                frame[param_name] = nn.Parameter(x.detach().clone())
            _smplx_params[str(frame_idx)] = frame
        self.smplx_params = nn.ParameterDict(_smplx_params)

    def get_optimizable_params(self, lr):
        """The reference's optimizer groups, one per parameter, in its order; ``lr`` is its ``cfg.smplx_param_lr``."""
        optimizable_params = []
        for frame_idx in self.smplx_params.keys():
            for param_name in self.smplx_params[frame_idx].keys():
                optimizable_params.append({'params': [self.smplx_params[frame_idx][param_name]],
                                           'name': 'smplx_' + param_name + '_' + frame_idx, 'lr': lr})
        return optimizable_params

    def forward(self, frame_idxs, packed=False):
        """The reference's list of dicts, one per frame: the pose entries as axis-angle, ``expr`` and ``trans`` the
        Parameters themselves.  With ``packed=True`` every dict has one more key, ``'pose'``: the frame's pose rows in
        its keys' order, ``[55, 3]`` for SMPL-X.  All frames of the call share one launch each way (up to nine)."""
        what = 'SMPLXParamDict.forward'
        frames, d6 = [], []
        for frame_idx in frame_idxs:
            frame_idx = str(int(frame_idx))
            if frame_idx not in self.smplx_params:
                raise KeyError('%s: no frame %s among the %d initialised' % (what, frame_idx, len(self.smplx_params)))
            names = list(self.smplx_params[frame_idx].keys())
            frames.append((frame_idx, names))
            d6 += [self.smplx_params[frame_idx][n] for n in names if 'pose' in n]
        for t in d6:
            need_rocm(t.device, what)
        res = pose_params(d6, packed=packed)
        out, spans, k, row = [], [], 0, 0
        for frame_idx, names in frames:
            smplx_param, first = {}, row
            for param_name in names:
                if 'pose' in param_name:
                    smplx_param[param_name] = res[k]
                    row += res[k].numel() // 3
                    k += 1
                else:
                    smplx_param[param_name] = self.smplx_params[frame_idx][param_name]
            spans.append((first, row))
            out.append(smplx_param)
        if packed:
            # One frame: the packed tensor itself.  Frames of one size (SMPL-X: 55 rows each): one unbind, whose backward
            # is one stack of the frames' cotangents.  Otherwise one slice per frame.
            sizes = {b - a for a, b in spans}
            if len(out) == 1:
                poses = [res[-1]]
            elif len(sizes) == 1 and 0 not in sizes:
                poses = res[-1].view(len(out), sizes.pop(), 3).unbind(0)
            else:
                poses = [res[-1][a:b] for a, b in spans]
            for smplx_param, pose in zip(out, poses):
                smplx_param['pose'] = pose
        return out
