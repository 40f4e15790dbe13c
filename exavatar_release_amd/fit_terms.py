"""HIP mesh terms of the fitting loss: the four gather-style terms of ``fitting/main/model.py:207-252`` that had no HIP form.

* ``EdgeLengthLoss(face)`` -- reference ``fitting/common/nets/loss.py:125-149``: ``forward(coord_out, coord_gt, valid)`` returns
  ``[B, 3F, 1]`` in the reference's ``cat`` order (all ``(v0, v1)`` edges, then ``(v0, v2)``, then ``(v1, v2)``).  ``coord_gt``
  is ``[B, V, 3]`` or ``[1, V, 3]``, ``valid`` ``[1, V, 1]``, ``[B, V, 1]`` or ``[V]``.  The face table goes to the device once
  (the reference copies it on every call).
* ``FaceOffsetSymmetricReg(vertex_num, face_vertex_idx, closest_faces, bc)`` -- reference ``loss.py:151-167`` without the
  ``smpl_x`` global: ``forward(face_offset [B, Vf, 3])`` returns ``[B, Vf]``.  ``flip_symmetry_plan`` compacts the problem
  once on the host to the Vf rows that are ever read: no ``[B, 10475, 3]`` padding, no table copies per call.
* ``PoseLoss()`` -- reference ``loss.py:73-87``: ``forward(pose_out, pose_gt)`` takes ``[B, 3J]`` or ``[B, J, 3]`` and returns
  ``[B, J, 3, 3]``, ``|axis_angle_to_matrix(out) - axis_angle_to_matrix(gt)|`` by pytorch3d's quaternion route, the device
  functions the forward kinematics use (``csrc/axis_angle.h``), one thread per rotation.
* ``centered_v2v_loss(out, target, weight, scale=10.0)`` -- ``model.py:235-237``:
  ``|(a - mean_v a) - (t - mean_v t)| * weight * scale`` as ``[B, V, 3]``.

The kernels are ``csrc/fit_terms.hip`` behind ``include/exa_mesh.h`` (``exa_mesh_edge_length_*``, ``exa_mesh_flip_symmetry_*``,
``exa_mesh_pose_loss_*``, ``exa_mesh_centered_v2v_*``), which writes out every operation and the order of every sum; ROCm
float32 tensors only, no CPU path.  The CPU restatement that pins them is ``tests/fit_oracle.py``.

Each backward gathers: every vertex (face row) sums the slots that name it from a transposed table in CSR form, built once
per module on the host (``exa_mesh_vertex_faces``; the plan's own transpose), in ascending order -- no atomics, no memset
and a summation order the header states, so the same inputs give the same bits on every call, where the order of the
reference's ``index_put_(accumulate=True)`` is PyTorch's own business.  The centred term's means and the mean in its
gradient are fixed two-level sums (``csrc/fixed_sum.h``) whose partials live in a workspace.

One deliberate deviation: **an edge whose predicted length is exactly 0 contributes a gradient of exactly 0**.  The
reference's ``sqrt`` backward divides 0 by 0 there and returns NaN for both end points (and a face that repeats a vertex
always has such an edge).  Everywhere else ``sign(0) = 0``, as in torch.

``coord_gt``, ``valid``, ``pose_gt``, ``target`` and ``weight`` are data in the reference and get no gradient.  Every term is
one launch each way (the centred term two), on the current stream, with outputs from the torch allocator and neither
allocation nor synchronisation inside the library, so forward and backward can be captured into a hipGraph.
"""
import collections

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._device import (_ptr, _workspace, check_devices, check_no_grad, check_rows, check_shape, check_tensor, grad_in,
                      launch)
from ._tables import face_tables, follow, host_i32, host_ptr

ROWS = 256                # EXA_MESH_FIT_ROWS


# ---- EdgeLengthLoss ----------------------------------------------------------------------------------------------------
class _EdgeLength(torch.autograd.Function):
    """coord_out [B, V, 3], coord_gt [Bt, V, 3], valid [Bv, V] (contiguous float32), faces [F, 3], the CSR (int32) ->
    [B, 3F, 1]."""

    @staticmethod
    def forward(ctx, out, gt, valid, faces, offsets, entries):
        B, V, F = out.shape[0], out.shape[1], faces.shape[0]
        loss = torch.empty((B, 3 * F, 1), dtype=torch.float32, device=out.device)
        ctx.sizes = (B, gt.shape[0], valid.shape[0], V, F)
        ctx.save_for_backward(out, gt, valid, faces, offsets, entries)
        launch(_lib.MESH, 'exa_mesh_edge_length_forward', out.device, *ctx.sizes, _ptr(out), _ptr(gt), _ptr(valid),
               _ptr(faces), _ptr(loss))
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        if grad_loss is None or not ctx.needs_input_grad[0]:
            return (None,) * 6
        out, gt, valid, faces, offsets, entries = ctx.saved_tensors
        dout = torch.empty_like(out)
        launch(_lib.MESH, 'exa_mesh_edge_length_backward', out.device, *ctx.sizes, _ptr(out), _ptr(gt), _ptr(valid),
               _ptr(faces), _ptr(offsets), _ptr(entries), _ptr(grad_in(grad_loss)), _ptr(dout))
        return (dout,) + (None,) * 5


class EdgeLengthLoss(nn.Module):
    """Drop-in for the reference's ``EdgeLengthLoss`` (``loss.py:125-149``): same constructor, same
    ``forward(coord_out, coord_gt, valid)`` and ``[B, 3F, 1]`` result.  ``face`` is an integer ``[F, 3]`` array or tensor;
    an index outside ``[0, V)`` is refused before any GPU work, a face that repeats a vertex is legal (that edge has length
    0).  An edge of predicted length exactly 0 gets a zero gradient where the reference returns NaN (module docstring).
    The int32 tables (``faces`` and the vertex -> (face, corner) CSR) are built on first use per vertex count and device."""

    def __init__(self, face):
        super(EdgeLengthLoss, self).__init__()
        self.face = face
        self._faces = host_i32('EdgeLengthLoss', 'face', face, (None, 3))
        self._tables = {}     # (V, device) -> (faces, CSR offsets, CSR entries) on the device

    def _device_tables(self, V, device):
        hit = self._tables.get((V, device))
        if hit is None:
            hit = self._tables[(V, device)] = face_tables(self._faces, V, device)
        return hit

    def forward(self, coord_out, coord_gt, valid):
        what = 'EdgeLengthLoss'
        check_shape(what, 'coord_out', coord_out, (None, None, 3), '[B, V, 3]')
        B, V = coord_out.shape[:2]
        check_shape(what, 'coord_gt', coord_gt, (B, V, 3), '[%d, %d, 3] or [1, %d, 3]' % (B, V, V), shared=True)
        check_tensor(what, 'valid', valid)
        if tuple(valid.shape) not in ((V,), (1, V, 1), (B, V, 1)):
            raise ValueError('%s: valid must be [%d], [1, %d, 1] or [%d, %d, 1] (it is %s)' % (what, V, V, B, V, tuple(valid.shape)))
        check_no_grad(what, 'coord_gt', coord_gt)
        check_no_grad(what, 'valid', valid)
        check_devices(what, 'coord_out', coord_out, coord_gt=coord_gt, valid=valid)
        tables = self._device_tables(V, coord_out.device)
        return _EdgeLength.apply(coord_out.contiguous(), coord_gt.contiguous(), valid.reshape(B if valid.dim() == 3 and valid.shape[0] == B else 1, V).contiguous(), *tables)


# ---- FaceOffsetSymmetricReg --------------------------------------------------------------------------------------------
FlipSymmetryPlan = collections.namedtuple('FlipSymmetryPlan', ['vertex_row', 'taps', 'weights', 'offsets', 'entries'])


def flip_symmetry_plan(vertex_num, face_vertex_idx, closest_faces, bc):
    """The flip-symmetry problem compacted to the Vf rows that are ever read, as CPU tensors: ``vertex_row`` ``[V_full]``
    (the face row of every vertex, -1 elsewhere), ``taps`` ``[Vf, 3]`` int32 in ``[-1, Vf)`` (the face row of
    ``closest_faces[face_vertex_idx[i], k]``, -1 where that vertex carries no offset and reads as zero), ``weights``
    ``[Vf, 3]`` (``bc`` of the same rows) and the taps' transpose as a CSR, ``offsets`` ``[Vf + 1]`` and ``entries`` (value
    ``3 * row + slot``, ascending).  ``closest_faces`` ``[vertex_num, 3]`` and ``bc`` ``[vertex_num, 3]`` are the reference's
    ``smpl_x.flip_corr``.  An index outside ``[0, vertex_num)`` and a vertex named twice in ``face_vertex_idx`` (the
    reference's indexed assignment is order-dependent there) are refused by the library."""
    what = 'flip_symmetry_plan'
    if isinstance(vertex_num, bool) or not isinstance(vertex_num, (int, np.integer)) or vertex_num < 0:
        raise ValueError('%s: vertex_num must be an integer >= 0 (it is %r)' % (what, vertex_num))
    V = int(vertex_num)
    fvi = host_i32(what, 'face_vertex_idx', face_vertex_idx, (None,))
    cf = host_i32(what, 'closest_faces', closest_faces, (V, 3))
    w = bc.detach().cpu().numpy() if isinstance(bc, torch.Tensor) else np.asarray(bc)
    if w.shape != (V, 3) or w.dtype.kind != 'f':
        raise ValueError('%s: bc must be a floating [%d, 3] array (it is %s %s)' % (what, V, w.dtype, w.shape))
    w = np.ascontiguousarray(w, dtype=np.float32)
    Vf, row = fvi.shape[0], np.zeros(V, dtype=np.int32)
    taps, weights = np.zeros((Vf, 3), dtype=np.int32), np.zeros((Vf, 3), dtype=np.float32)
    offsets, entries = np.zeros(Vf + 1, dtype=np.int32), np.zeros(max(3 * Vf, 1), dtype=np.int32)
    _lib.MESH.check(_lib.load().exa_mesh_flip_symmetry_plan(V, Vf, *(host_ptr(a) for a in (fvi, cf, w, row, taps, weights,
                                                                                           offsets, entries))))
    return FlipSymmetryPlan(*(torch.from_numpy(a) for a in (row, taps, weights, offsets, entries[:max(int(offsets[Vf]), 1)])))


class _FlipSymmetry(torch.autograd.Function):
    """face_offset [B, Vf, 3] (contiguous float32), taps, weights [Vf, 3], the CSR -> [B, Vf]."""

    @staticmethod
    def forward(ctx, p, taps, weights, offsets, entries):
        B, Vf = p.shape[:2]
        loss = torch.empty((B, Vf), dtype=torch.float32, device=p.device)
        ctx.save_for_backward(p, taps, weights, offsets, entries)
        launch(_lib.MESH, 'exa_mesh_flip_symmetry_forward', p.device, B, Vf, _ptr(p), _ptr(taps), _ptr(weights), _ptr(loss))
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        if grad_loss is None or not ctx.needs_input_grad[0]:
            return (None,) * 5
        p, taps, weights, offsets, entries = ctx.saved_tensors
        dp = torch.empty_like(p)
        launch(_lib.MESH, 'exa_mesh_flip_symmetry_backward', p.device, p.shape[0], p.shape[1], _ptr(p), _ptr(taps),
               _ptr(weights), _ptr(offsets), _ptr(entries), _ptr(grad_in(grad_loss)), _ptr(dp))
        return (dp,) + (None,) * 4


class FaceOffsetSymmetricReg(nn.Module):
    """Drop-in for the reference's ``FaceOffsetSymmetricReg`` (``loss.py:151-167``): ``forward(face_offset)`` ->
    ``[B, Vf]``.  The data the reference reads from its ``smpl_x`` global are constructor arguments: ``vertex_num``,
    ``face_vertex_idx`` ``[Vf]``, and ``flip_corr``'s ``closest_faces`` and ``bc`` (both ``[vertex_num, 3]``).  The plan
    (``flip_symmetry_plan``) is built once, here; its arrays are non-persistent buffers (``state_dict`` stays empty;
    ``.to(device)`` moves them, and a module that was never moved follows its input)."""

    PLAN = ('taps', 'weights', 'tap_offsets', 'tap_entries')

    def __init__(self, vertex_num, face_vertex_idx, closest_faces, bc):
        super(FaceOffsetSymmetricReg, self).__init__()
        plan = flip_symmetry_plan(vertex_num, face_vertex_idx, closest_faces, bc)
        self.face_vertex_num = plan.taps.shape[0]
        for name, t in zip(self.PLAN, plan[1:]):
            self.register_buffer(name, t, persistent=False)

    def forward(self, face_offset):
        what = 'FaceOffsetSymmetricReg'
        Vf = self.face_vertex_num
        check_shape(what, 'face_offset', face_offset, (None, Vf, 3), '[B, Vf, 3] with Vf = %d' % Vf)
        check_devices(what, 'face_offset', face_offset)
        follow(self, self.PLAN, face_offset.device)
        return _FlipSymmetry.apply(face_offset.contiguous(), self.taps, self.weights, self.tap_offsets, self.tap_entries)


# ---- PoseLoss ------------------------------------------------------------------------------------------------------------
class _PoseLoss(torch.autograd.Function):
    """pose_out, pose_gt [N, 3] (contiguous float32) -> [N, 9]."""

    @staticmethod
    def forward(ctx, out, gt):
        loss = torch.empty((out.shape[0], 9), dtype=torch.float32, device=out.device)
        ctx.save_for_backward(out, gt)
        launch(_lib.MESH, 'exa_mesh_pose_loss_forward', out.device, out.shape[0], _ptr(out), _ptr(gt), _ptr(loss))
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        if grad_loss is None or not ctx.needs_input_grad[0]:
            return None, None
        out, gt = ctx.saved_tensors
        dout = torch.empty_like(out)
        launch(_lib.MESH, 'exa_mesh_pose_loss_backward', out.device, out.shape[0], _ptr(out), _ptr(gt),
               _ptr(grad_in(grad_loss)), _ptr(dout))
        return dout, None


class PoseLoss(nn.Module):
    """Drop-in for the reference's ``PoseLoss`` (``loss.py:73-87``): ``forward(pose_out, pose_gt)`` with ``[B, 3J]`` or
    ``[B, J, 3]`` axis-angle inputs (each in either layout) returns ``[B, J, 3, 3]``.  The conventions are those of the
    forward kinematics' step 1: the small-angle branch below ``1e-6`` and ``d angle / d x := 0`` at a zero row.  The gradient
    goes to ``pose_out`` only."""

    def forward(self, pose_out, pose_gt):
        what = 'PoseLoss'
        for name, x in (('pose_out', pose_out), ('pose_gt', pose_gt)):
            check_tensor(what, name, x)
            if not ((x.dim() == 2 and x.shape[1] % 3 == 0) or (x.dim() == 3 and x.shape[2] == 3)):
                raise ValueError('%s: %s must be [B, 3J] or [B, J, 3] (it is %s)' % (what, name, tuple(x.shape)))
        B, J = pose_out.shape[0], pose_out.shape[1] // 3 if pose_out.dim() == 2 else pose_out.shape[1]
        if pose_gt.shape[0] != B or pose_gt.numel() != pose_out.numel():
            raise ValueError('%s: pose_gt must hold the rotations of pose_out, %s (it is %s)'
                             % (what, tuple(pose_out.shape), tuple(pose_gt.shape)))
        check_no_grad(what, 'pose_gt', pose_gt)
        check_devices(what, 'pose_out', pose_out, pose_gt=pose_gt)
        loss = _PoseLoss.apply(pose_out.reshape(-1, 3).contiguous(), pose_gt.reshape(-1, 3).contiguous())
        return loss.view(B, J, 3, 3)


# ---- the centred vertex-to-vertex term -----------------------------------------------------------------------------------
class _CenteredV2V(torch.autograd.Function):
    """out, target [B, V, 3], weight [V] (contiguous float32), scale -> [B, V, 3]."""

    @staticmethod
    def forward(ctx, out, target, weight, scale):
        B, V = out.shape[:2]
        dev = out.device
        loss = torch.empty_like(out)
        means = torch.empty((B, 6), dtype=torch.float32, device=dev)
        ctx.scale = scale
        ctx.save_for_backward(out, target, weight, means)
        if B * V:
            blocks = int(_lib.load().exa_mesh_centered_v2v_blocks(V))
            partials = _workspace(4 * B * 6 * blocks, dev)
            launch(_lib.MESH, 'exa_mesh_centered_v2v_forward', dev, B, V, _ptr(out), _ptr(target), _ptr(weight), scale,
                   _ptr(partials), _ptr(means), _ptr(loss))
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        if grad_loss is None or not ctx.needs_input_grad[0]:
            return (None,) * 4
        out, target, weight, means = ctx.saved_tensors
        B, V = out.shape[:2]
        dout = torch.empty_like(out)
        if B * V:
            blocks = int(_lib.load().exa_mesh_centered_v2v_blocks(V))
            partials = _workspace(4 * B * 3 * blocks, out.device)
            launch(_lib.MESH, 'exa_mesh_centered_v2v_backward', out.device, B, V, _ptr(out), _ptr(target), _ptr(weight),
                   ctx.scale, _ptr(means), _ptr(grad_in(grad_loss)), _ptr(partials), _ptr(dout))
        return (dout,) + (None,) * 3


def centered_v2v_loss(out, target, weight, scale=10.0):
    """``|(out - out.mean(1)[:, None]) - (target - target.mean(1)[:, None])| * weight * scale`` (``model.py:235-237``) as
    ``[B, V, 3]``, with a gradient to ``out``.  ``out``, ``target``: ``[B, V, 3]``; ``weight``: ``[V]``, ``[V, 1]`` or
    ``[1, V, 1]`` (the reference's ``is_not_neck``); ``scale`` a Python number that travels by value.  The means, and the
    mean over vertices in the gradient, are two-level sums in the header's order, divided by ``float(V)``."""
    what = 'centered_v2v_loss'
    check_shape(what, 'out', out, (None, None, 3), '[B, V, 3]')
    B, V = out.shape[:2]
    check_shape(what, 'target', target, (B, V, 3), '[%d, %d, 3], the shape of out' % (B, V))
    weight_rows = check_rows(what, 'weight', weight, V)
    if isinstance(scale, (bool, torch.Tensor)) or not isinstance(scale, (int, float, np.floating, np.integer)):
        raise ValueError('%s: scale must be a Python number (it is %r)' % (what, type(scale).__name__))
    check_no_grad(what, 'target', target)
    check_devices(what, 'out', out, target=target, weight=weight)
    return _CenteredV2V.apply(out.contiguous(), target.contiguous(), weight_rows, float(scale))
