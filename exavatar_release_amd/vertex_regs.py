"""HIP arm and hand regularisers: drop-ins for ExAvatar's ``ArmRGBReg``, ``HandRGBReg``, ``HandMeanReg`` and ``get_arm``.

* ``ArmRGBReg().forward(mesh_neutral_pose, is_upper_arm, is_lower_arm, rgb)`` -- reference ``loss.py:173-197``, called twice
  per iteration at ``model.py:251``: every lower-arm vertex is pulled towards the mean colour of its ``k`` nearest
  upper-arm vertices among those within ``dist_x_thr`` along x.  The functional form is
  ``plan = arm_neighbors(mesh_neutral_pose, is_upper_arm, is_lower_arm)`` once per iteration, then
  ``arm_rgb_loss(plan, rgb)`` per colour tensor.
* ``get_arm(mesh_neutral_pose, skinning_weight, face, arm_joint_idx, normal=None)`` -- reference ``smpl_x.py:139-148``.
* ``HandRGBReg().forward(rgb, is_rhand, is_lhand)`` -- reference ``loss.py:161-171``, twice per iteration at ``model.py:249``.
* ``HandMeanReg(face).forward(mesh_neutral_pose, offset, is_rhand, is_lhand, normal=None)`` -- reference ``loss.py:148-159``,
  twice per iteration at ``model.py:223``.

The kernels are ``csrc/vertex_regs.hip`` behind ``include/exa_mesh.h``, which states every operation and the order of
every sum; ROCm float32 tensors only, no CPU path.  The CPU restatement that pins them is ``tests/reg_oracle.py``.  No
kernel uses atomics, so the same inputs give the same bits on every call.

ArmRGBReg
---------
For a lower-arm vertex l and an upper-arm vertex u the pair is valid iff ``|x_l - x_u| < dist_x_thr``, compared in
float32 as torch compares a float32 tensor with the Python scalar ``0.01``.  Valid pairs are ordered by the key
``(d2, u)`` with ``d2 = (dx*dx + dy*dy) + dz*dz``, then the vertex index.  The reference orders by ``sqrt(d2)``; the square
root is monotone, so it only merges neighbouring distances into ties, which ``topk`` then breaks in an order of its own.
``n_l`` counts the valid u of l, ``k = min(top_k, min_l n_l)``, and the target of l is the mean of ``rgb`` over its ``k``
smallest keys, summed in key order from +0 and divided by ``float(k)``.  The reference's ``9999`` stand-in distance of an
invalid pair never wins, because ``k <= n_l`` for every l.  ``k`` stays on the device: nothing is read back.  With
``k == 0`` (a lower vertex without a valid partner, or no upper vertex) the target is ``0 / 0 = NaN`` -- the reference's
mean over an empty set -- and so is the loss; it is not trapped.  The target is detached and the mesh gets no gradient
(in the reference it reaches only the indices): ``grad rgb[b,l,c] = (2 d) g`` and exactly +0 on every other row.

``ArmRGBReg.forward`` returns ``[B, L, 3]`` like the reference: the dense ``[B, V, 3]`` result indexed with the mask, which
is the one host synchronisation the reference has too.  It keeps the plan of its last call and reuses it while the three
tensors are the same objects with the same ``_version`` and ``data_ptr``, so the second call of an iteration selects
nothing.  Where the reference raises for ``L == 0`` (``torch.min`` of an empty tensor), this returns an empty
``[B, 0, 3]``.

HandRGBReg / HandMeanReg
------------------------
The masks are constant buffers: their ascending index lists and inverse ranks are built once per pair of mask tensors and
device (one synchronisation, on first use) and cached as ``mesh_laplacian_loss`` caches its tables.  ``HandRGBReg`` raises
``ValueError`` for hands of different sizes, where the reference fails to broadcast.  Its means are the two-level sum of
the header (chunks of 256 rows), detached as in the reference.  ``HandMeanReg`` takes ``face`` in its constructor because
there is no ``smpl_x`` global here; its gradient is torch's for ``F.normalize`` and ``clamp(min=0)``, including at
equality, so a zero offset row gets the finite ``g * n * 1e12``.  ``normal`` (``vertex_normals(mesh, face)``, ``[V, 3]`` or
``[1, V, 3]``) lets one call per iteration serve ``get_arm`` and both ``HandMeanReg`` calls; it is data and gets no gradient.

Each call allocates its outputs from the torch allocator and launches on the current stream: the plan three kernels, the
arm loss one each way, ``HandRGBReg`` two forward and one backward, ``HandMeanReg`` one each way.  Once the hand tables are
cached nothing synchronises, so the calls can be captured into a hipGraph.
"""
import ctypes
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._device import _ptr, _workspace, check_devices, check_mask, check_no_grad, check_rows, check_shape, grad_in, launch
from ._tables import Cache, stamp

MAX_TOP_K = 64            # EXA_MESH_ARM_MAX_K
ARM_WAVES = 8             # EXA_MESH_ARM_WAVES
ARM_TILE = 1024           # EXA_MESH_ARM_TILE: upper records staged in LDS at a time
HEADER_INTS = 4           # EXA_MESH_ARM_HEADER_INTS
CHUNK = 256               # EXA_MESH_REG_CHUNK


# ---- argument checks: dtype and shape first, the device last, each a ValueError naming the argument -------------------
def _normal_rows(what, normal, V):
    return check_rows(what, 'normal', normal, V, ((V, 3), (1, V, 3)), '[V, 3] or [1, V, 3]')


def _normals_of(mesh, face):
    from .mesh import vertex_normals
    return vertex_normals(mesh.detach(), face)[0]


# ---- ArmRGBReg ---------------------------------------------------------------------------------------------------------
class ArmPlan:
    """The neighbour plan of one mesh (``arm_neighbors``): one workspace from the torch allocator, cut into sections whose
    tensors are views made on first use (building a plan costs the host one allocation and one C call).  ``count`` (L),
    ``upper_count`` (U), ``k`` and ``n_min`` are 0-dim int32 views of the device ``header``; ``nbr`` ``[rows, top_k]``
    holds, for the first L rows, the upper-arm vertices of the ``top_k`` smallest keys in key order (-1 where a row has
    fewer), ``n_valid`` ``[rows]`` their counts ``n_l`` and ``lower_rank`` ``[V]`` every vertex's row (-1 outside the lower
    arm); ``upper_rec`` / ``lower_rec`` ``[V, 4]`` are the record lists.  ``selection_launches`` counts how often this
    plan's selection ran (once); ``ArmPlan.total_selection_launches`` counts all plans'."""

    total_selection_launches = 0
    _SCALARS = {'upper_count': 0, 'count': 1, 'k': 2, 'n_min': 3}

    def __init__(self, V, rows, top_k, dist_x_thr, device):
        self.V, self.rows, self.top_k, self.dist_x_thr, self.device = V, rows, top_k, dist_x_thr, device
        i32, f32 = torch.int32, torch.float32
        layout = (('header', i32, (HEADER_INTS,)), ('upper_rec', f32, (V, 4)), ('lower_rec', f32, (V, 4)),
                  ('lower_rank', i32, (V,)), ('nbr', i32, (rows, top_k)), ('n_valid', i32, (rows,)),
                  ('wg_min', i32, ((rows + ARM_WAVES - 1) // ARM_WAVES,)))
        self._sections, off = {}, 0
        for name, dtype, shape in layout:
            n = 4
            for d in shape:
                n *= d
            self._sections[name] = (off, n, dtype, shape)
            off += (n + 255) & ~255                              # every section starts on a 256-byte boundary
        self._ws = _workspace(off, device)
        self._base = self._ws.data_ptr()
        self.selection_launches = 0

    def ptr(self, name):
        return ctypes.c_void_p(self._base + self._sections[name][0])

    def __getattr__(self, name):                                 # the sections and header scalars as tensors, on first use
        sections = self.__dict__.get('_sections')
        if sections is not None and name in sections:
            off, n, dtype, shape = sections[name]
            t = self._ws[off:off + n].view(dtype).reshape(shape)
        elif sections is not None and name in self._SCALARS:
            t = self.header[self._SCALARS[name]]
        else:
            raise AttributeError(name)
        setattr(self, name, t)
        return t


def arm_neighbors(mesh_neutral_pose, is_upper_arm, is_lower_arm, dist_x_thr=0.01, top_k=50, row_capacity=None):
    """The plan both ``arm_rgb_loss`` calls of an iteration share: build it once per ``mesh_neutral_pose``.  The mesh is
    ``[V, 3]`` float32 (it gets no gradient), the masks bool ``[V]`` on its device.  ``row_capacity`` is the caller's
    bound on the number of lower-arm vertices (default V, always safe): it sizes the selection's grid and lists, since
    the true L stays on the device; lower-arm vertices beyond it get NaN.  Three launches, no synchronisation."""
    what = 'arm_neighbors'
    check_shape(what, 'mesh_neutral_pose', mesh_neutral_pose, (None, 3), '[V, 3]')
    V = mesh_neutral_pose.shape[0]
    check_mask(what, 'is_upper_arm', is_upper_arm, V)
    check_mask(what, 'is_lower_arm', is_lower_arm, V)
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= MAX_TOP_K:
        raise ValueError('%s: top_k must be an integer 1 .. %d (it is %r)' % (what, MAX_TOP_K, top_k))
    thr = float(dist_x_thr)
    # the kernel compares in float32, as torch compares a float32 tensor with a Python scalar
    with np.errstate(over='ignore'):
        thr32 = float(np.float32(thr))
    if not math.isfinite(thr32) or not thr32 > 0:
        raise ValueError('%s: dist_x_thr must be finite and > 0 as a float32 (it is %r)' % (what, dist_x_thr))
    rows = V if row_capacity is None else int(row_capacity)
    if not 0 <= rows <= V:
        raise ValueError('%s: row_capacity must be 0 .. V = %d (it is %r)' % (what, V, row_capacity))
    check_devices(what, 'mesh_neutral_pose', mesh_neutral_pose, is_upper_arm=is_upper_arm, is_lower_arm=is_lower_arm)
    mesh = mesh_neutral_pose.detach().contiguous()
    up, lo = is_upper_arm.contiguous(), is_lower_arm.contiguous()
    plan = ArmPlan(V, rows, top_k, thr32, mesh.device)
    launch(_lib.MESH, 'exa_mesh_arm_plan', mesh.device, V, rows, top_k, thr32, _ptr(mesh), _ptr(up), _ptr(lo),
           plan.ptr('upper_rec'), plan.ptr('lower_rec'), plan.ptr('lower_rank'), plan.ptr('nbr'), plan.ptr('n_valid'),
           plan.ptr('wg_min'), plan.ptr('header'))
    plan.selection_launches += 1
    ArmPlan.total_selection_launches += 1
    return plan


class _ArmLoss(torch.autograd.Function):
    """rgb [B, V, 3] (float32, contiguous), plan -> (loss [B, V, 3], d [B, V, 3]); d is not differentiable."""

    @staticmethod
    def forward(ctx, rgb, plan):
        B, V = rgb.shape[0], rgb.shape[1]
        loss, d = torch.empty_like(rgb), torch.empty_like(rgb)
        launch(_lib.MESH, 'exa_mesh_arm_loss_forward', rgb.device, B, V, plan.rows, plan.top_k, _ptr(rgb),
               plan.ptr('lower_rank'), plan.ptr('nbr'), plan.ptr('header'), _ptr(loss), _ptr(d))
        ctx.save_for_backward(d)
        ctx.plan = plan                                          # keeps the workspace (the ranks the backward reads) alive
        ctx.mark_non_differentiable(d)
        return loss, d

    @staticmethod
    def backward(ctx, grad_loss, _grad_d):
        if grad_loss is None or not ctx.needs_input_grad[0]:
            return None, None
        d, = ctx.saved_tensors
        grad_loss = grad_in(grad_loss)
        gout = torch.empty_like(d)
        launch(_lib.MESH, 'exa_mesh_arm_loss_backward', d.device, d.shape[0], d.shape[1], _ptr(d), _ptr(grad_loss),
               ctx.plan.ptr('lower_rank'), _ptr(gout))
        return gout, None


def arm_rgb_loss(plan, rgb, return_d=False):
    """``ArmRGBReg`` for every vertex: ``[B, V, 3]``, the reference's loss on the lower-arm rows and +0 on every other row
    (which get a gradient of exactly +0).  ``dense.sum() / (3 * B * plan.count)`` is the trainer's ``.mean()`` without a
    synchronisation.  One launch each way.  With ``return_d`` also ``d = rgb - target`` (no gradient)."""
    what = 'arm_rgb_loss'
    if not isinstance(plan, ArmPlan):
        raise ValueError('%s: plan must be an ArmPlan (arm_neighbors)' % what)
    check_shape(what, 'rgb', rgb, (None, plan.V, 3), '[B, V, 3] with V = %d' % plan.V)
    if rgb.device != plan.device:
        raise ValueError('%s: rgb is not on the device of plan' % what)
    loss, d = _ArmLoss.apply(rgb.contiguous(), plan)
    return (loss, d) if return_d else loss


class ArmRGBReg(nn.Module):
    """Drop-in for the reference's ``ArmRGBReg`` (``loss.py:173-197``): same ``forward`` signature, ``[B, L, 3]`` result.
    ``dist_x_thr`` and ``top_k`` are the reference's constants.  ``plan`` is the plan of the last call."""

    def __init__(self, dist_x_thr=0.01, top_k=50):
        super(ArmRGBReg, self).__init__()
        self.dist_x_thr, self.top_k = dist_x_thr, top_k
        self.plan = None
        self._key = None     # (stamp of the three inputs and the two constants, the inputs themselves)

    def forward(self, mesh_neutral_pose, is_upper_arm, is_lower_arm, rgb):
        key = None
        if all(isinstance(t, torch.Tensor) for t in (mesh_neutral_pose, is_upper_arm, is_lower_arm)):
            key = stamp(mesh_neutral_pose, is_upper_arm, is_lower_arm) + (self.dist_x_thr, self.top_k)
        if self.plan is None or key is None or self._key is None or self._key[0] != key:
            self.plan = arm_neighbors(mesh_neutral_pose, is_upper_arm, is_lower_arm, self.dist_x_thr, self.top_k)
            self._key = (key, mesh_neutral_pose, is_upper_arm, is_lower_arm)
        return arm_rgb_loss(self.plan, rgb)[:, is_lower_arm, :]


def get_arm(mesh_neutral_pose, skinning_weight, face, arm_joint_idx, normal=None):
    """The reference's ``smpl_x.get_arm`` (``smpl_x.py:139-148``): ``(is_upper_arm, is_lower_arm)``, bool ``[V]``.  A vertex is
    on an arm when its largest skinning weight belongs to one of ``arm_joint_idx`` (the reference's R_Shoulder, R_Elbow,
    L_Shoulder, L_Elbow), on the upper side when its normal's y exceeds ``cos(pi / 3)``.  The normals are
    ``vertex_normals(mesh_neutral_pose, face)``, whose sums run in a fixed order, so the masks are the same bits on every
    call; pass ``normal`` to share one normals call with ``HandMeanReg``.  The reference compares float32 normals with the
    double ``math.cos(math.pi / 3) = 0.5000000000000001``; no float32 lies between 0.5 and that, so ``> 0.5f`` and
    ``<= 0.5f`` decide identically."""
    what = 'get_arm'
    check_shape(what, 'mesh_neutral_pose', mesh_neutral_pose, (None, 3), '[V, 3]')
    V = mesh_neutral_pose.shape[0]
    check_shape(what, 'skinning_weight', skinning_weight, (V, None), '[V, J] with V = %d' % V)
    check_no_grad(what, 'skinning_weight', skinning_weight, 'a buffer')
    joints = [int(j) for j in arm_joint_idx]
    if not joints or any(not 0 <= j < skinning_weight.shape[1] for j in joints):
        raise ValueError('%s: arm_joint_idx must name joints in [0, %d)' % (what, skinning_weight.shape[1]))
    if normal is not None:
        normal = _normal_rows(what, normal, V)
    check_devices(what, 'mesh_neutral_pose', mesh_neutral_pose, skinning_weight=skinning_weight, normal=normal)
    if normal is None:
        normal = _normals_of(mesh_neutral_pose, face)
    part_label = skinning_weight.argmax(1)
    is_arm = part_label == joints[0]
    for j in joints[1:]:
        is_arm = is_arm | (part_label == j)
    return is_arm & (normal[:, 1] > 0.5), is_arm & (normal[:, 1] <= 0.5)


# ---- the hands' index tables -------------------------------------------------------------------------------------------
def index_tables(mask):
    """(ascending indices of the set entries [n] int32, inverse ranks [V] int32: position in that list, -1 outside) of a
    bool ``[V]`` mask, on its device.  One synchronisation (the list's length)."""
    idx = torch.nonzero(mask).reshape(-1).to(torch.int32)
    rank = torch.full((mask.shape[0],), -1, dtype=torch.int32, device=mask.device)
    rank[idx.long()] = torch.arange(idx.shape[0], dtype=torch.int32, device=mask.device)
    return idx, rank


_hand_tables = Cache()     # stamp of the two masks -> {'r': tables, 'l': tables, 'h': tables of the union}


def _hands(is_rhand, is_lhand):
    key = stamp(is_rhand, is_lhand)
    return _hand_tables.find(key) or _hand_tables.keep(key, {'r': index_tables(is_rhand), 'l': index_tables(is_lhand),
                                                             'h': index_tables(is_rhand | is_lhand)}, is_rhand, is_lhand)


# ---- HandRGBReg --------------------------------------------------------------------------------------------------------
class _HandRgb(torch.autograd.Function):
    """rgb [B, V, 3] (float32, contiguous), the two hands' tables -> loss [B, N, 3]."""

    @staticmethod
    def forward(ctx, rgb, r_idx, l_idx, r_rank, l_rank):
        B, V, N = rgb.shape[0], rgb.shape[1], r_idx.shape[0]
        dev = rgb.device
        loss = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
        means = torch.empty((B, 2, 3), dtype=torch.float32, device=dev)
        nbytes = _lib.hand_rgb_workspace_size(B, N)
        ws = _workspace(nbytes, dev)
        launch(_lib.MESH, 'exa_mesh_hand_rgb_forward', dev, B, V, N, _ptr(rgb), _ptr(r_idx), _ptr(l_idx),
               _ptr(ws) if nbytes else None, nbytes, _ptr(means), _ptr(loss))
        ctx.save_for_backward(rgb, means, r_rank, l_rank)
        ctx.N = N
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        if grad_loss is None or not ctx.needs_input_grad[0]:
            return (None,) * 5
        rgb, means, r_rank, l_rank = ctx.saved_tensors
        grad_loss = grad_in(grad_loss)
        gout = torch.empty_like(rgb)
        launch(_lib.MESH, 'exa_mesh_hand_rgb_backward', rgb.device, rgb.shape[0], rgb.shape[1], ctx.N, _ptr(rgb),
               _ptr(means), _ptr(grad_loss), _ptr(r_rank), _ptr(l_rank), _ptr(gout))
        return (gout,) + (None,) * 4


class HandRGBReg(nn.Module):
    """Drop-in for the reference's ``HandRGBReg`` (``loss.py:161-171``): ``forward(rgb, is_rhand, is_lhand)`` -> ``[B, N, 3]``,
    row i the squared distance of the right hand's i-th vertex from the right hand's mean colour plus the same for the
    left hand.  A vertex in both masks sums its two gradient terms right hand first."""

    def forward(self, rgb, is_rhand, is_lhand):
        what = 'HandRGBReg'
        check_shape(what, 'rgb', rgb, (None, None, 3), '[B, V, 3]')
        V = rgb.shape[1]
        check_mask(what, 'is_rhand', is_rhand, V)
        check_mask(what, 'is_lhand', is_lhand, V)
        tables = _hands(is_rhand, is_lhand)
        (r_idx, r_rank), (l_idx, l_rank) = tables['r'], tables['l']
        if r_idx.shape[0] != l_idx.shape[0]:
            raise ValueError('%s: is_rhand and is_lhand must select equally many vertices (they select %d and %d)'
                             % (what, r_idx.shape[0], l_idx.shape[0]))
        check_devices(what, 'rgb', rgb, is_rhand=is_rhand, is_lhand=is_lhand)
        return _HandRgb.apply(rgb.contiguous(), r_idx, l_idx, r_rank, l_rank)


# ---- HandMeanReg -------------------------------------------------------------------------------------------------------
class _HandMean(torch.autograd.Function):
    """offset [B, V, 3], normal [V, 3] (float32, contiguous), the union's tables -> loss [B, H]."""

    @staticmethod
    def forward(ctx, offset, normal, h_idx, h_rank):
        B, V, H = offset.shape[0], offset.shape[1], h_idx.shape[0]
        loss = torch.empty((B, H), dtype=torch.float32, device=offset.device)
        launch(_lib.MESH, 'exa_mesh_hand_mean_forward', offset.device, B, V, H, _ptr(offset), _ptr(normal), _ptr(h_idx),
               _ptr(loss))
        ctx.save_for_backward(offset, normal, h_rank)
        ctx.H = H
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        if grad_loss is None or not ctx.needs_input_grad[0]:
            return (None,) * 4
        offset, normal, h_rank = ctx.saved_tensors
        grad_loss = grad_in(grad_loss)
        gout = torch.empty_like(offset)
        launch(_lib.MESH, 'exa_mesh_hand_mean_backward', offset.device, offset.shape[0], offset.shape[1], ctx.H,
               _ptr(offset), _ptr(normal), _ptr(grad_loss), _ptr(h_rank), _ptr(gout))
        return (gout,) + (None,) * 3


class HandMeanReg(nn.Module):
    """Drop-in for the reference's ``HandMeanReg`` (``loss.py:148-159``): ``forward(mesh_neutral_pose, offset, is_rhand,
    is_lhand)`` -> ``[B, H]`` over the union of the masks in ascending vertex order, the part of every hand vertex's
    normalised offset that points along its normal.  ``face`` (the upsampled mesh's, the reference's
    ``smpl_x.face_upsampled``) is a constructor argument; ``normal`` skips the normals call."""

    def __init__(self, face):
        super(HandMeanReg, self).__init__()
        self.face = face

    def forward(self, mesh_neutral_pose, offset, is_rhand, is_lhand, normal=None):
        what = 'HandMeanReg'
        check_shape(what, 'mesh_neutral_pose', mesh_neutral_pose, (None, 3), '[V, 3]')
        V = mesh_neutral_pose.shape[0]
        check_shape(what, 'offset', offset, (None, V, 3), '[B, V, 3] with V = %d' % V)
        check_mask(what, 'is_rhand', is_rhand, V)
        check_mask(what, 'is_lhand', is_lhand, V)
        if normal is not None:
            normal = _normal_rows(what, normal, V)
        check_devices(what, 'offset', offset, mesh_neutral_pose=mesh_neutral_pose, is_rhand=is_rhand, is_lhand=is_lhand,
                       normal=normal)
        if normal is None:
            normal = _normals_of(mesh_neutral_pose, self.face)
        h_idx, h_rank = _hands(is_rhand, is_lhand)['h']
        return _HandMean.apply(offset.contiguous(), normal, h_idx, h_rank)
