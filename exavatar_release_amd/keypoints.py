"""HIP keypoints of the fitting: the landmark and extra-joint tail of the SMPL-X / FLAME layer, the camera tail of
``get_smplx_coord`` / ``get_flame_coord`` and ``CoordLoss``.

* ``BodyKeypoints`` -- the layer's full ``joints`` list (reference ``smplx/body_models.py:1257-1283``: the skeleton joints,
  the extra vertices of ``vertex_joint_selector``, the static landmarks, the dynamic contour landmarks of
  ``find_dynamic_lmk_idx_and_bcoords``, ``lbs.py:30-153``), a selection ``kpt_idx`` of its rows, and the tail of
  ``Model.get_smplx_coord`` / ``get_flame_coord`` (``fitting/main/model.py:97-117, 140-157``): root-relative camera
  coordinates, ``+ trans``, the pinhole projection and the optional ``root_rel`` subtraction.
  ``forward(vertices, joints, rot=None, trans=None, focal=None, princpt=None, root_rel=False, want_mesh=True)`` returns
  ``KeypointOutput(kpt_cam [B, K, 3], root_cam [B, 3], kpt_proj [B, K, 2] or None, mesh_cam [B, V, 3] or None,
  yaw_bin [B] int32)``.  ``vertices``, ``joints`` and ``rot`` are what ``PosedBody`` returns, stacked over the batch, or the
  torch layer's.  One launch forward (two with ``mesh_cam``), two backward (three with a cotangent for ``mesh_cam``).
* ``CoordLoss(lhand_idx, rhand_idx, lwrist_idx, rwrist_idx)`` -- the reference's class (``fitting/common/nets/loss.py:9-71``)
  without its ``smpl_x`` global: ``forward(kpt_proj, kpt_proj_gt, kpt_valid, kpt_cam, weight=None)`` returns ``[B, K, 2]``.
  The per-item Python loop with its read-backs is one launch of one wave per item; ``weight`` is the caller's ``* weight``
  (``model.py:213``) folded in.  ``kpt_valid >= 0`` is assumed (the data loaders produce 0 / 1); an item in which a hand has
  no entry ``> 0`` is skipped, where the reference would raise.

The kernels are ``csrc/keypoints.hip`` behind ``include/exa_mesh.h`` (``exa_mesh_keypoints_*``, ``exa_mesh_coord_loss_*``),
which writes out every operation and the order of every sum; ROCm float32 tensors only, no CPU path.  The CPU restatement
that pins them is ``tests/kpt_oracle.py``.  A landmark row is ``fmaf(v2, w2, fmaf(v1, w1, v0 * w0))`` over its face's corners: the order
``torch.einsum`` takes on the device, so that the rows equal the reference's there bit for bit (the stage's only fused
operations; everything else is rounded operation by operation).

All tables are data: built and validated once on the host (every vertex index in ``[0, V)``, every face id in ``[0, F)``,
every chain joint in ``[0, J)``, ``kpt_idx`` and ``root_idx`` in range -- an out-of-range index cannot reach the device) and
held as non-persistent buffers, so ``state_dict`` is unchanged.  The selection is compiled into one source record per
keypoint (a joint, one vertex, three vertices with weights, or a dynamic slot) and, for the backward, into the records'
transpose: per touched vertex its entries ``(k, corner, bin or -1)`` in ascending order, and per joint the records naming it.
The backward gathers over those -- no atomics, no memset, sums in the header's order -- so the same inputs give the same
bits on every call.  ``rot`` takes no gradient (the reference's path ends in ``.to(long)``), nor does the camera data.
Outputs come from the torch allocator on the current stream with neither allocation nor synchronisation inside the
library, so forward and backward can be captured into a hipGraph.

``root_idx`` names a row of the full list (the layer's ``joints`` followed by ``append_vertices``), like the entries of
``kpt_idx``: the reference's ``kpt_cam[:, smpl_x.kpt['root_idx']]`` is row ``smpl_x.kpt['idx'][smpl_x.kpt['root_idx']]``.
"""
import collections

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._device import _ptr, _workspace, check_devices, check_no_grad, check_shape, check_tensor, grad_in, launch
from ._tables import Cache, follow, host_i32

ROWS = 256                # EXA_MESH_KPT_ROWS
BINS = 79                 # EXA_MESH_KPT_BINS
JOINT, VERTEX, STATIC, DYNAMIC = 0, 1, 2, 3      # EXA_MESH_KPT_*

KeypointOutput = collections.namedtuple('KeypointOutput', ['kpt_cam', 'root_cam', 'kpt_proj', 'mesh_cam', 'yaw_bin'])
KeypointTables = collections.namedtuple('KeypointTables', ['rec', 'rec_w', 'dyn_vtx', 'dyn_w', 'chain', 'vrow', 'voff',
                                                           'vent_k', 'vent_bin', 'vent_w', 'joff', 'jent'])


def _host_f32(what, name, x, shape):
    """A float table as a contiguous float32 numpy array of ``shape`` (None: any length); one that requires grad is refused."""
    check_no_grad(what, name, x, kind='a buffer')
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if a.dtype.kind != 'f' and a.size:
        raise ValueError('%s: %s must hold floats (it is %s)' % (what, name, a.dtype))
    if a.ndim != len(shape) or any(s is not None and a.shape[i] != s for i, s in enumerate(shape)):
        raise ValueError('%s: %s must be %s (it is %s)' % (
            what, name, '[' + ', '.join('n' if s is None else str(s) for s in shape) + ']', a.shape))
    return np.ascontiguousarray(a, dtype=np.float32)


def _in_range(what, name, a, n, of):
    if a.size and (a.min() < 0 or a.max() >= n):
        bad = a.reshape(-1)[np.flatnonzero((a.reshape(-1) < 0) | (a.reshape(-1) >= n))[0]]
        raise ValueError('%s: %s holds %d, outside [0, %d) (%s)' % (what, name, int(bad), n, of))


def _size(what, name, n):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
        raise ValueError('%s: %s must be an integer >= 0 (it is %r)' % (what, name, n))
    return int(n)


def keypoint_tables(num_vertices, num_joints, faces=None, extra_vertices=(), lmk_faces_idx=(), lmk_bary_coords=None,
                    dynamic_lmk_faces_idx=None, dynamic_lmk_bary_coords=None, neck_kin_chain=(), kpt_idx=None, root_idx=0,
                    append_vertices=()):
    """The host compile of one selection: ``(KeypointTables of numpy arrays, Ld, T, number of rows)``.  Every index is
    checked here; the arrays are what ``include/exa_mesh.h`` calls ``ExaMeshKeypoints`` (record K is the root)."""
    what = 'BodyKeypoints'
    V, J = _size(what, 'num_vertices', num_vertices), _size(what, 'num_joints', num_joints)
    extra = host_i32(what, 'extra_vertices', extra_vertices, (None,))
    append = host_i32(what, 'append_vertices', append_vertices, (None,))
    lmk_f = host_i32(what, 'lmk_faces_idx', lmk_faces_idx, (None,))
    Ls = lmk_f.shape[0]
    lmk_w = _host_f32(what, 'lmk_bary_coords', np.zeros((0, 3), np.float32) if lmk_bary_coords is None else lmk_bary_coords, (Ls, 3))
    chain = host_i32(what, 'neck_kin_chain', neck_kin_chain, (None,))
    if (dynamic_lmk_faces_idx is None) != (dynamic_lmk_bary_coords is None):
        raise ValueError('%s: dynamic_lmk_faces_idx and dynamic_lmk_bary_coords come together' % what)
    if dynamic_lmk_faces_idx is None:
        dyn_f, dyn_w = np.zeros((BINS, 0), np.int32), np.zeros((BINS, 0, 3), np.float32)
    else:
        a = dynamic_lmk_faces_idx
        rows = a.shape[0] if hasattr(a, 'shape') and len(a.shape) else len(a)
        if rows != BINS:
            raise ValueError('%s: dynamic_lmk_faces_idx must have %d rows, the yaw bins of the layer (it has %d)' % (what, BINS, rows))
        dyn_f = host_i32(what, 'dynamic_lmk_faces_idx', a, (BINS, None))
        dyn_w = _host_f32(what, 'dynamic_lmk_bary_coords', dynamic_lmk_bary_coords, (BINS, dyn_f.shape[1], 3))
    Ld = dyn_f.shape[1]
    if Ls or Ld:
        if faces is None:
            raise ValueError('%s: faces is required with landmarks' % what)
        faces = host_i32(what, 'faces', faces, (None, 3))
        F = faces.shape[0]
        _in_range(what, 'faces', faces, V, 'the vertices')
        _in_range(what, 'lmk_faces_idx', lmk_f, F, 'the faces')
        _in_range(what, 'dynamic_lmk_faces_idx', dyn_f, F, 'the faces')
    else:
        faces = np.zeros((0, 3), np.int32)
    _in_range(what, 'extra_vertices', extra, V, 'the vertices')
    _in_range(what, 'append_vertices', append, V, 'the vertices')
    _in_range(what, 'neck_kin_chain', chain, J, 'the joints')
    if Ld and not chain.size:
        raise ValueError('%s: neck_kin_chain is required with dynamic landmarks' % what)

    # every row of the full list as a record
    E, A = extra.shape[0], append.shape[0]
    R = J + E + Ls + Ld + A
    rec_all, w_all = np.zeros((R, 4), np.int32), np.zeros((R, 3), np.float32)
    o = 0
    rec_all[o:o + J, 0], rec_all[o:o + J, 1] = JOINT, np.arange(J)
    o += J
    rec_all[o:o + E, 0], rec_all[o:o + E, 1] = VERTEX, extra
    o += E
    rec_all[o:o + Ls, 0], rec_all[o:o + Ls, 1:], w_all[o:o + Ls] = STATIC, faces[lmk_f].reshape(Ls, 3), lmk_w
    o += Ls
    rec_all[o:o + Ld, 0], rec_all[o:o + Ld, 1] = DYNAMIC, np.arange(Ld)
    o += Ld
    rec_all[o:o + A, 0], rec_all[o:o + A, 1] = VERTEX, append
    idx = np.arange(R, dtype=np.int32) if kpt_idx is None else host_i32(what, 'kpt_idx', kpt_idx, (None,))
    _in_range(what, 'kpt_idx', idx, R, 'the rows: %d joints, %d extra vertices, %d static and %d dynamic landmarks, %d appended'
              % (J, E, Ls, Ld, A))
    root = _size(what, 'root_idx', root_idx)
    if root >= R:
        raise ValueError('%s: root_idx holds %d, outside [0, %d) (the rows)' % (what, root, R))
    sel = np.concatenate([idx, np.array([root], np.int32)])
    rec, rec_w = np.ascontiguousarray(rec_all[sel]), np.ascontiguousarray(w_all[sel])
    dyn_vtx = np.ascontiguousarray(faces[dyn_f].reshape(BINS, Ld, 3)) if Ld else np.zeros((BINS, 0, 3), np.int32)

    # the transpose: (vertex, k, corner, bin, weight) per entry, ascending (vertex, k, corner, bin)
    ks = np.arange(sel.shape[0], dtype=np.int64)
    parts = []
    m = rec[:, 0] == VERTEX
    parts.append((rec[m, 1], ks[m], np.zeros(m.sum(), np.int64), np.full(m.sum(), -1, np.int64), np.ones(m.sum(), np.float32)))
    m = rec[:, 0] == STATIC
    for c in range(3):
        parts.append((rec[m, 1 + c], ks[m], np.full(m.sum(), c, np.int64), np.full(m.sum(), -1, np.int64), rec_w[m, c]))
    m = rec[:, 0] == DYNAMIC
    if m.any():
        slot, n = rec[m, 1], int(m.sum())
        bins = np.repeat(np.arange(BINS, dtype=np.int64), n * 3)
        kk = np.tile(np.repeat(ks[m], 3), BINS)
        cc = np.tile(np.arange(3, dtype=np.int64), BINS * n)
        parts.append((dyn_vtx[:, slot, :].reshape(-1), kk, cc, bins, dyn_w[:, slot, :].reshape(-1)))
    ev, ek, ec, eb, ew = (np.concatenate([p[i] for p in parts]) for i in range(5))
    order = np.lexsort((eb, ec, ek, ev))
    ev, ek, eb, ew = ev[order], ek[order], eb[order], ew[order]
    touched, counts = np.unique(ev, return_counts=True)
    T = touched.shape[0]
    vrow = np.full(V, -1, np.int32)
    vrow[touched] = np.arange(T, dtype=np.int32)
    voff = np.zeros(T + 1, np.int32)
    voff[1:] = np.cumsum(counts)
    pad = lambda a, dt: np.ascontiguousarray(a if a.size else np.zeros(1, dt), dtype=dt)     # noqa: E731  (never NULL)
    m = rec[:, 0] == JOINT
    jorder = np.lexsort((ks[m], rec[m, 1]))
    joff = np.zeros(J + 1, np.int32)
    joff[1:] = np.cumsum(np.bincount(rec[m, 1], minlength=J))
    tables = KeypointTables(rec, rec_w, dyn_vtx, dyn_w, pad(chain, np.int32), vrow, voff, pad(ek, np.int32),
                            pad(eb, np.int32), pad(ew, np.float32), joff, pad(ks[m][jorder], np.int32))
    return tables, Ld, T, R


class _Keypoints(torch.autograd.Function):
    """vertices [B, V, 3], joints [B, J, 3], trans [B, 3] or None (contiguous float32), rot, focal, princpt (data), the two
    flags, the module -> kpt_cam, root_cam, kpt_proj or None, mesh_cam or None, yaw_bin."""

    @staticmethod
    def forward(ctx, vertices, joints, trans, rot, focal, princpt, root_rel, want_mesh, mod):
        dev, B, K = vertices.device, vertices.shape[0], mod.num_keypoints
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
        kpt_cam, root_cam = new(B, K, 3), new(B, 3)
        kpt_proj = new(B, K, 2) if focal is not None else None
        mesh_cam = new(B, mod.num_vertices, 3) if want_mesh else None
        yaw_bin = torch.empty((B,), dtype=torch.int32, device=dev)
        launch(_lib.MESH, 'exa_mesh_keypoints_forward', dev, mod._descriptor(dev), B, _ptr(vertices), _ptr(joints),
               _ptr(rot), _ptr(trans), _ptr(focal), _ptr(princpt), int(root_rel), _ptr(kpt_cam), _ptr(root_cam),
               _ptr(kpt_proj), _ptr(mesh_cam), _ptr(yaw_bin))
        ctx.mod, ctx.root_rel = mod, root_rel
        ctx.save_for_backward(vertices, joints, trans, focal, princpt, yaw_bin)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(yaw_bin)
        return kpt_cam, root_cam, kpt_proj, mesh_cam, yaw_bin

    @staticmethod
    def backward(ctx, g_cam, g_root, g_proj, g_mesh, _g_bin):
        if not any(ctx.needs_input_grad[:3]):
            return (None,) * 9
        vertices, joints, trans, focal, princpt, yaw_bin = ctx.saved_tensors
        mod, dev, B = ctx.mod, vertices.device, vertices.shape[0]
        d_vertices, d_joints = torch.empty_like(vertices), torch.empty_like(joints)
        d_trans = torch.empty_like(trans) if trans is not None else None
        nbytes = _lib.size_query(_lib.MESH, 'exa_mesh_keypoints_workspace_size', B, mod.num_vertices, mod.num_keypoints)
        ws = _workspace(max(nbytes, 1), dev)
        launch(_lib.MESH, 'exa_mesh_keypoints_backward', dev, mod._descriptor(dev), B, _ptr(vertices), _ptr(joints),
               _ptr(trans), _ptr(focal), _ptr(princpt), int(ctx.root_rel), _ptr(yaw_bin), _ptr(grad_in(g_cam)),
               _ptr(grad_in(g_proj)), _ptr(grad_in(g_root)), _ptr(grad_in(g_mesh)), _ptr(ws), ws.numel(), _ptr(d_vertices),
               _ptr(d_joints), _ptr(d_trans))
        need = ctx.needs_input_grad
        return (d_vertices if need[0] else None, d_joints if need[1] else None, d_trans if need[2] else None) + (None,) * 6


class BodyKeypoints(nn.Module):
    """The layer's ``joints`` list, a selection of it and the camera tail of ``get_smplx_coord`` (module docstring).

    The rows, in the layer's order: ``num_joints`` skeleton joints, ``extra_vertices`` (``extra_joints_idxs``), the static
    landmarks (``lmk_faces_idx [Ls]``, ``lmk_bary_coords [Ls, 3]`` over ``faces [F, 3]``), the dynamic contour landmarks
    (``dynamic_lmk_faces_idx [79, Ld]``, ``dynamic_lmk_bary_coords [79, Ld, 3]``; None without ``use_face_contour``; any other
    first extent than 79 is refused, the bin rule is written for 79 rows), then ``append_vertices`` (FLAME's ``lear`` /
    ``rear``, ``model.py:143-145``).  ``neck_kin_chain``: joint indices in the layer's own order, neck first.  ``kpt_idx``
    selects the K output rows (duplicates allowed; None: all rows), ``root_idx`` the root row."""

    TABLES = KeypointTables._fields

    def __init__(self, num_vertices, num_joints, faces=None, extra_vertices=(), lmk_faces_idx=(), lmk_bary_coords=None,
                 dynamic_lmk_faces_idx=None, dynamic_lmk_bary_coords=None, neck_kin_chain=(), kpt_idx=None, root_idx=0,
                 append_vertices=()):
        super(BodyKeypoints, self).__init__()
        tables, Ld, T, R = keypoint_tables(num_vertices, num_joints, faces, extra_vertices, lmk_faces_idx, lmk_bary_coords,
                                           dynamic_lmk_faces_idx, dynamic_lmk_bary_coords, neck_kin_chain, kpt_idx, root_idx,
                                           append_vertices)
        self.num_vertices, self.num_joints, self.num_rows = int(num_vertices), int(num_joints), R
        self.num_keypoints, self.num_dynamic, self.num_touched = tables.rec.shape[0] - 1, Ld, T
        self.chain_length = len(host_i32('BodyKeypoints', 'neck_kin_chain', neck_kin_chain, (None,)))
        for name, a in zip(self.TABLES, tables):
            self.register_buffer(name, torch.from_numpy(a), persistent=False)
        self._descriptors = Cache()

    @classmethod
    def from_layer(cls, layer, kpt_idx=None, root_idx=0, append_vertices=()):
        """The tables of a vendored ``SMPLX`` / ``FLAME`` layer (``smplx/body_models.py``): ``v_template``, ``J_regressor``,
        ``faces_tensor``, ``vertex_joint_selector.extra_joints_idxs``, ``lmk_faces_idx``, ``lmk_bary_coords`` and, with
        ``use_face_contour``, ``dynamic_lmk_faces_idx``, ``dynamic_lmk_bary_coords`` and ``neck_kin_chain``."""
        contour = bool(getattr(layer, 'use_face_contour', False))
        return cls(layer.v_template.shape[0], layer.J_regressor.shape[0], faces=layer.faces_tensor,
                   extra_vertices=layer.vertex_joint_selector.extra_joints_idxs, lmk_faces_idx=layer.lmk_faces_idx,
                   lmk_bary_coords=layer.lmk_bary_coords,
                   dynamic_lmk_faces_idx=layer.dynamic_lmk_faces_idx if contour else None,
                   dynamic_lmk_bary_coords=layer.dynamic_lmk_bary_coords if contour else None,
                   neck_kin_chain=layer.neck_kin_chain if contour else (), kpt_idx=kpt_idx, root_idx=root_idx,
                   append_vertices=append_vertices)

    def _descriptor(self, device):
        """``ExaMeshKeypoints`` over the buffers on ``device`` (built once per device and set of buffers)."""
        follow(self, self.TABLES, device)
        key = (device, self.rec.data_ptr())
        desc = self._descriptors.find(key)
        if desc is None:
            bufs = [getattr(self, n) for n in self.TABLES]
            desc = _lib.ExaMeshKeypoints(self.num_vertices, self.num_joints, self.num_keypoints, self.num_dynamic,
                                         self.chain_length, self.num_touched, *[b.data_ptr() or None for b in bufs])
            self._descriptors.keep(key, desc, *bufs)
        return desc

    def forward(self, vertices, joints, rot=None, trans=None, focal=None, princpt=None, root_rel=False, want_mesh=True):
        what = 'BodyKeypoints'
        V, J = self.num_vertices, self.num_joints
        check_shape(what, 'vertices', vertices, (None, V, 3), '[B, V, 3] with V = %d' % V)
        B = vertices.shape[0]
        check_shape(what, 'joints', joints, (B, J, 3), '[%d, %d, 3]' % (B, J))
        if self.num_dynamic and rot is None:
            raise ValueError('%s: rot is required with dynamic landmarks (Ld = %d)' % (what, self.num_dynamic))
        if rot is not None:
            check_shape(what, 'rot', rot, (B, J, 3, 3), '[%d, %d, 3, 3]' % (B, J))
        if trans is not None:
            check_shape(what, 'trans', trans, (B, 3), '[%d, 3]' % B)
        if (focal is None) != (princpt is None):
            raise ValueError('%s: focal and princpt come together' % what)
        if focal is not None:
            check_shape(what, 'focal', focal, (B, 2), '[%d, 2]' % B)
            check_shape(what, 'princpt', princpt, (B, 2), '[%d, 2]' % B)
            check_no_grad(what, 'focal', focal, kind='camera data')
            check_no_grad(what, 'princpt', princpt, kind='camera data')
        check_devices(what, 'vertices', vertices, joints=joints, rot=rot, trans=trans, focal=focal, princpt=princpt)
        c = lambda x: None if x is None else x.contiguous()      # noqa: E731
        return KeypointOutput(*_Keypoints.apply(vertices.contiguous(), joints.contiguous(), c(trans),
                                                c(rot.detach()) if rot is not None and self.num_dynamic else None,
                                                c(focal), c(princpt), bool(root_rel), bool(want_mesh), self))


# ---- CoordLoss -----------------------------------------------------------------------------------------------------------
class _CoordLoss(torch.autograd.Function):
    """kpt_proj, kpt_proj_gt [B, K, 2], kpt_valid [B, K], kpt_cam [B, K, 3], weight [B, K, 2] or None (contiguous float32),
    lhand, rhand, part (int32) -> loss [B, K, 2], hand_w [B, K]."""

    @staticmethod
    def forward(ctx, proj, gt, valid, cam, weight, lhand, rhand, part):
        B, K = proj.shape[:2]
        loss = torch.empty_like(proj)
        hand_w = torch.empty((B, K), dtype=torch.float32, device=proj.device)
        launch(_lib.MESH, 'exa_mesh_coord_loss_forward', proj.device, B, K, lhand.shape[0], rhand.shape[0], _ptr(lhand),
               _ptr(rhand), _ptr(part), _ptr(proj), _ptr(gt), _ptr(valid), _ptr(cam), _ptr(weight), _ptr(hand_w), _ptr(loss))
        ctx.save_for_backward(proj, gt, valid, weight, hand_w)
        ctx.mark_non_differentiable(hand_w)
        return loss, hand_w

    @staticmethod
    def backward(ctx, grad_loss, _g_hand_w):
        if grad_loss is None or not ctx.needs_input_grad[0]:
            return (None,) * 8
        proj, gt, valid, weight, hand_w = ctx.saved_tensors
        d_proj = torch.empty_like(proj)
        launch(_lib.MESH, 'exa_mesh_coord_loss_backward', proj.device, proj.shape[0], proj.shape[1], _ptr(proj), _ptr(gt),
               _ptr(valid), _ptr(weight), _ptr(hand_w), _ptr(grad_in(grad_loss)), _ptr(d_proj))
        return (d_proj,) + (None,) * 7


class CoordLoss(nn.Module):
    """Drop-in for the reference's ``CoordLoss`` (``loss.py:9-71``) with its ``smpl_x`` data as constructor arguments:
    ``lhand_idx`` / ``rhand_idx`` (``smpl_x.kpt['part_idx']['lhand' / 'rhand']``) and the two wrists' keypoint indices.
    ``forward(kpt_proj [B, K, 2], kpt_proj_gt [B, K, 2], kpt_valid [B, K, 1] or [B, K], kpt_cam [B, K, 3], weight=None)``
    returns ``[B, K, 2]``; ``weight [B, K, 2]`` multiplies the result in the kernel.  ``return_hand_w=True`` also returns
    the rule's ``[B, K]`` weights.  The gradient goes to ``kpt_proj`` only (the rule sits under ``no_grad``)."""

    def __init__(self, lhand_idx, rhand_idx, lwrist_idx, rwrist_idx):
        super(CoordLoss, self).__init__()
        what = 'CoordLoss'
        self._hands = (host_i32(what, 'lhand_idx', lhand_idx, (None,)), host_i32(what, 'rhand_idx', rhand_idx, (None,)))
        self._wrists = (_size(what, 'lwrist_idx', lwrist_idx), _size(what, 'rwrist_idx', rwrist_idx))
        for name, a in zip(('lhand_idx', 'rhand_idx'), self._hands):
            if not a.size:
                raise ValueError('%s: %s is empty' % (what, name))
            if a.min() < 0:
                raise ValueError('%s: %s holds %d, outside [0, K)' % (what, name, int(a.min())))
        self._tables = {}     # (K, device) -> (lhand, rhand, part) on the device

    def _device_tables(self, K, device):
        hit = self._tables.get((K, device))
        if hit is None:
            part = np.zeros(max(K, 1), np.int32)
            for bit, name, hand, wrist in ((1, 'l', self._hands[0], self._wrists[0]), (2, 'r', self._hands[1], self._wrists[1])):
                _in_range('CoordLoss', name + 'hand_idx', hand, K, 'the keypoints')
                _in_range('CoordLoss', name + 'wrist_idx', np.array([wrist]), K, 'the keypoints')
                part[hand] |= bit
                part[wrist] |= bit
            hit = self._tables[(K, device)] = tuple(torch.from_numpy(a).to(device) for a in self._hands + (part,))
        return hit

    def forward(self, kpt_proj, kpt_proj_gt, kpt_valid, kpt_cam, weight=None, return_hand_w=False):
        what = 'CoordLoss'
        check_shape(what, 'kpt_proj', kpt_proj, (None, None, 2), '[B, K, 2]')
        B, K = kpt_proj.shape[:2]
        check_shape(what, 'kpt_proj_gt', kpt_proj_gt, (B, K, 2), '[%d, %d, 2], the shape of kpt_proj' % (B, K))
        check_tensor(what, 'kpt_valid', kpt_valid)
        if tuple(kpt_valid.shape) not in ((B, K, 1), (B, K)):
            raise ValueError('%s: kpt_valid must be [%d, %d, 1] or [%d, %d] (it is %s)' % (what, B, K, B, K, tuple(kpt_valid.shape)))
        check_shape(what, 'kpt_cam', kpt_cam, (B, K, 3), '[%d, %d, 3]' % (B, K))
        if weight is not None:
            check_shape(what, 'weight', weight, (B, K, 2), '[%d, %d, 2], the shape of kpt_proj' % (B, K))
        for name, x in (('kpt_proj_gt', kpt_proj_gt), ('kpt_valid', kpt_valid), ('weight', weight)):
            check_no_grad(what, name, x)
        check_devices(what, 'kpt_proj', kpt_proj, kpt_proj_gt=kpt_proj_gt, kpt_valid=kpt_valid, kpt_cam=kpt_cam, weight=weight)
        tables = self._device_tables(K, kpt_proj.device) if K else (None, None, None)
        if not K:
            return (torch.empty_like(kpt_proj), kpt_proj.new_empty((B, 0))) if return_hand_w else torch.empty_like(kpt_proj)
        loss, hand_w = _CoordLoss.apply(kpt_proj.contiguous(), kpt_proj_gt.contiguous(), kpt_valid.reshape(B, K).contiguous(),
                                        kpt_cam.detach().contiguous(), None if weight is None else weight.contiguous(), *tables)
        return (loss, hand_w) if return_hand_w else loss
