"""HIP Gaussian offset and joint offset regularisers: the four terms of the training loss block that had no HIP form.

* ``OffsetRegs(mean_weight, scale_weight, joint_offset_ref, joint_weight, sym_pairs)`` -- reference
  ``avatar/main/model.py:217-232, 253-257``::

      loss['gaussian_mean_reg']    = (mean_offset ** 2 + mean_offset_offset ** 2) * weight
      loss['gaussian_scale_reg']   = (scale ** 2 + scale_offset ** 2) * weight
      loss['joint_offset_reg']     = (joint_offset - smpl_x.joint_offset.cuda()) ** 2 * weight
      loss['joint_offset_sym_reg'] = self.joint_offset_sym_reg(joint_offset)

  as ONE autograd node: two launches forward and one backward.  ``forward(mean_offset, mean_offset_offset, scale,
  scale_offset, joint_offset, reduce='mean')`` returns a dict with those four keys in that order: with ``reduce='mean'``
  four 0-dim views of one ``[4]`` tensor (each the term's ``.mean()``, ``train.py:43``), with ``reduce=None`` the four
  maps, each a drop-in for its expression.  In the warm-up pass the pre-clamp scale as ``scale`` (``scale_wo_clamp`` is a
  clone the reference makes only for this term).
* ``offset_regs(...)`` -- the functional form, the constants as arguments.
* ``JointOffsetSymmetricReg(joints_name)`` -- the reference's class (``loss.py:133-146``) without the ``smpl_x`` global:
  ``forward(joint_offset)`` returns the ``[n_pairs]`` map.  ``symmetric_joint_pairs(joints_name)`` builds the pairs once.
* ``loss_weights(is_rhand, is_lhand, is_face, is_face_expr, is_cavity, joint_part=None, joint_num=None)`` -- the
  per-vertex weights of ``model.py:217-247`` and the joint weight of ``model.py:253-255``, built once in plain torch
  (the reference rebuilds them every iteration with boolean-mask assignments, each a read-back of the mask).

The kernels are ``csrc/offset_regs.hip`` behind ``include/exa_mesh.h`` (``exa_mesh_offset_regs_*``), which writes out every
operation and the order of every sum; ROCm float32 tensors only, no CPU path.  The CPU restatement that pins them is
``tests/offset_oracle.py``.  The maps and every gradient equal the torch expressions bit for bit, except that the
gradient of a ``[B, V, 1]`` ``scale_offset`` adds its three channels as ``(c0 + c1) + c2`` where torch's device sum has an
order of its own.  The means are reproducible bit for bit and within ``(d + 2) * 2^-24`` of the exact mean, d the additions
an element passes through (``offset_oracle.mean_depth``).  The means' backward reads the four cotangents on the device and
scales by ``g * (1 / n)``, the rounded reciprocal first, as torch's backward of ``.mean()`` does on the device.

The weights, the reference offsets and the pairs are data and get no gradient.  A joint belongs to at most one pair
(checked when the pairs are built), so the backward gathers and needs no atomics.  An empty term (no vertices, no
pairs) gives an empty map or a NaN mean, as ``torch.mean`` of an empty tensor does, and zero gradients.  The calls
allocate their outputs with torch and neither allocate nor synchronise inside the library, so forward and backward can
be captured into a hipGraph.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._device import (_ptr, _ptrs, _workspace, check_devices, check_mask, check_no_grad, check_reduce, check_rows,
                      check_shape, check_tensor, grad_in, launch)
from ._tables import Cache, follow, host_i32, host_ptr

TERMS = ('gaussian_mean_reg', 'gaussian_scale_reg', 'joint_offset_reg', 'joint_offset_sym_reg')      # model.py's key order
ROWS = 256                # EXA_MESH_OFFSET_ROWS


# ---- the pairs ---------------------------------------------------------------------------------------------------------
def symmetric_joint_pairs(joints_name):
    """``(right, left)``: the indices of the ``'R_'`` joints in ascending order and of their ``'L_'`` partners, the two
    lists the reference's ``JointOffsetSymmetricReg.forward`` rebuilds on every call.  A missing partner raises
    ``ValueError``, as the reference's ``.index`` does."""
    names = list(joints_name)
    right = [j for j, n in enumerate(names) if n[:2] == 'R_']
    left = [names.index('L_' + names[j][2:]) for j in right]
    return right, left


def _pair_tables(sym_pairs, J, what):
    """(pair_r [P], pair_l [P], joint_pair [J]) int32 CPU tensors; the C ABI checks the indices and that no joint is named twice."""
    try:
        right, left = ([], []) if sym_pairs is None else sym_pairs
        right = [int(j) for j in (right.tolist() if isinstance(right, torch.Tensor) else right)]
        left = [int(j) for j in (left.tolist() if isinstance(left, torch.Tensor) else left)]
    except (TypeError, ValueError):
        raise ValueError('%s: sym_pairs must be (right indices, left indices), as symmetric_joint_pairs returns them' % what)
    if len(right) != len(left):
        raise ValueError('%s: sym_pairs must hold as many left as right joints (%d and %d)' % (what, len(right), len(left)))
    bad = [j for j in right + left if not 0 <= j < J]
    if bad:
        raise ValueError('%s: sym_pairs names joint %d outside [0, %d)' % (what, bad[0], J))
    if len(set(right + left)) != 2 * len(right):
        raise ValueError('%s: sym_pairs names a joint twice; a joint belongs to at most one pair' % what)
    r, l = host_i32(what, 'sym_pairs', right, (None,)), host_i32(what, 'sym_pairs', left, (None,))
    table = np.zeros(J, dtype=np.int32)
    _lib.MESH.check(_lib.load().exa_mesh_offset_regs_pair_table(J, len(right), host_ptr(r), host_ptr(l), host_ptr(table)))
    return torch.from_numpy(r), torch.from_numpy(l), torch.from_numpy(table)


_pair_cache = Cache()     # functional form: (right, left, J, device) -> the three device tables


def _device_pairs(sym_pairs, J, device, what):
    if isinstance(sym_pairs, tuple) and len(sym_pairs) == 3 and all(isinstance(t, torch.Tensor) for t in sym_pairs):
        return sym_pairs                                         # OffsetRegs' own buffers
    try:
        key = None if sym_pairs is None else (tuple(int(j) for j in sym_pairs[0]), tuple(int(j) for j in sym_pairs[1]))
    except (TypeError, ValueError, IndexError):
        raise ValueError('%s: sym_pairs must be (right indices, left indices), as symmetric_joint_pairs returns them' % what)
    key = (key, J, str(device))
    return _pair_cache.find(key) or _pair_cache.keep(key, tuple(t.to(device) for t in _pair_tables(key[0], J, what)))


# ---- the node ----------------------------------------------------------------------------------------------------------
class _OffsetRegs(torch.autograd.Function):
    """mean_offset, mean_offset_offset, scale [B, V, 3], scale_offset [B, V, 1 or 3], joint_offset [J, 3]; the constants
    w_mean, w_scale [V], joint_ref, w_joint [J, 3], pair_r, pair_l [P], joint_pair [J] (int32); all contiguous on one ROCm
    device; mean -> the four maps, or four 0-dim views of one [4] tensor."""

    @staticmethod
    def forward(ctx, mo, moo, sc, so, jo, w_mean, w_scale, jref, w_joint, pair_r, pair_l, joint_pair, mean):
        B, V, C, J, P = mo.shape[0], mo.shape[1], so.shape[2], jo.shape[0], pair_r.shape[0]
        dev = jo.device
        ctx.mean, ctx.sizes = mean, (B, V, C, J, P)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(mo, moo, sc, so, jo, w_mean, w_scale, jref, w_joint, pair_r, pair_l, joint_pair)
        vertex = (B, V, C, _ptr(mo), _ptr(moo), _ptr(sc), _ptr(so), _ptr(w_mean), _ptr(w_scale))
        joint = (B, V, J, P, _ptr(jo), _ptr(jref), _ptr(w_joint), _ptr(pair_r), _ptr(pair_l))
        if mean:
            blocks = int(_lib.load().exa_mesh_offset_regs_blocks(B, V))
            partials = _workspace(4 * max(2 * blocks, 1), dev)
            means = torch.empty(4, dtype=torch.float32, device=dev)
            launch(_lib.MESH, 'exa_mesh_offset_regs_vertex_forward', dev, *vertex, None, None, _ptr(partials))
            launch(_lib.MESH, 'exa_mesh_offset_regs_joint_forward', dev, *joint, None, None, _ptr(partials), _ptr(means))
            return means.unbind(0)
        f32 = dict(dtype=torch.float32, device=dev)
        mean_map, scale_map = torch.empty((B, V, 3), **f32), torch.empty((B, V, 3), **f32)
        joint_map, sym_map = torch.empty((J, 3), **f32), torch.empty((P,), **f32)
        if B * V:
            launch(_lib.MESH, 'exa_mesh_offset_regs_vertex_forward', dev, *vertex, _ptr(mean_map), _ptr(scale_map), None)
        if J:
            launch(_lib.MESH, 'exa_mesh_offset_regs_joint_forward', dev, *joint, _ptr(joint_map), _ptr(sym_map), None, None)
        return mean_map, scale_map, joint_map, sym_map

    @staticmethod
    def backward(ctx, *grads):
        mo, moo, sc, so, jo, w_mean, w_scale, jref, w_joint, pair_r, pair_l, joint_pair = ctx.saved_tensors
        B, V, C, J, P = ctx.sizes
        need = ctx.needs_input_grad
        shapes = ((B, V, 3), (B, V, 3), (J, 3), (P,))
        g = [grad_in(x) for x in grads]
        if not ctx.mean:
            g = [None if x is None else x.expand(shapes[k]).contiguous() for k, x in enumerate(g)]
        # the inputs a term reaches: a term without a cotangent leaves its inputs without a gradient, as autograd would
        reach = (g[0] is not None, g[0] is not None, g[1] is not None, g[1] is not None, g[2] is not None or g[3] is not None)
        inputs = (mo, moo, sc, so, jo)
        live = [x is not None and (ctx.mean or x.numel() > 0) for x in g]
        if not any(live):            # only cotangents of empty maps: nothing to read, the gradients are zeros
            return tuple(torch.zeros_like(x) if need[i] and reach[i] else None for i, x in enumerate(inputs)) + (None,) * 8
        outs = [torch.empty_like(x) if need[i] and reach[i] else None for i, x in enumerate(inputs)]
        if any(o is not None for o in outs):
            cot = _ptrs([x if ok else None for x, ok in zip(g, live)])
            launch(_lib.MESH, 'exa_mesh_offset_regs_backward', jo.device, B, V, C, J, P, _ptr(mo), _ptr(moo), _ptr(sc),
                   _ptr(so), _ptr(w_mean), _ptr(w_scale), _ptr(jo), _ptr(jref), _ptr(w_joint), _ptr(pair_r), _ptr(pair_l),
                   _ptr(joint_pair), None if ctx.mean else cot, cot if ctx.mean else None, *[_ptr(o) for o in outs])
        return tuple(outs) + (None,) * 8


# ---- argument checks: tensor, dtype, shape, then the device ------------------------------------------------------------
def offset_regs(mean_offset, mean_offset_offset, scale, scale_offset, joint_offset, mean_weight, scale_weight,
                joint_offset_ref, joint_weight, sym_pairs, reduce='mean'):
    """The four terms for a caller's own constants: a dict in ``TERMS`` order (module docstring).  ``mean_weight``,
    ``scale_weight``: ``[V]``, ``[V, 1]`` or ``[1, V, 1]``; ``joint_offset_ref``, ``joint_weight``: ``[J, 3]``; ``sym_pairs``:
    ``(right, left)`` index lists as ``symmetric_joint_pairs`` returns them (or None), whose device tables are cached per
    pair of lists and device.  Gradients go to whichever of the five inputs require them."""
    what = 'offset_regs'
    check_reduce(what, reduce)
    check_shape(what, 'mean_offset', mean_offset, (None, None, 3), '[B, V, 3]')
    B, V = mean_offset.shape[:2]
    like = '[%d, %d, 3], the shape of mean_offset' % (B, V)
    check_shape(what, 'mean_offset_offset', mean_offset_offset, (B, V, 3), like)
    check_shape(what, 'scale', scale, (B, V, 3), like)
    check_tensor(what, 'scale_offset', scale_offset)
    if scale_offset.dim() != 3 or tuple(scale_offset.shape[:2]) != (B, V) or scale_offset.shape[2] not in (1, 3):
        raise ValueError('%s: scale_offset must be [%d, %d, 1] or [%d, %d, 3] (it is %s)'
                         % (what, B, V, B, V, tuple(scale_offset.shape)))
    check_shape(what, 'joint_offset', joint_offset, (None, 3), '[J, 3]')
    J = joint_offset.shape[0]
    w_mean = check_rows(what, 'mean_weight', mean_weight, V)
    w_scale = check_rows(what, 'scale_weight', scale_weight, V)
    for name, x in (('joint_offset_ref', joint_offset_ref), ('joint_weight', joint_weight)):
        check_shape(what, name, x, (J, 3), '[J, 3] with J = %d' % J)
        check_no_grad(what, name, x)
    check_devices(what, 'joint_offset', joint_offset, mean_offset=mean_offset, mean_offset_offset=mean_offset_offset,
                   scale=scale, scale_offset=scale_offset, mean_weight=mean_weight, scale_weight=scale_weight,
                   joint_offset_ref=joint_offset_ref, joint_weight=joint_weight)
    pair_r, pair_l, joint_pair = _device_pairs(sym_pairs, J, joint_offset.device, what)
    if joint_pair.shape[0] != J or joint_pair.device != joint_offset.device:
        raise ValueError('%s: the pair tables are not for J = %d joints on the device of joint_offset' % (what, J))
    out = _OffsetRegs.apply(mean_offset.contiguous(), mean_offset_offset.contiguous(), scale.contiguous(),
                            scale_offset.contiguous(), joint_offset.contiguous(), w_mean, w_scale,
                            joint_offset_ref.contiguous(), joint_weight.contiguous(), pair_r, pair_l, joint_pair,
                            reduce == 'mean')
    return dict(zip(TERMS, out))


class OffsetRegs(nn.Module):
    """The four terms as a module that holds their constants (module docstring).  The constants are non-persistent buffers
    (``state_dict`` is unchanged; ``.to(device)`` moves them): ``mean_weight``, ``scale_weight`` as ``[V]`` rows,
    ``joint_offset_ref``, ``joint_weight`` ``[J, 3]``, and the int32 pair tables ``pair_right``, ``pair_left`` ``[n_pairs]``
    and ``joint_pair`` ``[J]``."""

    def __init__(self, mean_weight, scale_weight, joint_offset_ref, joint_weight, sym_pairs):
        super(OffsetRegs, self).__init__()
        what = 'OffsetRegs'
        check_tensor(what, 'mean_weight', mean_weight)
        V = mean_weight.numel()
        w_mean = check_rows(what, 'mean_weight', mean_weight, V)
        w_scale = check_rows(what, 'scale_weight', scale_weight, V)
        check_shape(what, 'joint_offset_ref', joint_offset_ref, (None, 3), '[J, 3]')
        J = joint_offset_ref.shape[0]
        check_shape(what, 'joint_weight', joint_weight, (J, 3), '[J, 3] with J = %d' % J)
        for name, x in (('joint_offset_ref', joint_offset_ref), ('joint_weight', joint_weight)):
            check_no_grad(what, name, x)
        dev = joint_offset_ref.device
        for name, x in (('mean_weight', mean_weight), ('scale_weight', scale_weight), ('joint_weight', joint_weight)):
            if x.device != dev:
                raise ValueError('%s: %s is not on the device of joint_offset_ref' % (what, name))
        tables = _pair_tables(sym_pairs, J, what)
        for name, x in zip(('mean_weight', 'scale_weight', 'joint_offset_ref', 'joint_weight', 'pair_right', 'pair_left',
                            'joint_pair'),
                           (w_mean, w_scale, joint_offset_ref.detach().contiguous(), joint_weight.detach().contiguous())
                           + tuple(t.to(dev) for t in tables)):
            self.register_buffer(name, x.detach(), persistent=False)

    def forward(self, mean_offset, mean_offset_offset, scale, scale_offset, joint_offset, reduce='mean'):
        return offset_regs(mean_offset, mean_offset_offset, scale, scale_offset, joint_offset, self.mean_weight,
                           self.scale_weight, self.joint_offset_ref, self.joint_weight,
                           (self.pair_right, self.pair_left, self.joint_pair), reduce)


class JointOffsetSymmetricReg(nn.Module):
    """Drop-in for the reference's ``JointOffsetSymmetricReg`` (``loss.py:133-146``): ``forward(joint_offset)`` ->
    ``[n_pairs]``, ``|x_R + x_L| + |y_R - y_L| + |z_R - z_L|`` per right / left pair.  ``joints_name`` (the reference's
    ``smpl_x.joints_name``) is a constructor argument; the pairs are built once, there."""

    def __init__(self, joints_name):
        super(JointOffsetSymmetricReg, self).__init__()
        self.joint_num = len(list(joints_name))
        self.sym_pairs = symmetric_joint_pairs(joints_name)
        for name, t in zip(('pair_right', 'pair_left', 'joint_pair'),
                           _pair_tables(self.sym_pairs, self.joint_num, 'JointOffsetSymmetricReg')):
            self.register_buffer(name, t, persistent=False)

    def forward(self, joint_offset):
        what = 'JointOffsetSymmetricReg'
        check_shape(what, 'joint_offset', joint_offset, (self.joint_num, 3), '[J, 3] with J = %d' % self.joint_num)
        check_devices(what, 'joint_offset', joint_offset)
        follow(self, ('joint_pair', 'pair_right', 'pair_left'), joint_offset.device)
        rows, none = joint_offset.new_empty((0, 0, 3)), joint_offset.new_empty((0,))
        unset = joint_offset.new_empty((self.joint_num, 3))     # term 2's constants: its map is computed and dropped
        return _OffsetRegs.apply(rows, rows, rows, rows, joint_offset.contiguous(), none, none, unset, unset,
                                 self.pair_right, self.pair_left, self.joint_pair, False)[3]


# ---- the constant weights of the block ---------------------------------------------------------------------------------
def loss_weights(is_rhand, is_lhand, is_face, is_face_expr, is_cavity, joint_part=None, joint_num=None):
    """The constant weights of the loss block, built once in plain torch on the masks' device: name -> ``[1, V, 1]`` float32
    for ``gaussian_mean_reg``, ``gaussian_scale_reg``, ``lap_mean``, ``lap_scale`` and ``lap_rgb`` (``model.py:217-247``, the
    reference's values in its assignment order, so a vertex in two masks gets the later one), and with ``joint_part`` (a
    mapping with ``'lhand'`` and ``'rhand'`` index lists, the reference's ``smpl_x.joint_part``) and ``joint_num`` also the
    ``[J, 3]`` weight of ``joint_offset_reg`` (``model.py:253-255``)."""
    what = 'loss_weights'
    masks = (('is_rhand', is_rhand), ('is_lhand', is_lhand), ('is_face', is_face), ('is_face_expr', is_face_expr),
             ('is_cavity', is_cavity))
    if not isinstance(is_rhand, torch.Tensor) or is_rhand.dim() != 1:
        raise ValueError('%s: is_rhand must be a bool [V] tensor' % what)
    V, dev = is_rhand.shape[0], is_rhand.device
    for name, m in masks:
        check_mask(what, name, m, V)
        if m.device != dev:
            raise ValueError('%s: %s is not on the device of is_rhand' % (what, name))
    r, l, f, fe, cav = (m for _, m in masks)
    ones = torch.ones((1, V, 1), dtype=torch.float32, device=dev)

    def make(base, *rules):
        w = ones * base
        for m, value in rules:
            w[:, m, :] = value
        return w
    out = {'gaussian_mean_reg': make(10, (r, 1000), (l, 1000), (f, 1), (fe, 10)),
           'gaussian_scale_reg': make(1, (r, 1000), (l, 1000), (fe, 10), (cav, 0)),
           'lap_mean': make(1, (fe, 50), (cav, 0.1)),
           'lap_scale': make(10, (r, 10), (l, 10), (fe, 0)),
           'lap_rgb': make(0.1, (r, 100), (l, 100))}
    if joint_part is not None:
        if isinstance(joint_num, bool) or not isinstance(joint_num, int) or joint_num < 0:
            raise ValueError('%s: joint_num must be given with joint_part, an integer >= 0 (it is %r)' % (what, joint_num))
        w = torch.ones((joint_num, 3), dtype=torch.float32, device=dev)
        for part in ('lhand', 'rhand'):
            idx = [int(j) for j in joint_part[part]]
            if any(not 0 <= j < joint_num for j in idx):
                raise ValueError('%s: joint_part[%r] names a joint outside [0, %d)' % (what, part, joint_num))
            w[idx, :] = 10
        out['joint_offset_reg'] = w
    return out
