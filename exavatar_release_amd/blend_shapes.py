"""HIP blend-shape offsets: ExAvatar's pose correctives and expression offsets over compacted tables.

* ``BlendShapes(pose_dirs, expr_dirs, pose_mask)`` -- built once per model from the reference's buffers: ``pose_dirs``
  ``[Kp, 3 V]`` (after ``avatar/common/nets/module.py:305``), ``expr_dirs`` ``[V, 3, Ke]`` (after ``module.py:306``) and
  ``pose_mask`` ``[V]`` bool (``(is_rhand + is_lhand + is_face_expr) > 0``, ``module.py:489``).
  ``pose_offsets(pose_feat, mean_offset_offset)`` is ``module.py:485-493`` and returns the reference's
  ``(output, mean_offset_offset)`` pair; ``expr_offsets(expr)`` is ``module.py:537``.
* ``blend_offsets(coef, table, base=None)`` -- the functional form both use, for a caller's own ``BlendTable``.
* ``make_table(dirs, keep)`` -- the plan: a ``BlendTable`` from a full ``[K, M]`` matrix and the ``[M]`` bool of its
  columns that matter.

The kernels are ``csrc/blend_shapes.hip`` behind ``include/exa_mesh.h`` (``exa_mesh_blend_*``); ROCm float32 tensors only,
no CPU path, ``1 <= K <= 512``.  The CPU restatement that pins them is ``tests/blend_oracle.py``.

Why a plan
----------
Both reference expressions are ``out[j] = sum_k coef[k] * dirs[k, j]``.  The reference reads all of ``pose_dirs`` (976 MB
at V = 167 281) and then multiplies every vertex outside hands and face by zero; ``expr_dirs`` rows are zero away from
the face.  The constructor keeps only the columns that matter, in ascending order -- for the pose table the three
channels of every masked vertex, for the expression table the three channels of every vertex whose ``expr_dirs`` row has
a non-zero entry -- as a feature-major ``[K, N_pad]`` matrix (leading dimension padded to a multiple of 4 floats for
16-byte loads, pad columns zero) with two maps: compact column -> flat output index (``cols``) and its inverse (``inv``,
-1 where an output is not covered).  They are non-persistent buffers: ``.to()`` moves them and ``state_dict()`` stays
empty.  The full tables are not kept.

Semantics
---------
Covered outputs get the sum, in the order ``include/exa_mesh.h`` states (eight K-segments of ``ceil(K / 8)`` rows summed
sequentially, their partials added in ascending order; every operation rounded in fp32, no fused multiply-add -- an
order that depends on K alone).  Uncovered outputs get ``base`` (``+0.0`` without one), written by the same launch.
With a base the second result is ``+0.0`` where covered and ``base`` elsewhere.  PyTorch's ``matmul`` sums in an order of
its own and the reference's ``x * (1 - mask) + y * mask`` can give ``-0.0`` where this gives ``+0.0``: the results agree
within the bound derived in ``tests/blend_oracle.py``, zeros compare equal.

``pose_feat`` is detached as the reference detaches it; the tables are data.  ``dL/d base`` is ``g_out + g_masked`` where
uncovered and 0 where covered; ``dL/d coef`` is a fixed two-level sum (chunks of 1024 compact columns, each a fixed tree,
added in ascending order) -- no atomics, so the same inputs give the same bits on every call.

Each call allocates its outputs (backward: a workspace from the torch allocator) and launches one kernel forward, at
most two backward, on the current stream; nothing synchronises, so calls can be captured into a hipGraph.
"""
import collections

import torch
import torch.nn as nn

from . import _lib
from ._device import _ptr, _workspace, check_no_grad, check_tensor, grad_in, launch

MAX_K = 512          # EXA_MESH_BLEND_MAX_K
MAX_OUT = 1 << 30    # outputs per table

# table [K, ld] float32 (ld a multiple of 4, columns N .. ld-1 zero), cols [N] int32 ascending, inv [M] int32
BlendTable = collections.namedtuple('BlendTable', ['table', 'cols', 'inv'])


def make_table(dirs, keep):
    """The plan of a full matrix ``dirs`` [K, M] (float32) and ``keep`` [M] (bool): the kept columns in ascending order
    as a ``BlendTable`` on the device of ``dirs``."""
    what = 'make_table'
    if not isinstance(dirs, torch.Tensor) or not isinstance(keep, torch.Tensor):
        raise TypeError('%s: dirs and keep must be tensors' % what)
    check_no_grad(what, 'dirs', dirs)
    check_tensor(what, 'dirs', dirs)
    if dirs.dim() != 2 or not 1 <= dirs.shape[0] <= MAX_K or dirs.shape[1] > MAX_OUT:
        raise ValueError('%s: dirs must be [K, M] with 1 <= K <= %d and M <= 2^30 (it is %s)'
                         % (what, MAX_K, tuple(dirs.shape)))
    if keep.dtype != torch.bool or tuple(keep.shape) != (dirs.shape[1],):
        raise ValueError('%s: keep must be a bool tensor of shape [M] = [%d] (it is %s %s)'
                         % (what, dirs.shape[1], keep.dtype, tuple(keep.shape)))
    K, M = dirs.shape
    cols = torch.nonzero(keep.to(dirs.device), as_tuple=False).reshape(-1)          # ascending
    N = cols.numel()
    table = torch.zeros(K, (N + 3) // 4 * 4, dtype=torch.float32, device=dirs.device)
    table[:, :N] = dirs.index_select(1, cols)
    inv = torch.full((M,), -1, dtype=torch.int32, device=dirs.device)
    inv[cols] = torch.arange(N, dtype=torch.int32, device=dirs.device)
    return BlendTable(table, cols.to(torch.int32), inv)


class _Blend(torch.autograd.Function):
    """coef [K], base [M] or None, the plan -> (out [M], masked [M] or None)."""

    @staticmethod
    def forward(ctx, coef, base, table, cols, inv):
        K, ld = table.shape
        N, M = cols.shape[0], inv.shape[0]
        dev = coef.device
        out = torch.empty(M, dtype=torch.float32, device=dev)
        masked = torch.empty(M, dtype=torch.float32, device=dev) if base is not None else None
        launch(_lib.MESH, 'exa_mesh_blend_forward', dev, K, N, ld, M, _ptr(coef), _ptr(table) if N else None,
               _ptr(cols) if N else None, _ptr(inv), _ptr(base), _ptr(out), _ptr(masked))
        ctx.save_for_backward(table, cols, inv)
        if masked is None:
            return out
        return out, masked

    @staticmethod
    def backward(ctx, g_out, g_masked=None):
        want_coef, want_base = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_coef or want_base):
            return (None,) * 5
        table, cols, inv = ctx.saved_tensors
        K, ld = table.shape
        N, M = cols.shape[0], inv.shape[0]
        dev = table.device
        g_out, g_masked = grad_in(g_out), grad_in(g_masked)
        dcoef = torch.empty(K, dtype=torch.float32, device=dev) if want_coef else None
        dbase = torch.empty(M, dtype=torch.float32, device=dev) if want_base else None
        nbytes = _lib.blend_workspace_size(K, N) if want_coef else 0
        ws = _workspace(nbytes, dev) if nbytes else None
        launch(_lib.MESH, 'exa_mesh_blend_backward', dev, K, N, ld, M, _ptr(table) if N else None,
               _ptr(cols) if N else None, _ptr(inv), _ptr(g_out), _ptr(g_masked), _ptr(ws), nbytes, _ptr(dcoef), _ptr(dbase))
        return dcoef, dbase, None, None, None


def _check_table(table, what):
    if not isinstance(table, BlendTable) or not all(isinstance(t, torch.Tensor) for t in table):
        raise TypeError('%s: table must be a BlendTable of tensors (make_table builds one)' % what)
    t, cols, inv = table
    check_no_grad(what, 'table', t)
    if t.dtype != torch.float32 or cols.dtype != torch.int32 or inv.dtype != torch.int32:
        raise ValueError('%s: table must be float32 and cols, inv int32 (they are %s, %s, %s)'
                         % (what, t.dtype, cols.dtype, inv.dtype))
    if t.dim() != 2 or cols.dim() != 1 or inv.dim() != 1 or not 1 <= t.shape[0] <= MAX_K or t.shape[1] % 4 \
            or not t.shape[1] - 3 <= cols.shape[0] <= min(t.shape[1], inv.shape[0]) or inv.shape[0] > MAX_OUT:
        raise ValueError('%s: table must be [K, N_pad] (1 <= K <= %d, N_pad = N rounded up to 4), cols [N] and inv [M], '
                         'N <= M (they are %s, %s, %s)' % (what, MAX_K, tuple(t.shape), tuple(cols.shape), tuple(inv.shape)))
    if not (t.is_contiguous() and cols.is_contiguous() and inv.is_contiguous()):
        raise ValueError('%s: table, cols and inv must be contiguous' % what)


def _check_inputs(coef, table, base, what):
    _check_table(table, what)
    K, M = table.table.shape[0], table.inv.shape[0]
    check_tensor(what, 'coef', coef, rocm=True)
    if base is not None:
        check_tensor(what, 'base', base, rocm=True, on=(coef, 'coef'))
    for name, x in zip(BlendTable._fields, table):
        if x.device != coef.device:
            raise ValueError('%s: the table (%s) is not on the device of coef; move the module with .to()' % (what, name))
    if tuple(coef.shape) not in ((K,), (1, K)):
        raise ValueError('%s: coef must be [K] or [1, K] with K = %d (it is %s)' % (what, K, tuple(coef.shape)))
    if base is not None and base.numel() != M:
        raise ValueError('%s: base must have M = %d elements (it is %s)' % (what, M, tuple(base.shape)))
    return coef.reshape(K).contiguous(), None if base is None else base.reshape(M).contiguous()


def blend_offsets(coef, table, base=None):
    """``out[j] = sum_k coef[k] * dirs[k, j]`` over the plan ``table`` (a ``BlendTable``), flat ``[M]``.  Without a base:
    the sums, ``+0.0`` where no column covers j.  With ``base`` (M elements): ``(out, masked)`` -- ``out`` the sum where
    covered and ``base`` elsewhere, ``masked`` ``+0.0`` where covered and ``base`` elsewhere.  ``coef`` ([K] or [1, K])
    and ``base`` get gradients when they require them; the table is data."""
    coef, base = _check_inputs(coef, table, base, 'blend_offsets')
    return _Blend.apply(coef, base, *table)


class BlendShapes(nn.Module):
    """The reference's pose correctives (``module.py:485-493``) and expression offsets (``module.py:537``) over
    compact tables built here from its ``pose_dirs`` [Kp, 3 V], ``expr_dirs`` [V, 3, Ke] and hand / face mask [V]."""

    def __init__(self, pose_dirs, expr_dirs, pose_mask):
        super(BlendShapes, self).__init__()
        what = 'BlendShapes'
        for name, x in (('pose_dirs', pose_dirs), ('expr_dirs', expr_dirs), ('pose_mask', pose_mask)):
            check_tensor(what, name, x, f32=False)
            check_no_grad(what, name, x)
        if pose_mask.dtype != torch.bool or pose_mask.dim() != 1:
            raise ValueError('%s: pose_mask must be a bool tensor of shape [V] (it is %s %s)'
                             % (what, pose_mask.dtype, tuple(pose_mask.shape)))
        V = pose_mask.shape[0]
        check_tensor(what, 'pose_dirs', pose_dirs)
        check_tensor(what, 'expr_dirs', expr_dirs)
        if pose_dirs.dim() != 2 or pose_dirs.shape[1] != 3 * V or not 1 <= pose_dirs.shape[0] <= MAX_K:
            raise ValueError('%s: pose_dirs must be [Kp, 3 V] with V = %d and 1 <= Kp <= %d (it is %s)'
                             % (what, V, MAX_K, tuple(pose_dirs.shape)))
        if expr_dirs.dim() != 3 or tuple(expr_dirs.shape[:2]) != (V, 3) or not 1 <= expr_dirs.shape[2] <= MAX_K:
            raise ValueError('%s: expr_dirs must be [V, 3, Ke] with V = %d and 1 <= Ke <= %d (it is %s)'
                             % (what, V, MAX_K, tuple(expr_dirs.shape)))
        self.vertex_num = V
        pose = make_table(pose_dirs, pose_mask.to(pose_dirs.device).repeat_interleave(3))
        expr_keep = (expr_dirs != 0).reshape(V, -1).any(1).repeat_interleave(3)
        expr = make_table(expr_dirs.reshape(3 * V, -1).t(), expr_keep)
        for prefix, plan in (('pose', pose), ('expr', expr)):
            for field, x in zip(BlendTable._fields, plan):
                self.register_buffer('%s_%s' % (prefix, field), x, persistent=False)

    @property
    def pose_plan(self):
        return BlendTable(self.pose_table, self.pose_cols, self.pose_inv)

    @property
    def expr_plan(self):
        return BlendTable(self.expr_table, self.expr_cols, self.expr_inv)

    def pose_offsets(self, pose_feat, mean_offset_offset):
        """``module.py:485-493``: ``pose_feat`` ([Kp] or [1, Kp], the ``axis_angle_to_matrix(pose) - I`` row; detached
        here as there) and the regressed ``mean_offset_offset`` [V, 3] -> ``(combined, mean_offset_offset_masked)``,
        both [V, 3]: the pose offset and ``+0.0`` at the masked vertices, ``mean_offset_offset`` twice elsewhere."""
        what = 'BlendShapes.pose_offsets'
        if not isinstance(pose_feat, torch.Tensor) or not isinstance(mean_offset_offset, torch.Tensor):
            raise TypeError('%s: pose_feat and mean_offset_offset must be tensors' % what)
        if tuple(mean_offset_offset.shape) != (self.vertex_num, 3):
            raise ValueError('%s: mean_offset_offset must be [V, 3] with V = %d (it is %s)'
                             % (what, self.vertex_num, tuple(mean_offset_offset.shape)))
        coef, base = _check_inputs(pose_feat.detach(), self.pose_plan, mean_offset_offset, what)
        out, masked = _Blend.apply(coef, base, *self.pose_plan)
        return out.view(self.vertex_num, 3), masked.view(self.vertex_num, 3)

    def expr_offsets(self, expr):
        """``module.py:537``: ``expr`` [Ke] -> ``(expr[None, None, :] * expr_dirs).sum(2)`` [V, 3], ``+0.0`` at the
        vertices whose ``expr_dirs`` row is zero; ``dL/d expr`` through the fixed two-level sum."""
        what = 'BlendShapes.expr_offsets'
        check_tensor(what, 'expr', expr, f32=False)
        coef, _ = _check_inputs(expr, self.expr_plan, None, what)
        return _Blend.apply(coef, None, *self.expr_plan).view(self.vertex_num, 3)
