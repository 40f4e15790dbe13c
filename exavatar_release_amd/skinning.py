"""HIP linear blend skinning: a drop-in for ExAvatar's ``get_transform_mat_vertex`` + ``lbs`` + the camera -> world step.

* ``skin_points(points, transform_mat_joint, skinning_weight, idx, trans, R, t)`` -- reference
  ``avatar/common/nets/module.py:413-422`` called at ``module.py:548-556``: every point set posed by its vertex's
  blended transform, the translation added and, when ``R`` and ``t`` are given, taken from camera to world coordinates.
  Returns one posed ``[V, 3]`` tensor per set; gradients reach every point set, ``transform_mat_joint`` and ``trans``,
  bit-reproducibly.

The kernels are ``csrc/skinning.hip`` behind ``include/exa_skin.h``; ROCm device tensors only, no CPU path.  The CPU
restatement that pins them is ``tests/skin_oracle.py``.

Semantics
---------
With ``w = skinning_weight[idx[v]]`` (``idx`` the int64 ``nn_vertex_idxs`` that ``knn_points`` gives, or None for the
identity) the vertex transform's rows 0-2 are ``A[r][c] = sum_j w_j * T[j][r][c]``, summed over all J joints in order
from +0, and ``p = A [x, y, z, 1] + trans``; with the camera step ``out = inverse(R) (p - t)``.  Every operation is
rounded in fp32 without fused multiply-adds, in the order the header writes out.  A is computed once per vertex and
applied to every set, as the reference's two ``lbs`` calls share ``transform_mat_vertex``.  ``inverse(R)`` is taken with
torch here, as the reference does.

The backward sums the per-vertex outer products into ``grad_T`` and ``grad_trans`` in a fixed two-level order (chunks of
256 vertices, then the chunk partials in order; see the header) with no atomics, so the same inputs give the same bits.
Row 3 of ``grad_T`` is zero, as the reference's autograd gives.  ``skinning_weight`` is a buffer and ``R`` / ``t`` are
data in the reference: they get no gradient, and a tensor of theirs that requires one is refused.  An index outside
``[0, len(skinning_weight))`` reads nothing and makes its vertex's weights NaN.

Each call allocates its outputs (and, backward, a workspace from the torch allocator) and launches one kernel forward,
two backward; the kernels do not synchronise and can be captured into a hipGraph.  The camera step's ``torch.inverse(R)``
is torch's and synchronises on ROCm, so a call with ``R`` cannot be captured; one without can.
"""
import torch

from . import _lib
from ._device import _ptr, _ptrs, _workspace, check_no_grad, check_tensor, grad_in, launch

MAX_JOINTS = 64           # EXA_SKIN_MAX_JOINTS
MAX_SETS = 4              # EXA_SKIN_MAX_SETS


class _Skin(torch.autograd.Function):
    """weights [Vw, J], idx [V] int64 or None, Rinv [3, 3] or None, t [3] or None, T [J, 4, 4], trans [3], *points
    [V, 3] (all float32, contiguous) -> tuple of posed [V, 3]."""

    @staticmethod
    def forward(ctx, weights, idx, Rinv, t, T, trans, *points):
        V, S, J, Vw = points[0].shape[0], len(points), T.shape[0], weights.shape[0]
        dev = T.device
        outs = [torch.empty((V, 3), dtype=torch.float32, device=dev) for _ in points]
        launch(_lib.SKIN, 'exa_skin_forward', dev, V, S, J, Vw, _ptrs(points), _ptr(weights), _ptr(idx), _ptr(T),
               _ptr(trans), _ptr(Rinv), _ptr(t), _ptrs(outs))
        ctx.save_for_backward(weights, idx, Rinv, T, *points)      # (idx and Rinv may be None: saved as None)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        weights, idx, Rinv, T, *points = ctx.saved_tensors
        V, S, J, Vw = points[0].shape[0], len(points), T.shape[0], weights.shape[0]
        dev = T.device
        need = ctx.needs_input_grad
        grads = [torch.zeros((V, 3), dtype=torch.float32, device=dev) if g is None else grad_in(g) for g in grads]
        gpts = [torch.empty((V, 3), dtype=torch.float32, device=dev) if need[6 + s] else None for s in range(S)]
        gT = torch.empty((J, 4, 4), dtype=torch.float32, device=dev) if need[4] else None
        gtrans = torch.empty(3, dtype=torch.float32, device=dev) if need[5] else None
        if any(g is not None for g in gpts) or gT is not None or gtrans is not None:
            nbytes = _lib.skin_workspace_size(V, J)
            ws = _workspace(nbytes, dev)
            launch(_lib.SKIN, 'exa_skin_backward', dev, V, S, J, Vw, _ptrs(points), _ptr(weights), _ptr(idx), _ptr(T),
                   _ptr(Rinv), _ptrs(grads), _ptrs(gpts), _ptr(gT), _ptr(gtrans), _ptr(ws) if nbytes else None, nbytes)
        return (None, None, None, None, gT, gtrans) + tuple(gpts)


def skin_points(points, transform_mat_joint, skinning_weight, idx=None, trans=None, R=None, t=None):
    """Pose 1-4 point sets ``[V, 3]`` (a tensor or a sequence of them) with linear blend skinning (module docstring).

    ``transform_mat_joint`` [J, 4, 4] (J <= 64), ``skinning_weight`` [Vw, J], ``idx`` [V] int64 or None (then Vw == V),
    ``trans`` [3] or [1, 3] or None (zero), ``R`` [3, 3] and ``t`` [3] or [1, 3] (both or neither: the camera -> world
    step ``inverse(R) (p - t)``).  Returns a tuple with one posed ``[V, 3]`` tensor per set."""
    what = 'skin_points'
    sets = (points,) if isinstance(points, torch.Tensor) else tuple(points)
    if not 1 <= len(sets) <= MAX_SETS:
        raise ValueError('skin_points: 1 .. %d point sets (got %d)' % (MAX_SETS, len(sets)))
    T = transform_mat_joint
    # what the reference holds as a buffer or as data gets no gradient
    check_no_grad(what, 'skinning_weight', skinning_weight, 'a buffer')
    check_no_grad(what, 'R', R, 'camera data')
    check_no_grad(what, 't', t, 'camera data')
    check_tensor(what, 'transform_mat_joint', T)
    if T.dim() != 3 or T.shape[1:] != (4, 4) or not 1 <= T.shape[0] <= MAX_JOINTS:
        raise ValueError('skin_points: transform_mat_joint must be [J, 4, 4] with 1 <= J <= %d' % MAX_JOINTS)
    J = T.shape[0]
    for s, x in enumerate(sets):
        check_tensor(what, 'points[%d]' % s, x)
        if x.dim() != 2 or x.shape[1] != 3 or x.shape[0] != sets[0].shape[0]:
            raise ValueError('skin_points: every point set must be [V, 3] with the same V')
    V = sets[0].shape[0]
    check_tensor(what, 'skinning_weight', skinning_weight)
    if skinning_weight.dim() != 2 or skinning_weight.shape[1] != J:
        raise ValueError('skin_points: skinning_weight must be [Vw, J] with J = %d' % J)
    if idx is not None:
        if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64 or tuple(idx.shape) != (V,):
            raise ValueError('skin_points: idx must be an int64 [V] tensor (V = %d)' % V)
    elif skinning_weight.shape[0] != V:
        raise ValueError('skin_points: without idx, skinning_weight must have V = %d rows' % V)
    if trans is not None:
        check_tensor(what, 'trans', trans)
        if tuple(trans.shape) not in ((3,), (1, 3)):
            raise ValueError('skin_points: trans must be [3] or [1, 3]')
    if (R is None) != (t is None):
        raise ValueError('skin_points: R and t must be given together')
    if R is not None:
        check_tensor(what, 'R', R)
        if tuple(R.shape) != (3, 3):
            raise ValueError('skin_points: R must have shape (3, 3) (it has %s)' % (tuple(R.shape),))
        check_tensor(what, 't', t)
        if tuple(t.shape) not in ((3,), (1, 3)):
            raise ValueError('skin_points: t must be [3] or [1, 3]')
    dev = T.device
    for name, x in [('transform_mat_joint', T), ('skinning_weight', skinning_weight), ('idx', idx), ('trans', trans),
                    ('R', R), ('t', t)] + [('points[%d]' % s, x) for s, x in enumerate(sets)]:
        if x is not None:
            check_tensor(what, name, x, f32=False, rocm=True, on=(T, 'transform_mat_joint'))
    if trans is None:
        trans = torch.zeros(3, dtype=torch.float32, device=dev)
    Rinv = tv = None
    if R is not None:
        Rinv = torch.inverse(R).contiguous()
        tv = t.reshape(3).contiguous()
    outs = _Skin.apply(skinning_weight.contiguous(), None if idx is None else idx.contiguous(), Rinv, tv,
                       T.contiguous(), trans.reshape(3).contiguous(), *[x.contiguous() for x in sets])
    return tuple(outs)
