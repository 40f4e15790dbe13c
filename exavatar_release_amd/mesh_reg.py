"""HIP mesh Laplacian regulariser: a drop-in for ExAvatar's ``LaplacianReg`` with a bit-reproducible backward.

* ``LaplacianReg(vertex_num, face, neighbor_max_num=10)`` -- reference ``avatar/common/nets/loss.py:97-131``, called six
  times per iteration at ``avatar/main/model.py:237-247``.  ``forward(out, target)`` (``target`` may be ``None``) returns
  the elementwise ``[B, V, C]`` loss; an optional third argument ``weight`` multiplies a per-vertex weight into it inside
  the kernel.  ``neighbor_idxs`` (int64) and ``neighbor_weights`` are attributes, as in the reference.
* ``mesh_laplacian_loss(out, target, neighbor_idxs, neighbor_weights, weight=None)`` -- the same for a caller's own table.

The kernels are ``csrc/mesh_reg.hip`` behind ``include/exa_mesh.h``; ROCm float32 tensors only, no CPU path.  The CPU
restatement that pins them is ``tests/lap_oracle.py``.

Semantics
---------
``lap(x)[b,v,c] = x[b,v,c]``, then for the K slots of vertex v's table row in order ``lap += x[b, idx[v,k], c] * w[v,k]``;
``d = lap(out)`` or ``lap(out) - lap(target)`` (``target`` ``[B, V, C]`` or ``[1, V, C]``); ``loss = d * d`` and, with a
weight, ``loss * weight[v]``.  Every operation is rounded in fp32 without fused multiply-adds, in this order.  PyTorch
evaluates the reference's ``(x[:, idx] * w).sum(2)`` in an order of its own, so the two differ by rounding; the bound is
derived in ``tests/lap_oracle.py``.  Padded slots (the vertex itself, weight 0) are evaluated like any other, as the
reference does.

The table is the reference's, element for element.  ``get_neighbor`` keeps ``list(adj[v])[:neighbor_max_num]`` of a
Python ``set``, so the slot order -- and, for a vertex with more neighbours than slots, WHICH neighbours are kept -- is
CPython's set iteration order, which is not ascending.  The constructor therefore fills one Python set per vertex with
the same operations in the same order (about 2 s for 90 000 vertices, once per model).

The backward gathers, for every vertex, the slots that name it from a transposed table in CSR form (ascending row, then
slot; built once per table and device by ``exa_mesh_neighbor_transpose``) -- no atomics and a summation order the header
states, so the same inputs give the same bits on every call by construction, where the order of the reference's
``index_put_(accumulate=True)`` is PyTorch's own business.  ``target`` and ``weight`` are data in the reference and get no
gradient.

Each call allocates its outputs (backward: a workspace from the torch allocator) and launches one kernel forward, two
backward, on the current stream; nothing synchronises once the tables are cached, so calls can be captured into a hipGraph.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._device import _ptr, _workspace, check_no_grad, check_rows, check_shape, check_tensor, grad_in, launch
from ._tables import Cache, host_i32, host_ptr, stamp

MAX_CHANNELS = 8          # EXA_MESH_LAP_MAX_CHANNELS
MAX_NEIGHBORS = 16        # EXA_MESH_LAP_MAX_NEIGHBORS


def neighbor_table(vertex_num, face, neighbor_max_num=10):
    """The reference's ``get_neighbor``: ``(neighbor_idxs [V, K] int64, neighbor_weights [V, K] float32)`` as numpy
    arrays.  Row v holds ``list(adj[v])[:K]`` -- adj[v] a Python set filled in ascending face order -- with weight
    ``-1 / n`` in those n slots, and v itself with weight 0 in the rest."""
    V, K = int(vertex_num), int(neighbor_max_num)
    if V < 0 or not 1 <= K <= MAX_NEIGHBORS:
        raise ValueError('LaplacianReg: vertex_num must be >= 0 and neighbor_max_num 1 .. %d' % MAX_NEIGHBORS)
    faces = (face.detach().cpu().numpy() if isinstance(face, torch.Tensor) else np.asarray(face)).tolist()
    adj = [set() for _ in range(V)]
    for f in faces:
        corners = set(f)
        for v in f:
            if not 0 <= v < V:
                raise ValueError('LaplacianReg: face index %d is outside [0, %d)' % (v, V))
            # the set operations the reference performs, so that the iteration order below is the reference's
            adj[v] |= corners - {v}
    idxs = np.tile(np.arange(V, dtype=np.int64)[:, None], (1, K))
    weights = np.zeros((V, K), dtype=np.float32)
    for v in range(V):
        n = min(len(adj[v]), K)
        if n == 0:
            raise ValueError('LaplacianReg: vertex %d belongs to no face (the reference divides by zero there)' % v)
        idxs[v, :n] = list(adj[v])[:n]
        weights[v, :n] = -1.0 / n
    return idxs, weights


def _device_tables(idxs, weights, device):
    """(idx [V, K] int32, w [V, K] float32, CSR offsets [V + 1], CSR entries [V * K]) on ``device``."""
    idx32 = host_i32('mesh_laplacian_loss', 'neighbor_idxs', idxs, (None, None))
    V, K = idx32.shape
    bad = idx32[(idx32 < 0) | (idx32 >= V)]
    if bad.size:      # a ValueError here; the library would refuse it too, as a RuntimeError
        raise ValueError('mesh_laplacian_loss: neighbour index %d is outside [0, %d)' % (bad[0], V))
    offsets, entries = np.zeros(V + 1, dtype=np.int32), np.zeros(max(V * K, 1), dtype=np.int32)
    _lib.MESH.check(_lib.load().exa_mesh_neighbor_transpose(V, K, host_ptr(idx32), host_ptr(offsets), host_ptr(entries)))
    return (torch.from_numpy(idx32).to(device), weights.detach().to(device=device, dtype=torch.float32).contiguous(),
            torch.from_numpy(offsets).to(device), torch.from_numpy(entries).to(device))


class _Laplacian(torch.autograd.Function):
    """out [B, V, C], target [Bt, V, C] or None, weight [V] or None (float32, contiguous), the four device tables
    -> (loss [B, V, C], d [B, V, C]); d is not differentiable."""

    @staticmethod
    def forward(ctx, out, target, weight, idx, w, offsets, entries):
        B, V, C = out.shape
        K = idx.shape[1]
        dev = out.device
        loss, d = torch.empty_like(out), torch.empty_like(out)
        launch(_lib.MESH, 'exa_mesh_laplacian_forward', dev, B, target.shape[0] if target is not None else 1, V, C, K,
               _ptr(out), _ptr(target), _ptr(idx), _ptr(w), _ptr(weight), _ptr(loss), _ptr(d))
        ctx.save_for_backward(d, w, offsets, entries, weight)      # (weight may be None: saved as None)
        ctx.mark_non_differentiable(d)
        return loss, d

    @staticmethod
    def backward(ctx, grad_loss, _grad_d):
        if grad_loss is None or not ctx.needs_input_grad[0]:
            return (None,) * 7
        d, w, offsets, entries, weight = ctx.saved_tensors
        B, V, C = d.shape
        dev = d.device
        grad_loss = grad_in(grad_loss)
        gout = torch.empty_like(d)
        nbytes = _lib.laplacian_workspace_size(B, V, C)
        ws = _workspace(nbytes, dev)
        launch(_lib.MESH, 'exa_mesh_laplacian_backward', dev, B, V, C, w.shape[1], _ptr(d), _ptr(grad_loss), _ptr(w),
               _ptr(weight), _ptr(offsets), _ptr(entries), _ptr(ws) if nbytes else None, nbytes, _ptr(gout))
        return (gout,) + (None,) * 6


def _check_inputs(out, target, weight, V, what):
    check_tensor(what, 'out', out, rocm=True)
    for name, x in (('target', target), ('weight', weight)):
        if x is not None:
            check_tensor(what, name, x, rocm=True, on=(out, 'out'))
    check_no_grad(what, 'target', target)
    if out.dim() != 3 or out.shape[1] != V or not 1 <= out.shape[2] <= MAX_CHANNELS:
        raise ValueError('%s: out must be [B, V, C] with V = %d and 1 <= C <= %d (it is %s)'
                         % (what, V, MAX_CHANNELS, tuple(out.shape)))
    if target is not None:
        check_shape(what, 'target', target, out.shape, '[B, V, C] or [1, V, C] like out', shared=True)
    if weight is not None:
        weight = check_rows(what, 'weight', weight, V, ((V,), (1, V, 1), (V, 1)), '[V], [1, V, 1] or [V, 1]')
    return out.contiguous(), None if target is None else target.contiguous(), weight


_tables = Cache()     # functional form: (stamp of idxs and weights, device) -> the four device tables


def mesh_laplacian_loss(out, target, neighbor_idxs, neighbor_weights, weight=None, return_d=False):
    """``LaplacianReg.forward`` for a caller's own table: ``neighbor_idxs`` [V, K] (an integer tensor, every entry in
    [0, V)) and ``neighbor_weights`` [V, K] float32, K <= 16, with general weights.  The device copies and the transposed
    table are cached per pair of tensor objects and device (an in-place change of either rebuilds them).  Returns the
    ``[B, V, C]`` loss, or ``(loss, d)`` with ``return_d`` (``d`` is what is squared; it carries no gradient)."""
    what = 'mesh_laplacian_loss'
    if not isinstance(neighbor_idxs, torch.Tensor) or not isinstance(neighbor_weights, torch.Tensor) \
            or neighbor_idxs.dim() != 2 or neighbor_idxs.shape != neighbor_weights.shape \
            or neighbor_idxs.dtype not in (torch.int32, torch.int64) or not 1 <= neighbor_idxs.shape[1] <= MAX_NEIGHBORS:
        raise ValueError('%s: neighbor_idxs (int32 / int64) and neighbor_weights must be [V, K] tensors, 1 <= K <= %d'
                         % (what, MAX_NEIGHBORS))
    check_no_grad(what, 'neighbor_weights', neighbor_weights)
    out, target, weight = _check_inputs(out, target, weight, neighbor_idxs.shape[0], what)
    key = stamp(neighbor_idxs, neighbor_weights) + (str(out.device),)
    tables = _tables.find(key) or _tables.keep(key, _device_tables(neighbor_idxs, neighbor_weights, out.device),
                                               neighbor_idxs, neighbor_weights)
    loss, d = _Laplacian.apply(out, target, weight, *tables)
    return (loss, d) if return_d else loss


class LaplacianReg(nn.Module):
    """Drop-in for the reference's ``LaplacianReg`` (``loss.py:97-131``): same constructor, same ``forward(out, target)``
    and result, same ``neighbor_idxs`` / ``neighbor_weights`` attributes (on the current ROCm device when there is one,
    as the reference's ``.cuda()`` puts them).  ``forward`` takes an optional per-vertex ``weight``."""

    def __init__(self, vertex_num, face, neighbor_max_num=10):
        super(LaplacianReg, self).__init__()
        self.neighbor_idxs, self.neighbor_weights = self.get_neighbor(vertex_num, face, neighbor_max_num)
        self._tables = {}     # device -> (idx int32, w, CSR offsets, CSR entries), built on first use

    def get_neighbor(self, vertex_num, face, neighbor_max_num=10):
        idxs, weights = neighbor_table(vertex_num, face, neighbor_max_num)
        idxs, weights = torch.from_numpy(idxs), torch.from_numpy(weights)
        if torch.cuda.is_available():
            idxs, weights = idxs.cuda(), weights.cuda()
        return idxs, weights

    def forward(self, out, target, weight=None):
        out, target, weight = _check_inputs(out, target, weight, self.neighbor_idxs.shape[0], 'LaplacianReg')
        tables = self._tables.get(out.device)
        if tables is None:
            tables = self._tables[out.device] = _device_tables(self.neighbor_idxs, self.neighbor_weights, out.device)
        return _Laplacian.apply(out, target, weight, *tables)[0]
