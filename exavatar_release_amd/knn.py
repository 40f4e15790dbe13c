"""HIP K-nearest-neighbour search: a drop-in for pytorch3d's ``knn_points`` where ExAvatar calls it.

* ``knn_points(p1, p2, K=1, return_nn=True)`` -- reference ``avatar/common/nets/module.py:543`` (the nearest template
  vertex of every upsampled Gaussian centre, every training sample and every animation frame) and ``module.py:86`` (a
  K = 4 self-query that sizes the scene Gaussians at init).  Returns ``KNN(dists, idx, knn)`` like
  ``p3d_standins.knn_points``, with the same shapes in every case (N, P1 or P2 = 0 included).

The kernels are ``csrc/knn.hip`` behind ``include/exa_knn.h``; ROCm device tensors only, no CPU path (CPU callers keep
``p3d_standins.knn_points``).  The CPU restatement that pins them is ``tests/knn_oracle.py``.

Semantics
---------
For batch element n and query i the result is the K smallest pairs ``(d(i, j), j)`` in lexicographic order: ascending
d, ties to the lower ref index j.  d is the fp32 squared distance evaluated operation by operation,
``dx = a.x - b.x`` (likewise y, z), ``d = (dx * dx + dy * dy) + dz * dz``, every operation rounded in fp32 and no fused
multiply-add; ``dists`` is that d bit for bit, ``idx`` is int64 and ``knn`` is ``p2[idx]``.  ``K = min(K, P2)`` as in
the stand-in; the results are always sorted (``return_sorted=False`` is accepted and changes nothing).  Supported: float32
points with D = 3 and 1 <= K <= 32.  ``lengths1`` / ``lengths2`` (padded batches) and ``norm != 2`` raise
NotImplementedError.  Inputs must be finite: the order above is not defined for NaN.

Because the order is total, the result does not depend on the order in which refs are visited: ``config.knn_cull``
(default True) lets the search skip chunks of refs whose bounding box is provably farther than every query's current K-th
neighbour, and returns the same bits as the brute-force search it replaces.

Gradients: ``dists`` and ``knn`` are differentiable with respect to both point sets.  Both go through the HIP backward
(``exa_knn_backward``), which sums every output element in a fixed order without atomics, so the gradients are
bit-reproducible; the stable ordering of ``idx`` it takes as input is a ``torch.sort(stable=True)``.
"""
from collections import namedtuple

import torch

from . import _lib
from ._device import _ptr, _workspace, config, grad_in, launch, need_rocm

KNN = namedtuple('KNN', 'dists idx knn')

MAX_K = 32


class _KnnPoints(torch.autograd.Function):
    """p1 [N,P1,3], p2 [N,P2,3] (float32, contiguous) -> (dists [N,P1,K], idx [N,P1,K] int64, knn [N,P1,K,3] or an
    empty placeholder)."""

    @staticmethod
    def forward(ctx, p1, p2, K, want_nn):
        N, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
        device = p1.device
        dists = torch.empty((N, P1, K), dtype=torch.float32, device=device)
        idx = torch.empty((N, P1, K), dtype=torch.int64, device=device)
        if N * P1 * K > 0:
            flags = 0 if config.knn_cull else _lib.KNN_NO_CULL
            nbytes = _lib.knn_workspace_size(N, P1, P2, K) if config.knn_cull else 0
            ws = _workspace(nbytes, device)
            launch(_lib.KNN, 'exa_knn_forward', device, N, P1, P2, K, _ptr(p1), _ptr(p2), flags, _ptr(ws), nbytes,
                   _ptr(dists), _ptr(idx), None)
        if want_nn:
            knn = torch.gather(p2, 1, idx.view(N, P1 * K, 1).expand(N, P1 * K, 3)).view(N, P1, K, 3)
        else:
            knn = p1.new_empty(0)
        ctx.K = K
        ctx.save_for_backward(p1, p2, idx)
        ctx.mark_non_differentiable(idx)
        return dists, idx, knn

    @staticmethod
    def backward(ctx, grad_dists, _grad_idx, grad_knn):
        p1, p2, idx = ctx.saved_tensors
        if grad_knn is not None and grad_knn.numel() == 0:
            grad_knn = None
        if grad_dists is None and grad_knn is None:
            return None, None, None, None
        N, P1, P2, K = p1.shape[0], p1.shape[1], p2.shape[1], ctx.K
        grad_dists, grad_knn = grad_in(grad_dists), grad_in(grad_knn)
        if K == 0:                                   # no refs: nothing was chosen
            return torch.zeros_like(p1), torch.zeros_like(p2), None, None
        grad_p1 = torch.empty_like(p1)
        grad_p2 = torch.empty_like(p2)
        if N * (P1 + P2) > 0:
            sorted_idx, order = torch.sort(idx.view(N, P1 * K), dim=1, stable=True)
            launch(_lib.KNN, 'exa_knn_backward', p1.device, N, P1, P2, K, _ptr(p1), _ptr(p2), _ptr(idx),
                   _ptr(grad_dists), _ptr(grad_knn), _ptr(sorted_idx), _ptr(order), _ptr(grad_p1), _ptr(grad_p2))
        return grad_p1, grad_p2, None, None


def knn_points(p1, p2, lengths1=None, lengths2=None, norm: int = 2, K: int = 1, version: int = -1,
               return_nn: bool = False, return_sorted: bool = True):
    """K nearest neighbours in ``p2`` [N, P2, 3] of every point of ``p1`` [N, P1, 3] on the ROCm device (module
    docstring).  Returns ``KNN(dists [N, P1, K] ascending squared distances, idx [N, P1, K] int64, knn [N, P1, K, 3] or
    None)`` with ``K = min(K, P2)``; ``dists`` and ``knn`` are differentiable with respect to ``p1`` and ``p2``."""
    if norm != 2:
        raise NotImplementedError('knn_points: squared L2 distances only (what the reference uses)')
    if lengths1 is not None or lengths2 is not None:
        raise NotImplementedError('knn_points: padded batches are not used by the reference')
    if p1.dim() != 3 or p2.dim() != 3 or p1.shape[0] != p2.shape[0] or p1.shape[2] != p2.shape[2]:
        raise ValueError('knn_points expects p1 [N, P1, D] and p2 [N, P2, D]')
    if p1.shape[2] != 3:
        raise NotImplementedError('knn_points: D = 3 only')
    if not 1 <= int(K) <= MAX_K:
        raise ValueError('knn_points: K must be 1 .. %d' % MAX_K)
    need_rocm(p1.device, 'knn_points')
    need_rocm(p2.device, 'knn_points')
    if p1.device != p2.device:
        raise ValueError('knn_points: p1 and p2 are on different devices')
    if p1.dtype != torch.float32 or p2.dtype != torch.float32:
        raise ValueError('knn_points: float32 points only')
    K = min(int(K), p2.shape[1])
    dists, idx, knn = _KnnPoints.apply(p1.contiguous(), p2.contiguous(), K, bool(return_nn))
    return KNN(dists=dists, idx=idx, knn=knn if return_nn else None)
