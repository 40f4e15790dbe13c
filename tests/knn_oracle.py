"""numpy float32 restatement of knn_points' semantics (include/exa_knn.h, exavatar_release_amd/knn.py), independent of the
HIP code and of the PyTorch stand-in.

For every batch element n and query i: the K smallest pairs (d(i, j), j) in lexicographic order, where
dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z and d = (dx * dx + dy * dy) + dz * dz, every operation a float32 numpy
operation (numpy rounds each one and never fuses a multiply-add).  K = min(K, P2)."""
import numpy as np


def sq_dists(a, b):
    """[P1, 3] x [P2, 3] float32 -> [P1, P2] float32 squared distances, spelled out operation by operation."""
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    xx = dx * dx
    yy = dy * dy
    zz = dz * dz
    s = xx + yy
    d = s + zz
    assert d.dtype == np.float32
    return d


def knn(p1, p2, K, block=2048):
    """p1 [N, P1, 3], p2 [N, P2, 3] (float32 arrays) -> (dists [N, P1, K] float32, idx [N, P1, K] int64)."""
    p1 = np.asarray(p1, dtype=np.float32)
    p2 = np.asarray(p2, dtype=np.float32)
    N, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    K = min(K, P2)
    dists = np.empty((N, P1, K), dtype=np.float32)
    idx = np.empty((N, P1, K), dtype=np.int64)
    j = np.arange(P2, dtype=np.int64)
    for n in range(N):
        for s in range(0, P1, block):
            d = sq_dists(p1[n, s:s + block], p2[n])
            for r in range(d.shape[0]):
                # lexsort: the LAST key is primary -> ascending d, ties to the lower j
                o = np.lexsort((j, d[r]))[:K]
                dists[n, s + r] = d[r, o]
                idx[n, s + r] = o
    return dists, idx


def knn_nearest(p1, p2, block=4096):
    """K = 1 for large inputs: the smallest (d, j) per query without sorting every row (argmin returns the FIRST
    minimum, i.e. the lower index on a tie).  Same result as knn(p1, p2, 1)."""
    p1 = np.asarray(p1, dtype=np.float32)
    p2 = np.asarray(p2, dtype=np.float32)
    N, P1 = p1.shape[0], p1.shape[1]
    dists = np.empty((N, P1, 1), dtype=np.float32)
    idx = np.empty((N, P1, 1), dtype=np.int64)
    for n in range(N):
        for s in range(0, P1, block):
            d = sq_dists(p1[n, s:s + block], p2[n])
            o = d.argmin(1)
            idx[n, s:s + block, 0] = o
            dists[n, s:s + block, 0] = d[np.arange(d.shape[0]), o]
    return dists, idx


def knn_small_k(p1, p2, K, block=1024):
    """Large inputs, small K: argpartition to a candidate set that surely contains the K smallest (d, j) -- every j
    whose d is <= the K-th smallest d -- then the lexicographic order on it.  Same result as knn(p1, p2, K)."""
    p1 = np.asarray(p1, dtype=np.float32)
    p2 = np.asarray(p2, dtype=np.float32)
    N, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    K = min(K, P2)
    dists = np.empty((N, P1, K), dtype=np.float32)
    idx = np.empty((N, P1, K), dtype=np.int64)
    for n in range(N):
        for s in range(0, P1, block):
            d = sq_dists(p1[n, s:s + block], p2[n])
            kth = np.partition(d, K - 1, axis=1)[:, K - 1:K]
            for r in range(d.shape[0]):
                cand = np.nonzero(d[r] <= kth[r])[0]           # ascending j
                o = cand[np.lexsort((cand, d[r, cand]))][:K]
                dists[n, s + r] = d[r, o]
                idx[n, s + r] = o
    return dists, idx
