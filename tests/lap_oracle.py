"""CPU oracles of the mesh Laplacian regulariser (include/exa_mesh.h, exavatar_release_amd/mesh_reg.py).

(a) ``forward32`` / ``backward32``: the header's arithmetic restated in numpy float32, one array operation per rounded
    operation and an explicit loop over the slots k (forward) and over the position in every vertex's incoming list
    (backward).  numpy evaluates ``a * b`` and ``c + p`` as two separately rounded array operations, so no product is
    fused into an add and no sum is re-associated: the results are what the kernels must give bit for bit.

(b) ``forward64`` / ``backward64``: the same functions of the same float32 inputs in float64 -- exact for the purpose,
    its own rounding is 2^-29 of the bound below -- returning next to every output a first-order bound on the error of ANY
    float32 evaluation of it, whatever its summation order.  With u = 2^-24:

    * lap.  ``lap = x_v + sum_k x_k w_k`` is a sum of K + 1 terms, K of them rounded products.  Every term passes through
      at most one product rounding and at most K additions, i.e. at most K + 1 roundings, in any order of summation, so
      to first order  |fl(lap) - lap| <= (K + 1) u (|x_v| + sum_k |x_k w_k|) =: E.
    * d.  Without a target d = lap(out) and E_d = E_out.  With one, d = lap(out) - lap(target): the two errors add and
      the subtraction rounds once:  E_d = E_out + E_target + u |d|.
    * loss.  d^2 moves by 2 |d| E_d when d moves by E_d, and the product rounds once:  E_loss = 2 |d| E_d + u d^2.  A
      weight multiplies value and bound by |weight| and rounds once more:  E_loss = (2 |d| E_d + u d^2) |weight| + u |loss|.
      (First order: the neglected term is E_d^2, which matters only where |d| < E_d.)
    * g = (grad_loss * weight) * (2 d).  2 d is exact; one rounding per product (two with a weight, one without):
      E_g = 2 |grad_loss weight| E_d + r u |g|,  r = 1 or 2.
    * dL/dout[v] = g_v + sum_e w_e g_u(e) over the n incoming slots: the inputs' bounds carry over, weighted, and the
      sum of n + 1 terms with n products adds, as for lap,  (n + 1) u (|g_v| + sum_e |w_e g_u|):
      E_grad = E_g[v] + sum_e |w_e| E_g[u(e)] + (n + 1) u (|g_v| + sum_e |w_e g_u(e)|).

    The bounds hold for the reference's own summation order too (PyTorch's ``sum(2)`` and its scatter-add backward),
    so two float32 evaluations differ by at most twice the bound.

``transpose`` is the incoming-list CSR in the order the header states, built independently of the library.
"""
import numpy as np

U = 2.0 ** -24


def transpose(idx):
    """CSR (offsets [V + 1], entries [V * K]) of the slots u * K + k that name each vertex, ascending u then k."""
    V, K = idx.shape
    flat = np.asarray(idx, dtype=np.int64).reshape(-1)
    entries = np.argsort(flat, kind='stable')              # stable: ascending slot number within a vertex
    offsets = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(flat, minlength=V), out=offsets[1:])
    return offsets.astype(np.int32), entries.astype(np.int32)


# ---- (a) float32, op by op ------------------------------------------------------------------------------------------
def lap32(x, idx, w):
    x = np.asarray(x, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    acc = x.copy()
    for k in range(idx.shape[1]):
        p = x[:, idx[:, k], :] * w[None, :, k, None]
        acc = acc + p
    return acc


def forward32(out, target, idx, w, weight=None):
    """-> (loss, d), float32 [B, V, C]."""
    d = lap32(out, idx, w)
    if target is not None:
        t = lap32(target, idx, w)
        d = d - t                                          # [1, V, C] broadcasts over b
    loss = d * d
    if weight is not None:
        loss = loss * np.asarray(weight, dtype=np.float32).reshape(1, -1, 1)
    return loss.astype(np.float32), d.astype(np.float32)


def backward32(d, grad_loss, idx, w, weight=None):
    """-> dL/dout, float32 [B, V, C], summed in the header's order."""
    d = np.asarray(d, dtype=np.float32)
    g = np.asarray(grad_loss, dtype=np.float32)
    if weight is not None:
        g = g * np.asarray(weight, dtype=np.float32).reshape(1, -1, 1)
    g = g * (np.float32(2.0) * d)
    wflat = np.asarray(w, dtype=np.float32).reshape(-1)
    K = idx.shape[1]
    offsets, entries = transpose(idx)
    deg = np.diff(offsets)
    acc = g.copy()
    for r in range(int(deg.max()) if deg.size else 0):     # the r-th incoming slot of every vertex that has one
        sel = np.nonzero(deg > r)[0]
        e = entries[offsets[sel] + r]
        p = wflat[e][None, :, None] * g[:, e // K, :]
        acc[:, sel, :] = acc[:, sel, :] + p
    return acc


# ---- (b) float64 with first-order bounds ----------------------------------------------------------------------------
def lap64(x, idx, w):
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    K = idx.shape[1]
    p = x[:, idx, :] * w[None, :, :, None]                 # [B, V, K, C]
    lap = x + p.sum(2)
    E = (K + 1) * U * (np.abs(x) + np.abs(p).sum(2))
    return lap, E


def forward64(out, target, idx, w, weight=None):
    """-> dict(loss, E_loss, d, E_d), float64 [B, V, C]."""
    d, E_d = lap64(out, idx, w)
    if target is not None:
        t, E_t = lap64(target, idx, w)
        d = d - t
        E_d = E_d + E_t + U * np.abs(d)
    loss = d * d
    E_loss = 2 * np.abs(d) * E_d + U * loss
    if weight is not None:
        wv = np.asarray(weight, dtype=np.float64).reshape(1, -1, 1)
        loss = loss * wv
        E_loss = E_loss * np.abs(wv) + U * np.abs(loss)
    return dict(loss=loss, E_loss=E_loss, d=d, E_d=E_d)


def backward64(d, E_d, grad_loss, idx, w, weight=None):
    """-> (dL/dout, E_grad), float64 [B, V, C]; d, E_d are forward64's."""
    gl = np.asarray(grad_loss, dtype=np.float64)
    rounds = 1
    if weight is not None:
        gl = gl * np.asarray(weight, dtype=np.float64).reshape(1, -1, 1)
        rounds = 2
    g = gl * (2 * d)
    E_g = 2 * np.abs(gl) * E_d + rounds * U * np.abs(g)
    V, K = idx.shape
    w = np.asarray(w, dtype=np.float64)
    grad, E, mag = g.copy(), E_g.copy(), np.abs(g)
    for k in range(K):                                     # float64: the order of this scatter does not matter
        t = g * w[None, :, k, None]
        np.add.at(grad, (slice(None), idx[:, k]), t)
        np.add.at(mag, (slice(None), idx[:, k]), np.abs(t))
        np.add.at(E, (slice(None), idx[:, k]), E_g * np.abs(w[None, :, k, None]))
    n = np.bincount(np.asarray(idx).reshape(-1), minlength=V).reshape(1, V, 1)
    return grad, E + (n + 1) * U * mag


# ---- test meshes ----------------------------------------------------------------------------------------------------
def grid_faces(rows, cols):
    """Two triangles per cell of a rows x cols vertex grid: corners of valence 2 and 3, edges of 4, interior of 6."""
    r, c = np.meshgrid(np.arange(rows - 1), np.arange(cols - 1), indexing='ij')
    a = (r * cols + c).reshape(-1)
    return np.concatenate([np.stack([a, a + 1, a + cols], 1), np.stack([a + 1, a + cols + 1, a + cols], 1)]).astype(np.int64)


def random_table(V, K, seed, pad=True, hub=False, orphan=False):
    """General weights and random neighbours (repeats and self-references allowed); with ``pad`` a third of the rows are
    padded as the reference pads (the vertex itself, weight 0); with ``hub`` a quarter of all slots, at most 300, name vertex 0
    (a long incoming list); with ``orphan`` no slot names vertex V - 1 (an empty one), where V > 1 allows it."""
    rng = np.random.RandomState(seed)
    idx = rng.randint(0, V, size=(V, K)).astype(np.int64)
    w = rng.standard_normal((V, K)).astype(np.float32)
    if hub:
        idx.reshape(-1)[rng.choice(V * K, size=min(V * K // 4, 300), replace=False)] = 0
    if pad:
        for v in rng.choice(V, size=max(V // 3, 1), replace=False):
            n = rng.randint(0, K + 1)
            idx[v, n:] = v
            w[v, n:] = 0.0
    if orphan and V > 1:
        idx[idx == V - 1] = 0
    return idx, w
