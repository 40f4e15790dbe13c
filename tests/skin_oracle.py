"""numpy restatement of the skinning's semantics (include/exa_skin.h, exavatar_release_amd/skinning.py), independent of
the HIP code and of the reference's torch expression.

With w = weights[idx[v]] (NaN for an index outside [0, Vw)), every operation one numpy operation in ``dtype`` (rounded,
never fused):
    A[r][c] = (((0 + w_0 T[0][r][c]) + w_1 T[1][r][c]) + ...)          r < 3, all J terms
    p_r = (((A[r][0] x + A[r][1] y) + A[r][2] z) + A[r][3]) + trans_r
    out_r = p_r, or (Rinv[r][0] d_0 + Rinv[r][1] d_1) + Rinv[r][2] d_2 with d = p - t
Backward, from the per-set output gradients g_s:
    g' = Rinv^T g (same left-to-right order) or g;  grad_x_c = (A[0][c] g'_0 + A[1][c] g'_1) + A[2][c] g'_2
    G_v[r][c] = sum over sets, in order from +0, of g'_{s,r} x~_{s,c}, x~ = (x, y, z, 1)
    grad_T[j][r][c] = sum_v w_{v,j} G_v[r][c],  grad_trans[r] = sum_v G_v[r][3],  row 3 of grad_T = 0
both vertex sums two-level: chunks of CHUNK vertices summed sequentially from +0, the chunk partials in chunk order
from +0.  The loops run over j, over the positions inside a chunk and over the chunks; the vertices are vectorised."""
import numpy as np

CHUNK = 256      # EXA_SKIN_CHUNK


def gather_weights(weights, idx, V, dtype=np.float32):
    """[V, J] weight rows of every vertex; NaN rows for indices outside [0, Vw)."""
    dt = np.dtype(dtype).type
    weights = np.asarray(weights, dtype=dt)
    if idx is None:
        return weights[:V]
    idx = np.asarray(idx, dtype=np.int64)
    ok = (idx >= 0) & (idx < weights.shape[0])
    out = np.full((V, weights.shape[1]), np.nan, dtype=dt)
    out[ok] = weights[idx[ok]]
    return out


def blend(w, T, dtype=np.float32):
    """A [V, 3, 4]: the J-term sums, j ascending from +0."""
    dt = np.dtype(dtype).type
    T = np.asarray(T, dtype=dt)
    A = np.zeros((w.shape[0], 3, 4), dtype=dt)
    with np.errstate(invalid='ignore'):        # NaN rows and 0 * inf are part of the semantics
        for j in range(T.shape[0]):
            A = A + w[:, j, None, None] * T[j, :3, :]
    return A


def forward(points, T, weights, idx=None, trans=None, Rinv=None, t=None, dtype=np.float32):
    """points: list of [V, 3]; returns the list of posed [V, 3] in ``dtype``."""
    dt = np.dtype(dtype).type
    pts = [np.asarray(p, dtype=dt) for p in points]
    V = pts[0].shape[0]
    A = blend(gather_weights(weights, idx, V, dt), T, dt)
    tr = np.zeros(3, dtype=dt) if trans is None else np.asarray(trans, dtype=dt).reshape(3)
    outs = []
    for x in pts:
        p = [(((A[:, r, 0] * x[:, 0] + A[:, r, 1] * x[:, 1]) + A[:, r, 2] * x[:, 2]) + A[:, r, 3]) + tr[r]
             for r in range(3)]
        if Rinv is not None:
            R = np.asarray(Rinv, dtype=dt)
            tt = np.asarray(t, dtype=dt).reshape(3)
            d = [p[c] - tt[c] for c in range(3)]
            p = [(R[r, 0] * d[0] + R[r, 1] * d[1]) + R[r, 2] * d[2] for r in range(3)]
        outs.append(np.stack(p, 1))
    return outs


def chunked_sum(terms, dtype=np.float32):
    """Two-level sum over axis 0 of ``terms`` [V, ...]: chunks of CHUNK summed sequentially from +0, then the partials
    in chunk order from +0."""
    dt = np.dtype(dtype).type
    V = terms.shape[0]
    n = -(-V // CHUNK)
    part = np.zeros((n,) + terms.shape[1:], dtype=dt)
    for pos in range(CHUNK):
        rows = np.arange(n) * CHUNK + pos
        live = rows < V
        part[live] = part[live] + terms[rows[live]]
    total = np.zeros(terms.shape[1:], dtype=dt)
    for k in range(n):
        total = total + part[k]
    return total


def backward(points, grads, T, weights, idx=None, Rinv=None, dtype=np.float32):
    """grads: list of [V, 3] output gradients.  Returns (grad_points list, grad_T [J, 4, 4], grad_trans [3])."""
    dt = np.dtype(dtype).type
    pts = [np.asarray(p, dtype=dt) for p in points]
    V = pts[0].shape[0]
    T = np.asarray(T, dtype=dt)
    J = T.shape[0]
    w = gather_weights(weights, idx, V, dt)
    A = blend(w, T, dt)
    G = np.zeros((V, 3, 4), dtype=dt)
    gpts = []
    for x, g in zip(pts, grads):
        g = np.asarray(g, dtype=dt)
        if Rinv is not None:
            R = np.asarray(Rinv, dtype=dt)
            gp = np.stack([(R[0, c] * g[:, 0] + R[1, c] * g[:, 1]) + R[2, c] * g[:, 2] for c in range(3)], 1)
        else:
            gp = g
        gpts.append(np.stack([(A[:, 0, c] * gp[:, 0] + A[:, 1, c] * gp[:, 1]) + A[:, 2, c] * gp[:, 2]
                              for c in range(3)], 1))
        xt = np.concatenate([x, np.ones((V, 1), dtype=dt)], 1)
        G = G + gp[:, :, None] * xt[:, None, :]
    gT = np.zeros((J, 4, 4), dtype=dt)
    for j in range(J):
        gT[j, :3, :] = chunked_sum(w[:, j, None, None] * G, dt)
    gtrans = chunked_sum(G[:, :, 3], dt)
    return gpts, gT, gtrans


def magnitudes(points, grads, T, weights, idx=None, trans=None, Rinv=None, t=None):
    """float64 sums of the absolute values of every term that enters each output (the same expressions on |.|): the
    forward outputs, the point gradients, grad_T [J, 4, 4] and grad_trans [3]."""
    ab = lambda a: None if a is None else np.abs(np.asarray(a, dtype=np.float64))      # noqa: E731
    P, Gs = [ab(p) for p in points], [ab(g) for g in grads] if grads is not None else None
    w = np.abs(gather_weights(weights, idx, P[0].shape[0], np.float64))
    M = blend(w, ab(T), np.float64)
    tr = np.zeros(3) if trans is None else ab(trans).reshape(3)
    R = ab(Rinv)
    outs = []
    for x in P:
        p = M[:, :, :3] @ x[:, :, None]
        p = p[:, :, 0] + M[:, :, 3] + tr
        if R is not None:
            p = (p + ab(t).reshape(1, 3)) @ R.T
        outs.append(p)
    if Gs is None:
        return outs
    res = backward(P, Gs, ab(T), w, None, R, np.float64)
    return outs, res[0], res[1], res[2]


# ---- first-order error bounds: |fp32 - exact| <= K u * magnitude, K the roundings on the deepest path of a term ----
U = 2.0 ** -24


def k_forward(J):
    """J roundings in A (J products and J - 1 additions after the exact first one), 4 in q (a product and three
    additions), 1 for + trans, 1 for - t, 3 for the camera row (a product and two additions): J + 9."""
    return J + 9


def k_grad_points(J):
    """J in A, 3 in g' (camera row), 3 in grad_x (a product and two additions): J + 6."""
    return J + 6


def k_grad_sums(V, S):
    """3 in g', 1 product and S - 1 additions in G, 1 product w G, at most CHUNK - 1 additions inside a chunk and
    ceil(V / CHUNK) - 1 between the partials: S + 3 + CHUNK + ceil(V / CHUNK)."""
    return S + 3 + min(V, CHUNK) + max(1, -(-V // CHUNK))


def reference_expression(points, T, weights, idx=None, trans=None, R=None, t=None):
    """The reference's torch expression (module.py:413-422, 554-556) on whatever device and dtype the tensors have:
    the dense matmul of the gathered weights with T.view(J, 16), one bmm per set, + trans, inverse(R) (p - t)."""
    import torch
    J, V = T.shape[0], points[0].shape[0]
    sw = weights[idx, :] if idx is not None else weights
    tmv = torch.matmul(sw, T.view(J, 16)).view(V, 4, 4)
    outs = []
    for x in points:
        xyz = torch.cat((x, torch.ones_like(x[:, :1])), 1)
        xyz = torch.bmm(tmv, xyz[:, :, None]).view(V, 4)[:, :3]
        if trans is not None:
            xyz = xyz + trans
        if R is not None:
            xyz = torch.matmul(torch.inverse(R), (xyz - t.view(1, 3)).permute(1, 0)).permute(1, 0)
        outs.append(xyz)
    return outs
