"""numpy restatement of the fused MLP's semantics (include/exa_mlp.h, exavatar_release_amd/mlp.py), independent of the
HIP code and of the reference's torch expression.

In float32 every operation is one numpy float32 operation (rounded to nearest even) and every fused multiply-add is
``fma32``: the product exact in float64, the sum by TwoSum, rounded to odd at 53 bits, then cast to float32 -- which
is the correctly rounded fmaf.  In float64 the same loops run with plain float64 operations (the fused multiply-adds
become a product and a sum), so that the restatement can be checked against the reference's module and autograd.

Net: ``layers`` a list of dicts {W [128, K], b, gamma, beta [128], G, eps}, layer 0's W holding the per-row columns
only; ``Ws`` [128, S] and ``p`` [S] the shared block (or None); ``Wh`` [nh, 128], ``bh`` [nh] the stacked heads.
The rows are vectorised; the loops run over k, over the channels of a group and over the rows of a chunk."""
import numpy as np

CHUNK = 512      # EXA_MLP_CHUNK
H = 128


def fma32(a, b, c):
    """Correctly rounded float32 fma(a, b, c), elementwise with broadcasting."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        p = a * b                                    # exact: 24 + 24 bits
        s = p + c
        bp = s - c
        e = (p - bp) + (c - (s - bp))                # TwoSum: p + c == s + e exactly
        fix = np.isfinite(s) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)   # round to odd
        return s.astype(np.float32)


def korder(K):
    """The header's pi(K) over K zero-padded to a multiple of 8 (indices >= K are the zero terms)."""
    Kp = (K + 7) // 8 * 8
    return [8 * q + j + 4 * hh for q in range(Kp // 8) for j in range(4) for hh in (0, 1)]


def _fma(a, b, c, dt):
    if dt == np.float32:
        return fma32(a, b, c)
    return c + a * b


def linear(W, X, init, dt):
    """out[n, j] = chain over k in pi(K) of fma(W[j, k], X[n, k], acc) from init[n, j]; W [M, K], X [N, K]."""
    W = np.asarray(W, dt)
    X = np.asarray(X, dt)
    K = W.shape[1]
    acc = np.array(init, dt, copy=True)
    zero = dt(0)
    for k in korder(K):
        if k < K:
            acc = _fma(W[None, :, k], X[:, k, None], acc, dt)
        else:
            acc = acc + zero
    return acc


def _half_channels(G):
    """For each group, the channel lists of lane half 0 and 1 in the header's order."""
    tpg = 4 // G
    out = []
    for g in range(G):
        halves = []
        for h in (0, 1):
            halves.append([32 * t + (r & 3) + 8 * (r >> 2) + 4 * h for t in range(g * tpg, (g + 1) * tpg)
                           for r in range(16)])
        out.append(halves)
    return out


def group_sum(V, G, dt):
    """[N, G] group sums of V [N, 128] in the header's order."""
    out = np.zeros((V.shape[0], G), dt)
    for g, halves in enumerate(_half_channels(G)):
        s = []
        for chans in halves:
            acc = np.zeros(V.shape[0], dt)
            for c in chans:
                acc = acc + V[:, c]
            s.append(acc)
        out[:, g] = s[0] + s[1]
    return out


def _expand(v, G):
    return np.repeat(v, H // G, axis=1)


def relu(y):
    return np.where((y > 0) | np.isnan(y), y, y.dtype.type(0))


def gn_forward(z, gamma, beta, G, eps, dt):
    n = dt(H // G)
    mean = group_sum(z, G, dt) / n
    d = z - _expand(mean, G)
    var = group_sum(d * d, G, dt) / n
    rstd = dt(1) / np.sqrt(var + dt(eps))
    xhat = d * _expand(rstd, G)
    y = xhat * np.asarray(gamma, dt)[None] + np.asarray(beta, dt)[None]
    return xhat, rstd, y


def folded_bias(net, dt):
    b = np.asarray(net['layers'][0]['b'], dt).copy()
    if net.get('p') is not None:
        Ws = np.asarray(net['Ws'], dt)
        p = np.asarray(net['p'], dt)
        for c in range(p.shape[0]):
            b = _fma(Ws[:, c], p[c], b, dt)
    return b


def forward(net, x, dtype=np.float32, keep=False):
    """Head outputs [N, nh] (and, with keep, the per-layer inputs, xhat, rstd and y)."""
    dt = np.dtype(dtype).type
    x = np.asarray(x, dt)
    N = x.shape[0]
    a = x
    saved = []
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for l, L in enumerate(net['layers']):
            bias = folded_bias(net, dt) if l == 0 else np.asarray(L['b'], dt)
            z = linear(L['W'], a, np.broadcast_to(bias[None], (N, H)), dt)
            xhat, rstd, y = gn_forward(z, L['gamma'], L['beta'], L['G'], L['eps'], dt)
            saved.append({'in': a, 'xhat': xhat, 'rstd': rstd, 'y': y})
            a = relu(y)
        bh = np.asarray(net['bh'], dt)
        out = linear(net['Wh'], a, np.broadcast_to(bh[None], (N, bh.shape[0])), dt)
    return (out, saved, a) if keep else out


def _chunk_sum_terms(T, dt):
    """Two-level sum over axis 0 of per-row terms T [N, ...]: chunks summed from +0 in row order, then chunk order."""
    N = T.shape[0]
    tot = np.zeros(T.shape[1:], dt)
    for c0 in range(0, N, CHUNK):
        acc = np.zeros(T.shape[1:], dt)
        for r in range(c0, min(N, c0 + CHUNK)):
            acc = acc + T[r]
        tot = tot + acc
    return tot


def _chunk_sum_outer(A, B, dt):
    """grad[j, k] = two-level sum over rows of fma(A[r, j], B[r, k], acc); a chunk with an odd number of rows gets one
    trailing zero row.  The chunks run vectorised."""
    N = A.shape[0]
    nch = (N + CHUNK - 1) // CHUNK
    pad = nch * CHUNK - N
    A = np.concatenate([A, np.zeros((pad, A.shape[1]), dt)]).reshape(nch, CHUNK, A.shape[1])
    B = np.concatenate([B, np.zeros((pad, B.shape[1]), dt)]).reshape(nch, CHUNK, B.shape[1])
    rows = np.array([min(CHUNK, N - c * CHUNK) for c in range(nch)])
    steps = (rows + 1) // 2 * 2                       # rows of each chunk's chain, an odd count padded by one zero row
    acc = np.zeros((nch, A.shape[2], B.shape[2]), dt)
    for r in range(CHUNK):
        live = r < steps                              # rows past a chunk's padded end are not part of its chain
        if not live.any():
            break
        acc = np.where(live[:, None, None], _fma(A[:, r, :, None], B[:, r, None, :], acc, dt), acc)
    tot = np.zeros(acc.shape[1:], dt)
    for c in range(nch):
        tot = tot + acc[c]
    return tot


def backward(net, x, gout, dtype=np.float32):
    """Gradients from gout [N, nh]: dict with 'x' [N, K0], 'layers' (list of dicts W, b, gamma, beta), 'Wh', 'bh',
    and 'Ws' when the net has a shared block."""
    dt = np.dtype(dtype).type
    x = np.asarray(x, dt)
    gout = np.asarray(gout, dt)
    N = x.shape[0]
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        _, saved, aL = forward(net, x, dt, keep=True)
        Wh = np.asarray(net['Wh'], dt)
        dA = linear(Wh.T, gout, np.zeros((N, H), dt), dt)
        g = {'Wh': _chunk_sum_outer(gout, aL, dt), 'bh': _chunk_sum_terms(gout, dt), 'layers': [None] * len(saved)}
        for l in range(len(saved) - 1, -1, -1):
            L, s = net['layers'][l], saved[l]
            G = L['G']
            n = dt(H // G)
            gamma = np.asarray(L['gamma'], dt)
            dY = np.where(s['y'] > 0, dA, dt(0))
            e = dY * gamma[None]
            m1 = group_sum(e, G, dt) / n
            m2 = group_sum(e * s['xhat'], G, dt) / n
            dZ = _expand(s['rstd'], G) * ((e - _expand(m1, G)) - s['xhat'] * _expand(m2, G))
            W = np.asarray(L['W'], dt)
            g['layers'][l] = {'W': _chunk_sum_outer(dZ, s['in'], dt), 'b': _chunk_sum_terms(dZ, dt),
                              'gamma': _chunk_sum_terms(dY * s['xhat'], dt), 'beta': _chunk_sum_terms(dY, dt)}
            dA = linear(W.T, dZ, np.zeros((N, W.shape[1]), dt), dt)
        g['x'] = dA
        if net.get('p') is not None:
            g['Ws'] = g['layers'][0]['b'][:, None] * np.asarray(net['p'], dt)[None, :]
    return g


def net_from_modules(layers, heads, per_row_cols, shared_cols=None, p=None, dtype=np.float32):
    """The oracle's net from torch modules: ``layers`` [(Linear, GroupNorm)], ``heads`` [Linear]; ``per_row_cols`` and
    ``shared_cols`` lists of layer 0's column indices."""
    def arr(t):
        return t.detach().cpu().numpy().astype(dtype)
    out = {'layers': []}
    for l, (lin, gn) in enumerate(layers):
        W = arr(lin.weight)
        out['layers'].append({'W': W[:, per_row_cols] if l == 0 else W, 'b': arr(lin.bias), 'gamma': arr(gn.weight),
                              'beta': arr(gn.bias), 'G': gn.num_groups, 'eps': gn.eps})
    if shared_cols:
        out['Ws'] = arr(layers[0][0].weight)[:, shared_cols]
        out['p'] = np.asarray(p, dtype)
    out['Wh'] = np.concatenate([arr(h.weight) for h in heads])
    out['bh'] = np.concatenate([arr(h.bias) for h in heads])
    return out
