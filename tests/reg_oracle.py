"""CPU oracles of the arm and hand regularisers (include/exa_mesh.h, exavatar_release_amd/vertex_regs.py).

(a) ``*32``: the header's arithmetic restated in numpy float32, one array operation per rounded operation and an explicit
    loop wherever the header states an order (the k neighbours of the arm target, the rows of a chunk and the chunks of the
    hand means).  numpy evaluates ``a * b`` and ``c + p`` as two separately rounded array operations, so no product is
    fused into an add and no sum is re-associated: the results are what the kernels must give bit for bit.

(b) ``*64``: the same functions of the same float32 inputs in float64 -- exact for the purpose -- returning next to every
    output a first-order bound on the error of a float32 evaluation of it.  With u = 2^-24:

    * arm target.  ``target = (sum of k rows) / k``.  In ANY order of summation a term passes through at most k - 1
      additions; the division rounds once, or twice where it is a product with a rounded reciprocal: at most k + 1
      roundings, so to first order  |fl(target) - target| <= (k + 1) u (sum_j |rgb_j|) / k =: E_t.  The neighbour SET is
      not a matter of rounding: it is decided on the keys, and a wrong set moves a target by about |rgb| / k ~ 1e-2,
      five orders above E_t ~ 1e-7.
    * arm d, loss, gradient.  d = rgb - target rounds once: E_d = E_t + u |d|.  loss = d d: E_loss = 2 |d| E_d + u d^2.
      grad = (2 d) g, 2 d exact, one product: E_grad = 2 |g| E_d + u |grad|.
    * hand means.  The header's two-level sum passes a term through at most min(N, 256) - 1 additions inside its chunk
      and chunks - 1 additions of partials, and the division rounds once (twice as a product with a reciprocal):
      R = min(N, 256) + chunks roundings at most,  E_m = R u (sum_i |rgb_i|) / N.  For N <= 256 (one chunk, R = N + 1)
      that covers every order of summation, PyTorch's ``mean`` included; beyond, it covers every summation that is no
      deeper than R, which a pairwise or cascaded sum is.
    * hand rgb loss and gradient.  dr = rgb - mean_r: E_dr = E_m + u |dr|, likewise dl.  loss = dr dr + dl dl:
      E_loss = (2 |dr| E_dr + u dr^2) + (2 |dl| E_dl + u dl^2) + u loss.  A gradient term g (2 dr):
      E = 2 |g| E_dr + u |term|; a vertex in both lists adds the two bounds and u |grad|.
    * hand mean.  o.o is three rounded squares and two additions (3 u relative), the root halves that and rounds once
      (2.5 u), q = o / s once more (3.5 u); each n_c q_c rounds once and passes at most two additions:
      E_dot = 7 u sum_c |n_c q_c|, and clamp(min=0) does not stretch it.  The gradient a_c + o_c w with
      a_c = g n_c / s and w = -(sum_c' g n_c' q_c' / s) / norm: fewer than 16 roundings on the way to either term,
      E_grad = 16 u (|g n_c| / s + |o_c| (sum_c' |g n_c' q_c'|) / (s norm)), the second part only where norm >= eps.
      Where |dot| <= E_dot two evaluations may clamp differently and where norm is within 3 u of eps they may pass the
      norm's gradient differently; such rows are reported (``unsure``) and left to the float32 oracle alone.

    The bounds hold for the reference's own order of operations too, so two float32 evaluations differ by at most twice
    the bound; tests/test_reg_oracle.py checks them against the reference's own recorded float32-vs-float64 error.
"""
import numpy as np

U = 2.0 ** -24
CHUNK = 256
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
F32 = np.float32


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


# ---- arm ---------------------------------------------------------------------------------------------------------------
def arm_plan32(mesh, is_upper, is_lower, dist_x_thr=0.01, top_k=50):
    """-> dict(upper [U], lower [L], nbr [L, top_k] int32 (-1 where a row has fewer), n_valid [L], n_min, k)."""
    mesh = _f32(mesh)
    up, lo = np.nonzero(is_upper)[0], np.nonzero(is_lower)[0]
    thr = F32(dist_x_thr)
    a, b = mesh[lo], mesh[up]
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    valid = np.abs(dx) < thr
    with np.errstate(over='ignore', invalid='ignore'):
        xx, yy, zz = dx * dx, dy * dy, dz * dz
        s = xx + yy
        d2 = s + zz
    bits = d2.view(np.uint32).astype(np.uint64)
    bits[np.isnan(d2)] = 0x7fc00000
    key = (bits << np.uint64(32)) | up[None, :].astype(np.uint64)
    key[~valid] = EMPTY
    n = valid.sum(1).astype(np.int32)
    n_min = int(n.min()) if lo.size else 0
    k = min(int(top_k), n_min)
    srt = np.sort(key, axis=1)[:, :top_k]
    nbr = np.full((lo.size, top_k), -1, dtype=np.int32)
    got = (srt & np.uint64(0xFFFFFFFF)).astype(np.int64)
    got[srt == EMPTY] = -1
    nbr[:, :srt.shape[1]] = got
    return dict(upper=up, lower=lo, nbr=nbr, n_valid=n, n_min=n_min, k=k, V=mesh.shape[0], top_k=int(top_k))


def arm_loss32(plan, rgb):
    """-> (loss, d), float32 [B, V, 3]: the reference's loss on the lower rows, +0 elsewhere."""
    rgb = _f32(rgb)
    lo, k = plan['lower'], plan['k']
    t = np.zeros((rgb.shape[0], lo.size, 3), dtype=np.float32)
    for j in range(k):
        t = t + rgb[:, plan['nbr'][:, j], :]
    with np.errstate(invalid='ignore', divide='ignore'):
        target = t / F32(k)
    dl = rgb[:, lo, :] - target
    d = np.zeros_like(rgb)
    loss = np.zeros_like(rgb)
    d[:, lo, :] = dl
    loss[:, lo, :] = dl * dl
    return loss, d


def arm_grad32(plan, d, grad_loss):
    """-> dL/drgb, float32 [B, V, 3]."""
    d, g = _f32(d), _f32(grad_loss)
    lo = plan['lower']
    grad = np.zeros_like(d)
    grad[:, lo, :] = (F32(2.0) * d[:, lo, :]) * g[:, lo, :]
    return grad


def arm_forward64(plan, rgb, grad_loss=None):
    """-> dict(loss, E_loss, d, E_d[, grad, E_grad]) on the LOWER rows only, float64 [B, L, 3]; the neighbour sets are
    the plan's."""
    x = np.asarray(rgb, dtype=np.float64)
    lo, k = plan['lower'], plan['k']
    rows = x[:, plan['nbr'][:, :k], :]                      # [B, L, k, 3]
    with np.errstate(invalid='ignore', divide='ignore'):
        target = rows.sum(2) / k
        E_t = (k + 1) * U * np.abs(rows).sum(2) / k
    d = x[:, lo, :] - target
    E_d = E_t + U * np.abs(d)
    out = dict(loss=d * d, E_loss=2 * np.abs(d) * E_d + U * d * d, d=d, E_d=E_d)
    if grad_loss is not None:
        g = np.asarray(grad_loss, dtype=np.float64)
        out['grad'] = 2 * d * g
        out['E_grad'] = 2 * np.abs(g) * E_d + U * np.abs(out['grad'])
    return out


# ---- hand rgb ----------------------------------------------------------------------------------------------------------
def index_tables(mask):
    """(ascending indices [n] int32, inverse ranks [V] int32: position in the list, -1 outside)."""
    idx = np.nonzero(mask)[0].astype(np.int32)
    rank = np.full(len(mask), -1, dtype=np.int32)
    rank[idx] = np.arange(idx.size, dtype=np.int32)
    return idx, rank


def two_level_mean32(rows):
    """rows [B, N, 3] float32 in list order -> [B, 3]: chunks of 256 summed sequentially from +0, the partials summed
    sequentially from +0, divided by float(N)."""
    rows = _f32(rows)
    B, N = rows.shape[0], rows.shape[1]
    s = np.zeros((B, 3), dtype=np.float32)
    for c0 in range(0, N, CHUNK):
        p = np.zeros((B, 3), dtype=np.float32)
        for i in range(c0, min(c0 + CHUNK, N)):
            p = p + rows[:, i, :]
        s = s + p
    with np.errstate(invalid='ignore', divide='ignore'):
        return s / F32(N)


def hand_rgb32(rgb, is_rhand, is_lhand):
    """-> (loss [B, N, 3], means [B, 2, 3])."""
    rgb = _f32(rgb)
    r, l = index_tables(is_rhand)[0], index_tables(is_lhand)[0]
    mr, ml = two_level_mean32(rgb[:, r, :]), two_level_mean32(rgb[:, l, :])
    dr, dl = rgb[:, r, :] - mr[:, None, :], rgb[:, l, :] - ml[:, None, :]
    a, b = dr * dr, dl * dl
    return a + b, np.stack([mr, ml], 1)


def hand_rgb_grad32(rgb, means, grad_loss, is_rhand, is_lhand):
    """-> dL/drgb [B, V, 3]: right term, then left term; the term alone in one list; +0 in neither."""
    rgb, means, g = _f32(rgb), _f32(means), _f32(grad_loss)
    r, l = index_tables(is_rhand)[0], index_tables(is_lhand)[0]
    tr = g * (F32(2.0) * (rgb[:, r, :] - means[:, None, 0, :]))
    tl = g * (F32(2.0) * (rgb[:, l, :] - means[:, None, 1, :]))
    grad = np.zeros_like(rgb)
    grad[:, r, :] = tr
    full_l = np.zeros_like(rgb)
    full_l[:, l, :] = tl
    both = np.nonzero(np.asarray(is_rhand) & np.asarray(is_lhand))[0]
    only_l = np.nonzero(~np.asarray(is_rhand) & np.asarray(is_lhand))[0]
    grad[:, only_l, :] = full_l[:, only_l, :]
    grad[:, both, :] = grad[:, both, :] + full_l[:, both, :]
    return grad


def hand_rgb64(rgb, is_rhand, is_lhand, grad_loss=None):
    """-> dict(loss, E_loss[, grad, E_grad]); float64, loss [B, N, 3], grad [B, V, 3]."""
    x = np.asarray(rgb, dtype=np.float64)
    r, l = index_tables(is_rhand)[0], index_tables(is_lhand)[0]
    N = r.size
    R = min(N, CHUNK) + (N + CHUNK - 1) // CHUNK
    d, E = {}, {}
    for name, idx in (('r', r), ('l', l)):
        rows = x[:, idx, :]
        m = rows.mean(1, keepdims=True)
        E_m = R * U * np.abs(rows).sum(1, keepdims=True) / N
        d[name] = rows - m
        E[name] = E_m + U * np.abs(d[name])
    loss = d['r'] ** 2 + d['l'] ** 2
    E_loss = sum(2 * np.abs(d[n]) * E[n] + U * d[n] ** 2 for n in 'rl') + U * loss
    out = dict(loss=loss, E_loss=E_loss)
    if grad_loss is not None:
        g = np.asarray(grad_loss, dtype=np.float64)
        grad, E_grad = np.zeros_like(x), np.zeros_like(x)
        for name, idx in (('r', r), ('l', l)):
            t = g * 2 * d[name]
            np.add.at(grad, (slice(None), idx), t)
            np.add.at(E_grad, (slice(None), idx), 2 * np.abs(g) * E[name] + U * np.abs(t))
        out['grad'], out['E_grad'] = grad, E_grad + U * np.abs(grad)
    return out


# ---- hand mean ---------------------------------------------------------------------------------------------------------
EPS32 = F32(1e-12)


def _hand_dot32(o, n):
    with np.errstate(over='ignore', invalid='ignore', divide='ignore', under='ignore'):
        norm = np.sqrt((o[..., 0] * o[..., 0] + o[..., 1] * o[..., 1]) + o[..., 2] * o[..., 2])
        s = np.where(norm < EPS32, EPS32, norm).astype(np.float32)
        q = o / s[..., None]
        dot = (n[..., 0] * q[..., 0] + n[..., 1] * q[..., 1]) + n[..., 2] * q[..., 2]
    return norm, s, q, dot


def hand_mean32(offset, normal, is_rhand, is_lhand):
    """-> loss [B, H] over the union of the masks, ascending."""
    h = index_tables(np.asarray(is_rhand) | np.asarray(is_lhand))[0]
    o, n = _f32(offset)[:, h, :], _f32(normal).reshape(-1, 3)[None, h, :]
    dot = _hand_dot32(o, n)[3]
    return np.where(dot < 0, F32(0.0), dot).astype(np.float32)


def hand_mean_grad32(offset, normal, grad_loss, is_rhand, is_lhand):
    """-> dL/doffset [B, V, 3]."""
    offset = _f32(offset)
    h = index_tables(np.asarray(is_rhand) | np.asarray(is_lhand))[0]
    o, n = offset[:, h, :], _f32(normal).reshape(-1, 3)[None, h, :]
    norm, s, q, dot = _hand_dot32(o, n)
    g = np.where(dot >= 0, _f32(grad_loss), F32(0.0)).astype(np.float32)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore', under='ignore'):
        dq = g[..., None] * n
        a = dq / s[..., None]
        qs = q / s[..., None]
        t = (dq[..., 0] * qs[..., 0] + dq[..., 1] * qs[..., 1]) + dq[..., 2] * qs[..., 2]
        w = (-t) / norm
        full = a + o * w[..., None]
    rows = np.where((norm >= EPS32)[..., None], full, a).astype(np.float32)
    grad = np.zeros_like(offset)
    grad[:, h, :] = rows
    return grad


def hand_mean64(offset, normal, is_rhand, is_lhand, grad_loss=None):
    """-> dict(loss, E_loss, unsure [B, H] bool[, grad, E_grad on the hand rows [B, H, 3]]), float64."""
    h = index_tables(np.asarray(is_rhand) | np.asarray(is_lhand))[0]
    o = np.asarray(offset, dtype=np.float64)[:, h, :]
    n = np.asarray(normal, dtype=np.float64).reshape(-1, 3)[None, h, :]
    eps = 1e-12
    norm = np.sqrt((o * o).sum(-1))
    s = np.maximum(norm, eps)
    q = o / s[..., None]
    dot = (n * q).sum(-1)
    E_dot = 7 * U * np.abs(n * q).sum(-1)
    unsure = ((np.abs(dot) <= E_dot) & (dot != 0)) | (np.abs(norm - eps) <= 3 * U * eps)
    out = dict(loss=np.maximum(dot, 0), E_loss=E_dot, unsure=unsure)
    if grad_loss is not None:
        g = np.where(dot >= 0, np.asarray(grad_loss, dtype=np.float64), 0.0)
        dq = g[..., None] * n
        a = dq / s[..., None]
        passes = norm >= eps
        with np.errstate(invalid='ignore', divide='ignore'):
            t = (dq * q).sum(-1) / s
            T = np.abs(dq * q).sum(-1) / s
            full = a + o * (-t / norm)[..., None]
            E_full = np.abs(o) * (T / norm)[..., None]
        out['grad'] = np.where(passes[..., None], full, a)
        out['E_grad'] = 16 * U * (np.abs(a) + np.where(passes[..., None], E_full, 0.0))
    return out


# ---- test meshes -------------------------------------------------------------------------------------------------------
def two_tube_arms(rings, per_ring, seed, extra=37):
    """Two tubes along x, the "arms", starting at x0 = +0.2 and x0 = -0.2: ring spacing 0.004, radius 0.04, every
    coordinate jittered by +-5e-4 (so every |dx| stays 1e-3 away from the 0.01 threshold), then ``extra`` vertices in
    front that belong to no arm.  Upper = the radial direction's y above 0.5.  -> (mesh [V, 3] float32, is_upper,
    is_lower)."""
    rng = np.random.RandomState(seed)
    pts, upper = [], []
    theta = 2 * np.pi * np.arange(per_ring) / per_ring
    for x0 in (0.2, -0.2):
        for r in range(rings):
            x = x0 + 0.004 * r * np.sign(x0)
            pts.append(np.stack([np.full(per_ring, x), 0.04 * np.sin(theta), 0.04 * np.cos(theta)], 1))
            upper.append(np.sin(theta) > 0.5)
    pts = np.concatenate(pts)
    pts = pts + rng.uniform(-5e-4, 5e-4, size=pts.shape)
    upper = np.concatenate(upper)
    front = np.stack([rng.uniform(-0.1, 0.1, extra), rng.uniform(-0.1, 0.1, extra), rng.uniform(0.3, 0.4, extra)], 1)
    mesh = np.concatenate([pts, front]).astype(np.float32)
    is_upper = np.concatenate([upper, np.zeros(extra, dtype=bool)])
    is_lower = np.concatenate([~upper, np.zeros(extra, dtype=bool)])
    return mesh, is_upper, is_lower


def grid_faces(rows, cols):
    """Two triangles per cell of a rows x cols vertex grid."""
    r, c = np.meshgrid(np.arange(rows - 1), np.arange(cols - 1), indexing='ij')
    a = (r * cols + c).reshape(-1)
    return np.concatenate([np.stack([a, a + 1, a + cols], 1), np.stack([a + 1, a + cols + 1, a + cols], 1)]).astype(np.int64)
