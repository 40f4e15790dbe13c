"""numpy restatement of the fitting loss's mesh terms (include/exa_mesh.h "Mesh terms of the fitting loss",
exavatar_release_amd/fit_terms.py), independent of the HIP code and of the reference's torch expressions.

Every function takes a ``dtype``: in float32 every line below is one numpy operation, rounded and never fused, in the
header's order -- what the kernels are held to bit for bit; in float64 the same lines are the exact semantics.  The
backward sums run "by rank": all first contributions of every vertex are added at once, then all second ones, .. which
adds each vertex's contributions in the header's order (ascending slot of the transposed table) without a Python loop
over vertices.  The transposed tables are built here with a stable argsort, independently of the library's.

Bounds against the reference's own float32 run (tests/test_fit_oracle.py), U = 2^-24, first order
----------------------------------------------------------------------------------------------
The reference leaves three sums to torch, whose order is not ours to state: ``sum((x_a - x_b) ** 2, 2)`` (edge), ``sum(x *
bc, 2)`` (symmetry) -- three terms each -- and ``mean(1)`` over V (centred term).  Everything else in the four expressions is
elementwise or written as ``a + b + c``, which Python evaluates as ``(a + b) + c``: the header's order.  Where torch's order
turns out to be the header's the maps coincide bit for bit, and the tests assert that: it is so for the symmetry term
(``(r0 w0 + r1 w1) + r2 w2``, on the CPU and on the device).  For the edge term torch adds the three squares in another
order, for the centred term its mean does, and for ``PoseLoss`` sin / cos are another library's: those are held to the
bounds below, which also cover the symmetry term should equality ever be lost.

* ``edge_bound``.  Any order of three non-negative terms makes two additions, each within U of its exact partial sum <= S:
  two orders differ by <= 4 U S.  The square root halves the relative error and rounds once on each side: d differs by
  <= 2 U d + 2 U d = 4 U d.  ``|d_out - d_gt| * m`` then differs by <= m 4 U (d_out + d_gt) plus one rounding of the
  subtraction and one of the product on each side, 4 U loss.
* ``sym_bound``.  Two orders of the three products r_k w_k differ by <= 4 U M_c, M_c = sum_k |r_k w_k|; p +- f rounds once
  per side (2 U |d_c|), the two additions of the three absolute values are in the same order on both sides, so they only
  carry the differences through: <= sum_c (4 U M_c + 2 U |d_c|) + 4 U loss (two additions per side).
* ``v2v_bound``.  A sum of V terms in ANY order is within (V - 1) U sum |x| of the exact sum; the header's is within
  depth U sum |x| (``v2v_depth``); the division rounds once per side.  So each mean differs by <= (V + depth + 1) U mean |x|,
  e by that for both means plus its three subtractions per side, 6 U (|a| + |ma| + |t| + |mt|), and the map by
  ``w * scale`` times that plus two products per side, 4 U loss.
* ``POSE_K``.  An entry of R passes, per side, through: the squared norm and its root (3.5 U), the half (exact), sinf /
  cosf (2 U each, a device library), s (1 U), s x (1 U), n (4 additions and 4 products of terms <= 1: 8 U), 2 / n (1 U), two
  products and a sum (3 U, magnitudes <= 2), the product with t and the final subtraction (2 U): under 32 U in all on
  values <= 2.  Two matrices on two sides and the subtraction: |oracle - reference| <= POSE_K U with POSE_K = 4 * 32 + 2.
"""
import numpy as np

from tests import sum_oracle

F32 = np.float32
U = 2.0 ** -24
SMALL = 1e-6
BLOCK = 256
EDGE_A, EDGE_B = (0, 0, 1), (1, 2, 2)          # the corners (a, b) of edge k
POSE_K = 4 * 32 + 2


def sign(x):
    return ((x > 0).astype(x.dtype) - (x < 0).astype(x.dtype)).astype(x.dtype)


def transpose(idx, n_targets):
    """(offsets [n_targets + 1], entries): for every target the flat slots of ``idx`` that name it, ascending; -1 names none."""
    flat = np.asarray(idx).reshape(-1)
    order = np.argsort(flat, kind='stable')
    order = order[flat[order] >= 0]
    counts = np.bincount(flat[order], minlength=n_targets)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), order.astype(np.int32)


def add_by_rank(acc, target, contrib):
    """acc[:, target[n]] += contrib[:, n] for n in order, one rank at a time: ``target`` is sorted by target, so the n-th
    contribution of every target is added before any (n + 1)-th one, each target's in their order."""
    target = np.asarray(target)
    if target.size == 0:
        return acc
    first = np.concatenate([[True], target[1:] != target[:-1]])
    start = np.maximum.accumulate(np.where(first, np.arange(target.size), 0))
    rank = np.arange(target.size) - start
    for r in range(int(rank.max()) + 1):
        sel = np.nonzero(rank == r)[0]
        acc[:, target[sel]] = acc[:, target[sel]] + contrib[:, sel]
    return acc


# ---- edge length ------------------------------------------------------------------------------------------------------
def _lengths(x, a, b):
    diff = x[:, a, :] - x[:, b, :]
    return np.sqrt((diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]), diff


def edge_forward(out, gt, valid, face, dtype=F32):
    """out [B, V, 3], gt [B or 1, V, 3], valid [B or 1, V], face [F, 3] -> [B, 3F, 1]."""
    out, gt, valid = (np.asarray(x, dtype=dtype) for x in (out, gt, valid))
    face = np.asarray(face).reshape(-1, 3)
    parts = []
    for k in range(3):
        a, b = face[:, EDGE_A[k]], face[:, EDGE_B[k]]
        d_out, d_gt = _lengths(out, a, b)[0], _lengths(gt, a, b)[0]
        parts.append(np.abs(d_out - d_gt) * (valid[:, a] * valid[:, b]))
    return np.concatenate(parts, 1)[..., None].astype(dtype)


def edge_backward(out, gt, valid, face, g, dtype=F32, magnitude=False):
    """dL/dout [B, V, 3] for the cotangent g [B, 3F, 1]; an edge with d_out == 0 contributes +0.  With ``magnitude`` the sum
    of the contributions' absolute values instead (what a first-order bound multiplies by K U)."""
    out, gt, valid, g = (np.asarray(x, dtype=dtype) for x in (out, gt, valid, g))
    face = np.asarray(face).reshape(-1, 3)
    B, V, F = out.shape[0], out.shape[1], face.shape[0]
    acc = np.zeros((B, V, 3), dtype=dtype)
    if F == 0 or B == 0:
        return acc
    _, entries = transpose(face, V)
    f, corner = entries // 3, entries % 3
    # the two edges of a corner in ascending k, and whether the corner is the edge's a
    k = np.stack([np.where(corner == 2, 1, 0), np.where(corner == 0, 1, 2)], 1).reshape(-1)
    f2, corner2 = np.repeat(f, 2), np.repeat(corner, 2)
    a = face[f2, np.asarray(EDGE_A)[k]]
    b = face[f2, np.asarray(EDGE_B)[k]]
    is_a = np.asarray(EDGE_A)[k] == corner2
    d_out, diff = _lengths(out, a, b)
    d_gt = _lengths(gt, a, b)[0]
    m = valid[:, a] * valid[:, b]
    gk = g.reshape(B, 3 * F)[:, k * F + f2]
    with np.errstate(divide='ignore', invalid='ignore'):
        t = ((gk * m) * sign(d_out - d_gt)) / d_out
        q = np.where((d_out == 0)[..., None], dtype(0), t[..., None] * diff)
    q = np.abs(q) if magnitude else np.where(is_a[None, :, None], q, -q)
    return add_by_rank(acc, face[f2, corner2], q)


def edge_bound(out, gt, valid, face):
    """[B, 3F, 1] float64: the bound on |oracle32 - reference32| of the module docstring."""
    o = edge_forward(out, gt, valid, face, np.float64)
    out, gt, valid = (np.asarray(x, dtype=np.float64) for x in (out, gt, valid))
    face = np.asarray(face).reshape(-1, 3)
    parts = []
    for k in range(3):
        a, b = face[:, EDGE_A[k]], face[:, EDGE_B[k]]
        parts.append((valid[:, a] * valid[:, b]) * 4 * U * (_lengths(out, a, b)[0] + _lengths(gt, a, b)[0]))
    return np.concatenate(parts, 1)[..., None] + 4 * U * o


def edge_ambiguous(out, gt, face, rel=1e-5):
    """[B, V] bool: vertices with an incident edge whose sign decision d_out - d_gt lies within ``rel`` of zero in float64,
    exact ties (and zero-length edges, which contribute nothing) excepted."""
    out, gt = np.asarray(out, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    face = np.asarray(face).reshape(-1, 3)
    bad = np.zeros(out.shape[:2], dtype=bool)
    for k in range(3):
        a, b = face[:, EDGE_A[k]], face[:, EDGE_B[k]]
        d_out, d_gt = _lengths(out, a, b)[0], _lengths(gt, a, b)[0]
        amb = (np.abs(d_out - d_gt) <= rel * np.maximum(d_out, d_gt)) & (d_out != d_gt) & (d_out != 0)
        for e in (a, b):
            np.logical_or.at(bad, (np.nonzero(amb)[0], e[np.nonzero(amb)[1]]), True)
    return bad


# ---- flip symmetry ----------------------------------------------------------------------------------------------------
def flip_plan(vertex_num, face_vertex_idx, closest_faces, bc):
    """(taps [Vf, 3] in [-1, Vf), weights [Vf, 3], offsets [Vf + 1], entries) as the header documents them."""
    fvi = np.asarray(face_vertex_idx, dtype=np.int64)
    row = np.full(vertex_num, -1, dtype=np.int64)
    row[fvi] = np.arange(fvi.size)
    taps = row[np.asarray(closest_faces, dtype=np.int64)[fvi]].astype(np.int32).reshape(-1, 3)
    weights = np.asarray(bc, dtype=F32)[fvi].reshape(-1, 3)
    offsets, entries = transpose(taps, fvi.size)
    return taps, weights, offsets, entries


def _sym_terms(p, taps, weights, rows=None, magnitude=False):
    """d [B, n, 3] of ``rows`` (all rows by default): d_0 = p_0 + f_0, d_c = p_c - f_c; with ``magnitude`` M_c instead."""
    rows = np.arange(taps.shape[0]) if rows is None else rows
    dt = p.dtype.type
    r = [np.where((taps[rows, k] < 0)[None, :, None], dt(0), p[:, np.maximum(taps[rows, k], 0), :]) for k in range(3)]
    w = [weights[rows, k].astype(p.dtype)[None, :, None] for k in range(3)]
    if magnitude:
        return (np.abs(r[0] * w[0]) + np.abs(r[1] * w[1])) + np.abs(r[2] * w[2])
    f = (r[0] * w[0] + r[1] * w[1]) + r[2] * w[2]
    x = p[:, rows, :]
    return np.stack([x[..., 0] + f[..., 0], x[..., 1] - f[..., 1], x[..., 2] - f[..., 2]], -1)


def sym_forward(p, taps, weights, dtype=F32):
    """p [B, Vf, 3] -> [B, Vf]."""
    d = _sym_terms(np.asarray(p, dtype=dtype), taps, weights)
    return ((np.abs(d[..., 0]) + np.abs(d[..., 1])) + np.abs(d[..., 2])).astype(dtype)


def sym_backward(p, taps, weights, g, dtype=F32, magnitude=False):
    """dL/dp [B, Vf, 3] for the cotangent g [B, Vf]: the row's own sign terms first, then the rows that tap it.  With
    ``magnitude`` the sum of the terms' absolute values instead."""
    p, g = np.asarray(p, dtype=dtype), np.asarray(g, dtype=dtype)
    Vf = taps.shape[0]
    if Vf == 0 or p.shape[0] == 0:
        return np.zeros(p.shape, dtype=dtype)
    acc = sign(_sym_terms(p, taps, weights)) * g[..., None]
    _, entries = transpose(taps, Vf)
    j, k = entries // 3, entries % 3
    s = sign(_sym_terms(p, taps, weights, j)) * g[:, j, None]
    u = np.stack([s[..., 0], -s[..., 1], -s[..., 2]], -1) * weights[j, k].astype(dtype)[None, :, None]
    if magnitude:
        acc, u = np.abs(acc), np.abs(u)
    return add_by_rank(acc, taps[j, k], u)


def sym_bound(p, taps, weights):
    p = np.asarray(p, dtype=np.float64)
    M = _sym_terms(p, taps, weights, magnitude=True).sum(-1)
    loss = sym_forward(p, taps, weights, np.float64)
    return U * (4 * M + 2 * loss + 4 * loss)


def sym_ambiguous(p, taps, weights, rel=1e-5):
    """[B, Vf] bool: rows whose gradient reads a sign decision within ``rel`` of zero (exact zeros excepted): their own, or
    that of a row that taps them."""
    p = np.asarray(p, dtype=np.float64)
    d = _sym_terms(p, taps, weights)
    scale = np.abs(p) + _sym_terms(p, taps, weights, magnitude=True)
    amb = ((np.abs(d) <= rel * scale) & (d != 0)).any(-1)
    bad = amb.copy()
    for k in range(3):
        live = taps[:, k] >= 0
        np.logical_or.at(bad, (slice(None), taps[live, k]), amb[:, live])
    return bad


# ---- pose ---------------------------------------------------------------------------------------------------------------
def _quaternion(pose, dt, trig):
    x, y, z = pose[..., 0], pose[..., 1], pose[..., 2]
    angle = np.sqrt((x * x + y * y) + z * z)
    half = dt(0.5) * angle
    small = angle < dt(SMALL)
    sh, ch = (np.asarray(fn(half), dtype=dt) for fn in trig)
    with np.errstate(invalid='ignore', divide='ignore'):
        s = np.where(small, dt(0.5) - (angle * angle) / dt(48.0), sh / angle)
    r, i, j, k = ch, s * x, s * y, s * z
    n = ((r * r + i * i) + j * j) + k * k
    return dict(x=x, y=y, z=z, angle=angle, small=small, sh=sh, ch=ch, s=s, r=r, i=i, j=j, k=k, n=n, two_s=dt(2.0) / n)


def _matrix(q, dt):
    r, i, j, k, t = q['r'], q['i'], q['j'], q['k'], q['two_s']
    one = dt(1.0)
    return np.stack([one - t * (j * j + k * k), t * (i * j - k * r), t * (i * k + j * r),
                     t * (i * j + k * r), one - t * (i * i + k * k), t * (j * k - i * r),
                     t * (i * k - j * r), t * (j * k + i * r), one - t * (i * i + j * j)], -1)


TRIG = (np.sin, np.cos)


def pose_forward(pose_out, pose_gt, dtype=F32, trig=TRIG):
    """[N, 3], [N, 3] -> [N, 9].  ``trig`` = (sin, cos) of the half angle: numpy's by default; the GPU tests pass the
    device's own, the one step of the route that is not bit-equal between a CPU and the device."""
    dt = np.dtype(dtype).type
    Ro = _matrix(_quaternion(np.asarray(pose_out, dtype=dt).reshape(-1, 3), dt, trig), dt)
    Rg = _matrix(_quaternion(np.asarray(pose_gt, dtype=dt).reshape(-1, 3), dt, trig), dt)
    return np.abs(Ro - Rg).astype(dt)


def pose_backward(pose_out, pose_gt, g, dtype=F32, trig=TRIG):
    """dL/dpose_out [N, 3] for the cotangent g [N, 9]: G = g * sign(R_out - R_gt), then the analytic Jacobian of the route
    (tests/kin_oracle.axis_angle_backward's lines), d angle / d x := 0 at angle == 0."""
    dt = np.dtype(dtype).type
    pose = np.asarray(pose_out, dtype=dt).reshape(-1, 3)
    q = _quaternion(pose, dt, trig)
    Ro = _matrix(q, dt)
    Rg = _matrix(_quaternion(np.asarray(pose_gt, dtype=dt).reshape(-1, 3), dt, trig), dt)
    G = np.asarray(g, dtype=dt).reshape(-1, 9) * sign(Ro - Rg)
    G = [G[..., n] for n in range(9)]
    x, y, z, r, i, j, k, t = (q[n] for n in ('x', 'y', 'z', 'r', 'i', 'j', 'k', 'two_s'))
    two = dt(2.0)
    m00, m01, m02 = j * j + k * k, i * j - k * r, i * k + j * r
    m10, m11, m12 = i * j + k * r, i * i + k * k, j * k - i * r
    m20, m21, m22 = i * k - j * r, j * k + i * r, i * i + j * j
    g_t = (((((((G[1] * m01 + G[2] * m02) + G[3] * m10) + G[5] * m12) + G[6] * m20) + G[7] * m21) - G[0] * m00)
           - G[4] * m11) - G[8] * m22
    h00, h01, h02 = -(t * G[0]), t * G[1], t * G[2]
    h10, h11, h12 = t * G[3], -(t * G[4]), t * G[5]
    h20, h21, h22 = t * G[6], t * G[7], -(t * G[8])
    g_r = ((((k * h10 - k * h01) + j * h02) - i * h12) - j * h20) + i * h21
    g_i = ((((((j * h01 + k * h02) + j * h10) + (two * i) * h11) - r * h12) + k * h20) + r * h21) + (two * i) * h22
    g_j = ((((((two * j) * h00 + i * h01) + r * h02) + i * h10) + k * h12) - r * h20) + k * h21 + (two * j) * h22
    g_k = ((((((two * k) * h00 - r * h01) + i * h02) + r * h10) + (two * k) * h11) + j * h12) + i * h20 + j * h21
    g_n = -(g_t * t) / q['n']
    g_r, g_i, g_j, g_k = g_r + (two * r) * g_n, g_i + (two * i) * g_n, g_j + (two * j) * g_n, g_k + (two * k) * g_n
    g_s = (g_i * x + g_j * y) + g_k * z
    g_half = -(q['sh'] * g_r)
    angle, s = q['angle'], q['s']
    with np.errstate(invalid='ignore', divide='ignore'):
        ga_small = dt(0.5) * g_half - g_s * (angle / dt(24.0))
        ga_big = dt(0.5) * (g_half + g_s * (q['ch'] / angle)) - g_s * (s / angle)
        g_angle = np.where(q['small'], ga_small, ga_big)
        zero = angle == 0
        u = [np.where(zero, dt(0.0), c / angle) for c in (x, y, z)]
    return np.stack([s * g_i + g_angle * u[0], s * g_j + g_angle * u[1], s * g_k + g_angle * u[2]], -1).astype(dt)


def pose_ambiguous(pose_out, pose_gt, rel=1e-5):
    """[N] bool: rotations with an entry of R_out - R_gt within ``rel`` of zero in float64 (exact zeros excepted)."""
    d = _matrix(_quaternion(np.asarray(pose_out, np.float64).reshape(-1, 3), np.float64, TRIG), np.float64) - \
        _matrix(_quaternion(np.asarray(pose_gt, np.float64).reshape(-1, 3), np.float64, TRIG), np.float64)
    return ((np.abs(d) <= rel) & (d != 0)).any(-1)


# ---- the centred vertex-to-vertex term -----------------------------------------------------------------------------------
def blocks(V):
    return (V + BLOCK - 1) // BLOCK


def v2v_depth(V):
    """The additions a value passes through in SUM2: 6 in its wave and 3 in its workgroup, then ceil(blocks / 256) in a
    thread of the second level and the same 6 + 3."""
    return 9 + blocks(blocks(V)) + 9


def sum2(x):
    """x [B, V, 3] -> [B, 3]: the header's SUM2 over the vertices, in x's dtype."""
    B, V = x.shape[:2]
    pad = np.zeros((B, blocks(V) * BLOCK, 3), dtype=x.dtype)
    pad[:, :V] = x
    partial = sum_oracle.wg_sum(np.moveaxis(pad.reshape(B, blocks(V), BLOCK, 3), 3, 1))       # [B, 3, blocks]
    out = np.zeros((B, 3), dtype=x.dtype)
    for b in range(B):
        for c in range(3):
            out[b, c] = sum_oracle.wg_sum(sum_oracle.strided_sum(partial[b, c]))
    return out


def v2v_means(out, target, dtype=F32):
    """[B, 6]: ma, then mt."""
    dt = np.dtype(dtype).type
    out, target = np.asarray(out, dtype=dt), np.asarray(target, dtype=dt)
    V = dt(out.shape[1])
    return np.concatenate([sum2(out) / V, sum2(target) / V], 1).astype(dt)


def _residual(out, target, m):
    return (out - m[:, None, :3]) - (target - m[:, None, 3:])


def v2v_forward(out, target, weight, scale=10.0, dtype=F32):
    dt = np.dtype(dtype).type
    out, target = np.asarray(out, dtype=dt), np.asarray(target, dtype=dt)
    w = np.asarray(weight, dtype=dt).reshape(1, -1, 1)
    if out.size == 0:
        return np.zeros(out.shape, dtype=dt)
    e = _residual(out, target, v2v_means(out, target, dt))
    return ((np.abs(e) * w) * dt(scale)).astype(dt)


def v2v_backward(out, target, weight, g, scale=10.0, dtype=F32):
    dt = np.dtype(dtype).type
    out, target, g = (np.asarray(x, dtype=dt) for x in (out, target, g))
    w = np.asarray(weight, dtype=dt).reshape(1, -1, 1)
    if out.size == 0:
        return np.zeros(out.shape, dtype=dt)
    e = _residual(out, target, v2v_means(out, target, dt))
    s = ((g * w) * dt(scale)) * sign(e)
    return (s - (sum2(s) / dt(out.shape[1]))[:, None, :]).astype(dt)


def v2v_bound(out, target, weight, scale=10.0):
    out, target = np.asarray(out, np.float64), np.asarray(target, np.float64)
    w = np.asarray(weight, np.float64).reshape(1, -1, 1)
    V = out.shape[1]
    k = V + v2v_depth(V) + 1
    ma, mt = np.abs(out).mean(1, keepdims=True), np.abs(target).mean(1, keepdims=True)
    e_bound = U * (k * (ma + mt) + 6 * (np.abs(out) + ma + np.abs(target) + mt))
    return w * scale * e_bound + 4 * U * v2v_forward(out, target, weight, scale, np.float64)


def v2v_ambiguous(out, target, rel=1e-5):
    """[B, V, 3] bool: elements whose e lies within ``rel`` (of |a| + |t|) of zero in float64, exact zeros excepted."""
    out, target = np.asarray(out, np.float64), np.asarray(target, np.float64)
    e = _residual(out, target, np.concatenate([out.mean(1), target.mean(1)], 1))
    return (np.abs(e) <= rel * (np.abs(out) + np.abs(target))) & (e != 0)


# ---- the cases ----------------------------------------------------------------------------------------------------------
def f32(a):
    return np.ascontiguousarray(a, dtype=F32)


def random_faces(rs, V, F):
    """[F, 3] int64: random triangles of three distinct vertices where V allows it."""
    if F == 0 or V == 0:
        return np.zeros((F, 3), dtype=np.int64)
    if V < 3:
        return rs.randint(0, V, (F, 3)).astype(np.int64)
    a = rs.randint(0, V, F)
    b = (a + 1 + rs.randint(0, V - 1, F)) % V
    c = rs.randint(0, V, F)
    clash = (c == a) | (c == b)
    while clash.any():
        c[clash] = rs.randint(0, V, int(clash.sum()))
        clash = (c == a) | (c == b)
    return np.stack([a, b, c], 1).astype(np.int64)


def edge_case(seed, B, V, F, valid_shape='1V1', gt_batch=None, face=None):
    """dict: out, gt [B or 1, V, 3] at the scale of a head in metres, valid (some zeros) in the requested shape, face, and a
    cotangent g [B, 3F, 1]."""
    rs = np.random.RandomState(seed)
    face = random_faces(rs, V, F) if face is None else np.asarray(face, dtype=np.int64)
    F = face.shape[0]
    gt = f32(0.1 * rs.randn(B if gt_batch is None else gt_batch, V, 3))
    out = f32(gt[:1] + 0.01 * rs.randn(B, V, 3)) if gt.shape[0] != B else f32(gt + 0.01 * rs.randn(B, V, 3))
    shape = {'1V1': (1, V, 1), 'BV1': (B, V, 1), 'V': (V,)}[valid_shape]
    valid = f32(rs.rand(*shape) > 0.2)
    return {'out': out, 'gt': gt, 'valid': valid, 'face': face, 'g': f32(rs.randn(B, 3 * F, 1))}


def valid_rows(c):
    """valid as the oracle takes it: [B or 1, V]."""
    v = c['valid']
    return v.reshape(v.shape[0] if v.ndim == 3 else 1, -1)


def sym_case(seed, B, V_full, Vf, hub=0, self_tap=True):
    """dict: the flip tables of a random correspondence, p [B, Vf, 3] and a cotangent g [B, Vf].  Row 0 taps only vertices
    without an offset (when there are any) and holds a zero offset: an exactly tied row.  ``hub``: that many rows tap row
    1 (a long CSR row); ``self_tap``: row 2 taps itself."""
    rs = np.random.RandomState(seed)
    fvi = np.sort(rs.permutation(V_full)[:Vf]).astype(np.int64)
    closest = rs.randint(0, V_full, (V_full, 3)).astype(np.int64)
    others = np.setdiff1d(np.arange(V_full), fvi)
    if others.size and Vf:
        closest[fvi[0]] = others[rs.randint(0, others.size, 3)]
    if Vf > 1 and hub:
        rows = 1 + rs.permutation(Vf - 1)[:hub]                  # (not row 0: its taps stay -1)
        closest[fvi[rows], rs.randint(0, 3, rows.size)] = fvi[1]
    if Vf > 2 and self_tap:
        closest[fvi[2], 1] = fvi[2]
    bc = rs.rand(V_full, 3)
    bc = f32(bc / bc.sum(1, keepdims=True))
    p = f32(0.005 * rs.randn(B, Vf, 3))
    if others.size and Vf:
        p[:, 0] = 0
    return {'vertex_num': V_full, 'face_vertex_idx': fvi, 'closest_faces': closest, 'bc': bc, 'p': p,
            'g': f32(rs.randn(B, Vf))}


def pose_case(seed, N, special=True):
    """dict: out, gt [N, 3] and a cotangent g [N, 9]; with ``special`` (and room): a zero row, an angle of 1e-7, angles near
    pi, and rows with out == gt."""
    rs = np.random.RandomState(seed)
    gt = f32(0.5 * rs.randn(N, 3))
    out = f32(gt + 0.1 * rs.randn(N, 3))
    if special and N >= 8:
        axis = rs.randn(4, 3)
        axis /= np.linalg.norm(axis, axis=1, keepdims=True)
        out[1] = 0
        out[2] = f32(1e-7 * axis[0])
        out[3], out[4] = f32(3.1415 * axis[1]), f32(3.1416 * axis[2])
        gt[5] = 0
        out[6] = gt[6]
        out[7], gt[7] = 0, 0
    return {'out': out, 'gt': gt, 'g': f32(rs.randn(N, 9))}


def v2v_case(seed, B, V, zero_weight=False):
    rs = np.random.RandomState(seed)
    t = f32(0.1 * rs.randn(B, V, 3) + 0.3 * rs.randn(B, 1, 3))
    a = f32(t + 0.002 * rs.randn(B, V, 3) + 0.05 * rs.randn(B, 1, 3))
    w = f32(np.zeros(V) if zero_weight else rs.rand(V) > 0.15)
    return {'out': a, 'target': t, 'weight': w.reshape(1, V, 1), 'g': f32(rs.randn(B, V, 3))}
