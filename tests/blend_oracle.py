"""CPU oracles of the blend-shape offsets (include/exa_mesh.h ``exa_mesh_blend_*``, exavatar_release_amd/blend_shapes.py).

(a) ``plan``: the compaction restated in numpy -- the kept columns of a full ``[K, M]`` matrix in ascending order as a
    feature-major ``[K, N_pad]`` table (N_pad = N rounded up to 4, pad columns zero), ``cols`` (compact column -> flat
    output index) and ``inv`` (its inverse, -1 where an output is not covered).

(b) ``forward32`` / ``backward32``: the header's arithmetic in numpy float32, one array operation per rounded operation.
    numpy evaluates ``a * b`` and ``c + p`` as two separately rounded array operations, so no product is fused into an
    add and no sum is re-associated: the results are what the kernels must give bit for bit.
      forward   rows cut into 8 segments of L = ceil(K / 8) rows; p_s = +0.0, then p_s = p_s + coef[k] * table[k, col] for
                the rows of segment s in ascending order; sum = p_0, then sum = sum + p_s for s = 1 .. 7; covered outputs
                get sum (masked: +0.0), uncovered ones base (+0.0 without one).
      backward  dL/dbase = g_out + g_masked where uncovered, +0.0 where covered.  dL/dcoef[k]: chunks of 1024 compact
                columns (g = 0 and table = 0 beyond N); lane t of 256 forms ((T0 g0 + T1 g1) + T2 g2) + T3 g3 over its
                columns 4 t .. 4 t + 3; each wave of 64 lanes is added as the tree q_i = q_i + q_(i + off), i < off, for
                off = 32 .. 1; the chunk's partial is ((w0 + w1) + w2) + w3; dL/dcoef[k] = +0.0 plus the partials in
                ascending chunk order.

(c) ``forward64`` / ``backward64``: the same functions of the same float32 inputs in float64, with a bound per element on
    the error of ANY float32 evaluation, whatever its order.  The bound is derived, not measured.  The inputs are exactly
    representable in fp32, so no input rounding enters.  An n-term dot product sum_i a_i b_i evaluated in fp32 -- n
    products, each rounded once, and n - 1 additions in any order, so every term passes through at most n roundings --
    has error at most gamma_n * sum_i |a_i b_i| with gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability
    of Numerical Algorithms, 2nd ed., eq. 3.5; it holds for every order of summation).  Starting a sum from +0.0 adds an
    exact operation and no rounding.
      out[j]      n = K:  E = gamma_K * sum_k |coef_k dirs_kj|;  uncovered outputs are copies: E = 0.
      dL/dcoef[k] n = N:  E = gamma_N * sum_s |dirs_k,s g_s|  (the kernel's zero pad terms are exact).
      dL/dbase    one addition of two fp32 values: E = u |g_out + g_masked|.
    PyTorch's own evaluation of the reference expressions obeys the same bounds, so two fp32 evaluations differ by at most
    twice the bound.
"""
import numpy as np

from tests import sum_oracle

U = 2.0 ** -24
SEGMENTS = 8         # EXA_MESH_BLEND_SEGMENTS
CHUNK = 1024         # EXA_MESH_BLEND_CHUNK


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- (a) the plan ---------------------------------------------------------------------------------------------------
def plan(dirs, keep):
    """dirs [K, M] float32, keep [M] bool -> (table [K, N_pad] float32, cols [N] int32, inv [M] int32)."""
    dirs = np.asarray(dirs, dtype=np.float32)
    keep = np.asarray(keep, dtype=bool)
    K, M = dirs.shape
    cols = np.flatnonzero(keep)
    N = cols.size
    table = np.zeros((K, (N + 3) // 4 * 4), dtype=np.float32)
    table[:, :N] = dirs[:, cols]
    inv = np.full(M, -1, dtype=np.int32)
    inv[cols] = np.arange(N, dtype=np.int32)
    return table, cols.astype(np.int32), inv


def pose_keep(pose_mask):
    """The three channels of every masked vertex."""
    return np.repeat(np.asarray(pose_mask, dtype=bool), 3)


def expr_full(expr_dirs):
    """expr_dirs [V, 3, Ke] -> (dirs [Ke, 3 V], keep [3 V]): the three channels of every vertex whose row has a non-zero."""
    e = np.asarray(expr_dirs, dtype=np.float32)
    V = e.shape[0]
    return np.ascontiguousarray(e.reshape(3 * V, -1).T), np.repeat((e != 0).reshape(V, -1).any(1), 3)


# ---- (b) float32, op by op ------------------------------------------------------------------------------------------
def forward32(coef, table, cols, inv, base=None):
    """-> (out [M], masked [M] or None), float32."""
    coef = np.asarray(coef, dtype=np.float32).reshape(-1)
    table = np.asarray(table, dtype=np.float32)
    K, N, M = table.shape[0], cols.size, inv.size
    L = (K + SEGMENTS - 1) // SEGMENTS
    total = None
    for s in range(SEGMENTS):
        p = np.zeros(N, dtype=np.float32)
        for k in range(s * L, min(K, (s + 1) * L)):
            prod = coef[k] * table[k, :N]
            p = p + prod
        total = p if s == 0 else total + p
    fill = np.zeros(M, dtype=np.float32) if base is None else np.asarray(base, dtype=np.float32).reshape(-1)
    out = fill.copy()
    out[cols] = total
    if base is None:
        return out, None
    masked = fill.copy()
    masked[cols] = np.float32(0.0)
    return out, masked


def backward32(table, cols, inv, g_out, g_masked=None):
    """-> (dL/dcoef [K], dL/dbase [M]), float32, summed in the header's order."""
    table = np.asarray(table, dtype=np.float32)
    g_out = np.asarray(g_out, dtype=np.float32).reshape(-1)
    K, N, M = table.shape[0], cols.size, inv.size
    chunks = (N + CHUNK - 1) // CHUNK
    g = np.zeros(chunks * CHUNK, dtype=np.float32)
    g[:N] = g_out[cols]
    g = g.reshape(chunks, 256, 4)
    dcoef = np.zeros(K, dtype=np.float32)
    for k0 in range(0, K, 32):                             # row blocks: only to bound the memory of the products
        T = np.zeros((min(K, k0 + 32) - k0, chunks * CHUNK), dtype=np.float32)
        T[:, :table.shape[1]] = table[k0:k0 + 32]
        T = T.reshape(T.shape[0], chunks, 256, 4)
        q = T[..., 0] * g[None, :, :, 0]
        for i in (1, 2, 3):
            prod = T[..., i] * g[None, :, :, i]
            q = q + prod
        partial = sum_oracle.waves(sum_oracle.tree(q.reshape(q.shape[0], chunks, 4, 64)))      # [rows, chunks]
        acc = np.zeros(partial.shape[0], dtype=np.float32)
        for c in range(chunks):
            acc = acc + partial[:, c]
        dcoef[k0:k0 + 32] = acc
    dbase = g_out.copy() if g_masked is None else g_out + np.asarray(g_masked, dtype=np.float32).reshape(-1)
    dbase[inv >= 0] = np.float32(0.0)
    return dcoef, dbase.astype(np.float32)


# ---- (c) float64 with derived bounds --------------------------------------------------------------------------------
def _rows(table, n, block=64):
    """The table's first n columns in float64, a block of rows at a time (the full-size pose table is 390 MB in fp32)."""
    for k0 in range(0, table.shape[0], block):
        yield k0, np.asarray(table[k0:k0 + block, :n], dtype=np.float64)


def forward64(coef, table, cols, inv, base=None):
    """-> dict(out, E_out, masked), float64 [M] (masked None without a base)."""
    coef = np.asarray(coef, dtype=np.float64).reshape(-1)
    K, N, M = table.shape[0], cols.size, inv.size
    fill = np.zeros(M) if base is None else np.asarray(base, dtype=np.float64).reshape(-1)
    out, E = fill.copy(), np.zeros(M)
    val, mag = np.zeros(N), np.zeros(N)
    for k0, T in _rows(table, N):
        val += coef[k0:k0 + T.shape[0]] @ T
        mag += np.abs(coef[k0:k0 + T.shape[0]]) @ np.abs(T)
    out[cols] = val
    E[cols] = gamma(K) * mag
    masked = None
    if base is not None:
        masked = fill.copy()
        masked[cols] = 0.0
    return dict(out=out, E_out=E, masked=masked)


def backward64(table, cols, inv, g_out, g_masked=None):
    """-> dict(dcoef, E_dcoef [K], dbase, E_dbase [M]), float64."""
    g_out = np.asarray(g_out, dtype=np.float64).reshape(-1)
    K, N = table.shape[0], cols.size
    g = g_out[cols]
    dcoef, mag = np.zeros(K), np.zeros(K)
    for k0, T in _rows(table, N):
        dcoef[k0:k0 + T.shape[0]] = T @ g
        mag[k0:k0 + T.shape[0]] = np.abs(T) @ np.abs(g)
    dbase = g_out.copy() if g_masked is None else g_out + np.asarray(g_masked, dtype=np.float64).reshape(-1)
    dbase[inv >= 0] = 0.0
    return dict(dcoef=dcoef, E_dcoef=gamma(max(N, 1)) * mag, dbase=dbase,
                E_dbase=(0.0 if g_masked is None else U) * np.abs(dbase))


# ---- test data ------------------------------------------------------------------------------------------------------
COVERAGES = ('none', 'one', 'random', 'all')


def coverage_mask(V, coverage, rng, share=0.4):
    """[V] bool: no vertex, one vertex, a random share of them (at least one), or all."""
    mask = np.zeros(V, dtype=bool)
    if coverage == 'one':
        mask[rng.randint(V)] = True
    elif coverage == 'random':
        mask[rng.choice(V, size=max(int(round(share * V)), 1), replace=False)] = True
    elif coverage == 'all':
        mask[:] = True
    elif coverage != 'none':
        raise ValueError(coverage)
    return mask


def random_case(K, V, coverage, seed, share=0.4):
    """Inputs generated in fp32: dirs [K, 3 V], vertex mask [V], coef [K], base, g_out, g_masked [3 V]."""
    rng = np.random.RandomState(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
    return dict(dirs=f(K, 3 * V), mask=coverage_mask(V, coverage, rng, share), coef=f(K), base=f(3 * V),
                g_out=f(3 * V), g_masked=f(3 * V))
