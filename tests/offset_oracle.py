"""The Gaussian offset and joint offset regularisers (include/exa_mesh.h, ``exa_mesh_offset_regs_*``) restated operation by
operation and sum by sum in numpy: in float32, where every array must equal the kernels' bit for bit, and in float64,
where the means are the exact values the float32 means are held against.

Arrays: ``mo``, ``moo``, ``sc`` [B, V, 3]; ``so`` [B, V, 1] or [B, V, 3]; ``wm``, ``ws`` [V]; ``jo``, ``ref``, ``wj`` [J, 3];
``pr``, ``pl`` [P] (the right and the left joints of the pairs).  Also the header's work split as plain functions
(``blocks``, ``mean_depth``) and the small random cases of the tests."""
import numpy as np

from tests import sum_oracle

BLOCK = 256              # EXA_MESH_OFFSET_ROWS: rows per workgroup = threads of a workgroup
TERMS = ('gaussian_mean_reg', 'gaussian_scale_reg', 'joint_offset_reg', 'joint_offset_sym_reg')
F32 = np.float32


def _a(x, dtype):
    return np.asarray(x, dtype=dtype)


# ---- the maps -----------------------------------------------------------------------------------------------------------
def maps(mo, moo, sc, so, wm, ws, jo, ref, wj, pr, pl, dtype=F32):
    """The four maps in ``TERMS`` order: ((a a) + (b b)) w per vertex element, ((jo - ref) (jo - ref)) wj per joint element
    and (|xr + xl| + |yr - yl|) + |zr - zl| per pair, every operation rounded to ``dtype``."""
    mo, moo, sc, so, jo, ref, wj = (_a(x, dtype) for x in (mo, moo, sc, so, jo, ref, wj))
    wm, ws = _a(wm, dtype).reshape(1, -1, 1), _a(ws, dtype).reshape(1, -1, 1)
    pr, pl = np.asarray(pr, dtype=np.int64).reshape(-1), np.asarray(pl, dtype=np.int64).reshape(-1)
    mean_map = ((mo * mo) + (moo * moo)) * wm
    scale_map = ((sc * sc) + (so * so)) * ws
    d = jo - ref
    joint_map = (d * d) * wj
    R, L = jo[pr], jo[pl]
    sym_map = (np.abs(R[:, 0] + L[:, 0]) + np.abs(R[:, 1] - L[:, 1])) + np.abs(R[:, 2] - L[:, 2])
    return mean_map, scale_map, joint_map, sym_map


# ---- the sums -----------------------------------------------------------------------------------------------------------
def vertex_partials(vmap):
    """[blocks] float32 of a [B, V, 3] map: per row (t0 + t1) + t2, +0 past the last row, WG per 256 consecutive rows."""
    rows = np.asarray(vmap, dtype=F32).reshape(-1, 3)
    r = (rows[:, 0] + rows[:, 1]) + rows[:, 2]
    n = blocks_of_rows(rows.shape[0])
    pad = np.zeros(n * BLOCK, F32)
    pad[:r.size] = r
    return sum_oracle.wg_sum(pad.reshape(n, BLOCK)) if n else np.zeros(0, F32)


def means32(all_maps):
    """[4] float32: the header's means of the four float32 maps (an empty map: NaN); each sum the strided sum, then WG."""
    flat = [vertex_partials(all_maps[0]), vertex_partials(all_maps[1]), all_maps[2], all_maps[3]]
    sums = [sum_oracle.wg_sum(sum_oracle.strided_sum(np.asarray(x, dtype=F32))) for x in flat]
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.array([F32(s) / F32(m.size) for s, m in zip(sums, all_maps)], dtype=F32)


def means64(*inputs):
    return np.array([float(m.mean()) if m.size else float('nan') for m in maps(*inputs, dtype=np.float64)])


# ---- the gradients ------------------------------------------------------------------------------------------------------
def sign(x):
    return (x > 0).astype(F32) - (x < 0).astype(F32)


def cotangents(all_maps, g_maps=None, g_means=None, reciprocal=True):
    """The four float32 cotangent arrays (None: the term has none).  ``g_maps``: four arrays or Nones.  ``g_means``: four
    scalars or Nones; ``reciprocal`` = True is the header's g = g_k * (1 / float32(N_k)), what torch's backward of
    ``.mean()`` forms on the device; False is g_k / float32(N_k), what it forms on the CPU."""
    assert (g_maps is None) != (g_means is None)
    if g_maps is not None:
        return [None if g is None else np.asarray(g, dtype=F32).reshape(m.shape) for g, m in zip(g_maps, all_maps)]
    out = []
    for g, m in zip(g_means, all_maps):
        if g is None:
            out.append(None)
            continue
        with np.errstate(divide='ignore', invalid='ignore'):
            k = F32(g) * (F32(1) / F32(m.size)) if reciprocal else F32(g) / F32(m.size)
        out.append(np.full(m.shape, k, dtype=F32))
    return out


def grads(mo, moo, sc, so, wm, ws, jo, ref, wj, pr, pl, g_maps=None, g_means=None, reciprocal=True):
    """dict name -> float32 gradient (None: no cotangent reaches it) of mo, moo, sc, so, jo in the header's order:
    (g w) (2 x); a one-channel ``so``: r = ((g0 w + g1 w) + g2 w), r (2 so); jo: d_reg + d_sym, one alone where the other
    term has no cotangent or the joint no pair."""
    mo, moo, sc, so, jo, ref, wj = (_a(x, F32) for x in (mo, moo, sc, so, jo, ref, wj))
    wm, ws = _a(wm, F32).reshape(1, -1, 1), _a(ws, F32).reshape(1, -1, 1)
    pr, pl = np.asarray(pr, dtype=np.int64).reshape(-1), np.asarray(pl, dtype=np.int64).reshape(-1)
    g = cotangents(maps(mo, moo, sc, so, wm, ws, jo, ref, wj, pr, pl), g_maps, g_means, reciprocal)
    two = F32(2)
    out = dict.fromkeys(('mo', 'moo', 'sc', 'so', 'jo'))
    if g[0] is not None:
        gw = g[0] * wm
        out['mo'], out['moo'] = gw * (two * mo), gw * (two * moo)
    if g[1] is not None:
        gw = g[1] * ws
        out['sc'] = gw * (two * sc)
        if so.shape[2] == 1:
            r = (gw[:, :, 0] + gw[:, :, 1]) + gw[:, :, 2]
            out['so'] = r[:, :, None] * (two * so)
        else:
            out['so'] = gw * (two * so)
    if g[2] is not None or g[3] is not None:
        J = jo.shape[0]
        d = np.zeros((J, 3), F32)
        if g[2] is not None:
            d = (g[2] * wj) * (two * (jo - ref))
        if g[3] is not None and pr.size:
            R, L = jo[pr], jo[pl]
            s = np.stack([sign(R[:, 0] + L[:, 0]), sign(R[:, 1] - L[:, 1]), sign(R[:, 2] - L[:, 2])], 1) * g[3][:, None]
            left = s * np.array([1, -1, -1], F32)
            if g[2] is not None:
                d[pr], d[pl] = d[pr] + s, d[pl] + left
            else:
                d[pr], d[pl] = s, left
        out['jo'] = d.astype(F32)
    return out


# ---- the header's work split ----------------------------------------------------------------------------------------------
def blocks_of_rows(rows):
    return (rows + BLOCK - 1) // BLOCK if rows > 0 else 0


def blocks(B, V):
    """exa_mesh_offset_regs_blocks: the workgroups (partials per term) of the vertex launch."""
    return blocks_of_rows(B * V) if B > 0 and V > 0 else 0


def mean_depth(B, V, J, P):
    """[4]: the additions an element passes through on its way into each mean, by the header's rule.  A vertex element: 2
    in its row, 6 in its wave and 3 in its workgroup, then ceil(partials / 256) in a thread of the reduction and the same
    6 + 3.  A joint element or a pair: ceil(N / 256) in its thread and 6 + 3."""
    trips = lambda n: (n + BLOCK - 1) // BLOCK      # noqa: E731
    v = 2 + 9 + trips(blocks(B, V)) + 9
    return [v, v, trips(3 * J) + 9, trips(P) + 9]


# ---- small random cases -----------------------------------------------------------------------------------------------
def make_case(seed, B, V, J, P, so_channels=1):
    """dict of float32 arrays (and int64 ``pr``, ``pl``) at the magnitudes of the loss block: offsets ~ 1e-2, scales ~ 1e-3,
    weights from the reference's values (0 among them), P disjoint right / left pairs among the J joints."""
    rs = np.random.RandomState(seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=F32)      # noqa: E731
    perm = rs.permutation(J)
    c = {'mo': f32(0.01 * rs.randn(B, V, 3)), 'moo': f32(0.01 * rs.randn(B, V, 3)),
         'sc': f32(rs.uniform(0.0005, 0.0015, (B, V, 3))), 'so': f32(0.1 * rs.randn(B, V, so_channels)),
         'wm': f32(rs.choice([1.0, 10.0, 1000.0], V)), 'ws': f32(rs.choice([0.0, 1.0, 10.0, 1000.0], V)),
         'ref': f32(0.01 * rs.randn(J, 3)), 'wj': f32(rs.choice([1.0, 10.0], (J, 3))),
         'pr': np.sort(perm[:P]).astype(np.int64), 'pl': perm[P:2 * P].astype(np.int64)}
    c['jo'] = f32(c['ref'] + 0.005 * rs.randn(J, 3))
    return c


ORDER = ('mo', 'moo', 'sc', 'so', 'wm', 'ws', 'jo', 'ref', 'wj', 'pr', 'pl')


def args(case):
    return tuple(case[k] for k in ORDER)


def block_case():
    """The offset terms' inputs of the loss block's case (tests/loss_case.py) in this module's names: the weights as the
    block builds them, the pre-clamp scale repeated to three channels (what both the warm-up's ``scale_wo_clamp`` and the
    other branch's ``scale`` hold) and the 24 right / left pairs of the SMPL-X names."""
    import torch
    from tests import loss_case as lc
    case = lc.build_case()
    masks = {k: torch.from_numpy(np.array(case[k])) for k in lc.MASKS}
    wt = lc.vertex_weights(masks, torch.ones((1, lc.V, 1)))
    names = list(lc.JOINTS_NAME)
    right = [j for j in range(lc.J) if names[j][:2] == 'R_']
    left = [names.index('L_' + names[j][2:]) for j in right]
    return {'mo': case['mean_offset'], 'moo': case['mean_offset_offset'], 'sc': np.repeat(case['scale_raw'], 3, axis=2),
            'so': case['scale_offset'], 'wm': wt['gaussian_mean_reg'].numpy().reshape(-1),
            'ws': wt['gaussian_scale_reg'].numpy().reshape(-1), 'jo': case['joint_offset'], 'ref': case['joint_offset_ref'],
            'wj': lc.joint_weight(torch.ones((lc.J, 3))).numpy(), 'pr': np.array(right), 'pl': np.array(left)}
