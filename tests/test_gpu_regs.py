"""The HIP arm and hand regularisers (exavatar_release_amd.vertex_regs) on the GPU.

Every output and gradient must equal the float32 oracle tests/reg_oracle.py BIT FOR BIT (a NaN must be a NaN; its bits are
the divider's business): the header fixes every rounding and the order of every sum, and the neighbour plan is decided
on integer keys.  Against the reference's own classes (tests/golden/ref_regs.npz) the results stay within twice the
float64 oracle's derived bound; the three rows of case d whose k-th key is an exact tie are compared with the oracle
alone.  Every call repeats bit for bit, and a captured graph replays the eager bits."""
import os

import numpy as np
import pytest
import torch

from exavatar_release_amd import vertex_normals
from exavatar_release_amd import vertex_regs as vr
from exavatar_release_amd.vertex_regs import (ArmPlan, ArmRGBReg, HandMeanReg, HandRGBReg, arm_neighbors, arm_rgb_loss,
                                              get_arm)
from tests import reg_oracle as ro

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_regs.npz')


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(GOLDEN))


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), '%s: %d of %d elements differ in their bits' % (what, int(bad.sum()), bad.size)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy()


# ---- arm ---------------------------------------------------------------------------------------------------------------
def _check_plan(plan, p):
    L = p['lower'].size
    header = _n(plan.header)
    assert header.tolist() == [p['upper'].size, L, p['k'], p['n_min']]
    assert int(plan.count) == L and int(plan.k) == p['k']
    assert np.array_equal(_n(plan.n_valid)[:L], p['n_valid'])
    assert np.array_equal(_n(plan.nbr)[:L], p['nbr'])
    rank = np.full(p['V'], -1, dtype=np.int32)
    rank[p['lower']] = np.arange(L)
    assert np.array_equal(_n(plan.lower_rank), rank)


def _check_arm(mesh, up, lo, rgb, G, top_k=50, thr=0.01, what=''):
    """Plan, dense loss, d and gradient against the oracle; every call twice.  -> the oracle's plan."""
    p = ro.arm_plan32(mesh, up, lo, thr, top_k)
    tm, tu, tl = _t(mesh), _t(up), _t(lo)
    plan = arm_neighbors(tm, tu, tl, thr, top_k)
    _check_plan(plan, p)
    plan2 = arm_neighbors(tm, tu, tl, thr, top_k)
    assert torch.equal(plan.nbr[:p['lower'].size], plan2.nbr[:p['lower'].size]) and torch.equal(plan.header, plan2.header)
    loss32, d32 = ro.arm_loss32(p, rgb)
    grad32 = ro.arm_grad32(p, d32, G)
    for _ in range(2):
        x = _t(rgb).requires_grad_(True)
        loss, d = arm_rgb_loss(plan, x, return_d=True)
        grad, = torch.autograd.grad(loss, x, _t(G))
        _same_bits(_n(loss), loss32, what + ' loss')
        _same_bits(_n(d), d32, what + ' d')
        _same_bits(_n(grad), grad32, what + ' dL/drgb')
    other = np.ones(mesh.shape[0], dtype=bool)
    other[p['lower']] = False
    assert not _n(grad).view(np.uint32)[:, other].any(), 'rows outside the lower arm get exactly +0'
    assert not _n(loss).view(np.uint32)[:, other].any()
    return p


@pytest.mark.parametrize('case', ['a', 'b', 'c', 'd'])
def test_arm_fixture_cases_equal_the_oracle_and_stay_within_the_bound_of_the_reference(golden, case):
    g = {k[2:]: v for k, v in golden.items() if k.startswith(case + '_')}
    mesh, up, lo, rgb, G = g['mesh'], g['is_upper'], g['is_lower'], g['rgb'], g['G']
    B, V = rgb.shape[0], rgb.shape[1]
    lower = np.nonzero(lo)[0]
    G_dense = np.zeros((B, V, 3), dtype=np.float32)
    G_dense[:, lower] = G
    p = _check_arm(mesh, up, lo, rgb, G_dense, what='case ' + case)
    assert p['k'] == int(g['k'])
    # the drop-in class: the reference's signature and [B, L, 3] result
    x = _t(rgb).requires_grad_(True)
    loss = ArmRGBReg()(_t(mesh), _t(up), _t(lo), x)
    grad, = torch.autograd.grad(loss, x, _t(G))
    loss32, d32 = ro.arm_loss32(p, rgb)
    _same_bits(_n(loss), loss32[:, lower], 'ArmRGBReg loss')
    _same_bits(_n(grad), ro.arm_grad32(p, d32, G_dense), 'ArmRGBReg dL/drgb')
    # the reference's own run: every untied row within twice the derived bound
    b64 = ro.arm_forward64(p, rgb, G)
    keep = np.ones(lower.size, dtype=bool)
    keep[g['tied_rows']] = False
    assert int((~keep).sum()) == (3 if case == 'd' else 0)
    err = np.abs(_n(loss).astype(np.float64) - g['loss32'])[:, keep]
    print('case %s: max |hip - ref| loss %.3e (bound %.3e)' % (case, err.max(), 2 * b64['E_loss'][:, keep].max()))
    assert (err <= 2 * b64['E_loss'][:, keep]).all()
    gerr = np.abs(_n(grad)[:, lower].astype(np.float64) - g['grad32'][:, lower])[:, keep]
    assert (gerr <= 2 * b64['E_grad'][:, keep]).all()
    assert not g['grad32'][:, ~lo].any()
    if case == 'c':      # the threshold decides as torch's float32 comparison does: u* is in the first two probes' sets only
        rows = g['probe_rows']
        has = (p['nbr'][rows, :p['k']] == int(g['ustar'])).any(1)
        assert has.tolist() == [True, True, False, False, False]


def _random_arm(V, U, L, seed, both=2, far_lower=False, duplicates=0):
    """Vertices with x in [0, 0.012) (most pairs valid at 0.01, not all); ``both`` vertices in both masks; with
    ``far_lower`` one lower vertex has no valid partner (k = 0); ``duplicates`` upper positions are repeated (ties
    that only the index breaks)."""
    rng = np.random.RandomState(seed)
    mesh = np.stack([rng.uniform(0, 0.012, V), rng.uniform(-0.05, 0.05, V), rng.uniform(-0.05, 0.05, V)], 1).astype(np.float32)
    perm = rng.permutation(V)
    both = min(both, U, L)
    up, lo = np.zeros(V, dtype=bool), np.zeros(V, dtype=bool)
    up[perm[:U]] = True
    lo[perm[U - both:U - both + L]] = True
    assert int(up.sum()) == U and int(lo.sum()) == L and int((up & lo).sum()) == both
    ups = np.nonzero(up & ~lo)[0]
    if duplicates:
        mesh[ups[duplicates:2 * duplicates]] = mesh[ups[:duplicates]]
    if far_lower:
        mesh[np.nonzero(lo & ~up)[0][0], 0] = 5.0
    return mesh, up, lo


ARM_CASES = {
    # name: (V, U, L, top_k, B, kwargs)
    'several-tiles': (6000, 5000, 300, 50, 1, dict(duplicates=40)),
    'U1': (40, 1, 13, 50, 2, {}),
    'U63': (120, 63, 13, 50, 1, {}),
    'U65': (120, 65, 13, 50, 3, {}),
    'topk1': (400, 200, 61, 1, 2, {}),
    'topk64': (400, 200, 61, 64, 2, dict(duplicates=10)),
    'k0': (300, 100, 21, 50, 2, dict(far_lower=True)),
    'no-upper': (50, 0, 9, 50, 1, dict(both=0)),
}


@pytest.mark.parametrize('name', sorted(ARM_CASES))
def test_arm_generated_cases_equal_the_oracle(name):
    V, U, L, top_k, B, kw = ARM_CASES[name]
    mesh, up, lo = _random_arm(V, U, L, seed=len(name) + V, **kw)
    rng = np.random.RandomState(V + B)
    rgb = rng.uniform(0, 1, (B, V, 3)).astype(np.float32)
    G = rng.standard_normal((B, V, 3)).astype(np.float32)
    p = _check_arm(mesh, up, lo, rgb, G, top_k=top_k, what=name)
    assert L % vr.ARM_WAVES != 0, 'the last workgroup of the selection is partly idle'
    if name == 'several-tiles':
        assert U > 4 * vr.ARM_TILE and p['k'] == 50
    if name in ('k0', 'no-upper'):
        assert p['k'] == 0
        loss32, _ = ro.arm_loss32(p, rgb)
        assert np.isnan(loss32[:, p['lower']]).all(), 'the reference\'s mean over an empty set'
    if name == 'topk64':
        assert p['k'] == 64
    if name == 'U1':
        assert p['k'] <= 1


def test_arm_class_reuses_one_plan_until_an_input_changes(golden):
    mesh, up, lo = _t(golden['a_mesh']), _t(golden['a_is_upper']), _t(golden['a_is_lower'])
    rgb = _t(golden['a_rgb'])
    reg = ArmRGBReg()
    before = ArmPlan.total_selection_launches
    first = reg(mesh, up, lo, rgb)
    plan = reg.plan
    second = reg(mesh, up, lo, rgb * 0.5)
    assert reg.plan is plan and plan.selection_launches == 1 and ArmPlan.total_selection_launches == before + 1
    assert torch.equal(first, reg(mesh, up, lo, rgb)) and not torch.equal(first, second)
    mesh.add_(0.0)                                             # an in-place change: a new version, a new plan
    reg(mesh, up, lo, rgb)
    assert reg.plan is not plan and ArmPlan.total_selection_launches == before + 2
    # a row capacity below V sizes the lists; the result is the same while it covers L
    L = int(golden['a_is_lower'].sum())
    small = arm_neighbors(mesh, up, lo, row_capacity=L + 3)
    assert small.nbr.shape[0] == L + 3
    assert torch.equal(arm_rgb_loss(small, rgb), arm_rgb_loss(reg.plan, rgb))
    # an empty lower arm: an empty result where the reference raises
    none = torch.zeros_like(lo)
    assert tuple(ArmRGBReg()(mesh, up, none, rgb).shape) == (rgb.shape[0], 0, 3)
    assert not arm_rgb_loss(arm_neighbors(mesh, up, none), rgb).any()
    # the trainer's mean without a synchronisation
    dense = arm_rgb_loss(reg.plan, rgb)
    mean = dense.sum() / (3 * rgb.shape[0] * reg.plan.count)
    assert abs(float(mean) - float(first.mean())) <= 1e-6 * float(first.mean())


# ---- hands -------------------------------------------------------------------------------------------------------------
def _check_hand_rgb(rgb, is_r, is_l, G, what):
    loss32, means32 = ro.hand_rgb32(rgb, is_r, is_l)
    grad32 = ro.hand_rgb_grad32(rgb, means32, G, is_r, is_l)
    reg = HandRGBReg()
    tr, tl = _t(is_r), _t(is_l)
    for _ in range(2):
        x = _t(rgb).requires_grad_(True)
        loss = reg(x, tr, tl)
        grad, = torch.autograd.grad(loss, x, _t(G))
        _same_bits(_n(loss), loss32, what + ' loss')
        _same_bits(_n(grad), grad32, what + ' dL/drgb')
    assert not _n(grad).view(np.uint32)[:, ~(is_r | is_l)].any(), 'rows outside the hands get exactly +0'
    return _n(loss), _n(grad)


def _check_hand_mean(verts, face, offset, normal, is_r, is_l, G, what):
    loss32 = ro.hand_mean32(offset, normal, is_r, is_l)
    grad32 = ro.hand_mean_grad32(offset, normal, G, is_r, is_l)
    reg = HandMeanReg(face)
    tr, tl, tv, tn = _t(is_r), _t(is_l), _t(verts), _t(normal)
    for _ in range(2):
        o = _t(offset).requires_grad_(True)
        loss = reg(tv, o, tr, tl, normal=tn)
        grad, = torch.autograd.grad(loss, o, _t(G))
        _same_bits(_n(loss), loss32, what + ' loss')
        _same_bits(_n(grad), grad32, what + ' dL/doffset')
    assert not _n(grad).view(np.uint32)[:, ~(is_r | is_l)].any(), 'rows outside the hands get exactly +0'
    return _n(loss), _n(grad)


def test_hand_fixture_equals_the_oracle_and_stays_within_the_bound_of_the_reference(golden):
    g = {k[2:]: v for k, v in golden.items() if k.startswith('h_')}
    is_r, is_l = g['is_rhand'], g['is_lhand']
    hand = np.nonzero(is_r | is_l)[0]
    loss, grad = _check_hand_rgb(g['rgb'], is_r, is_l, g['G_rgb'], 'HandRGBReg')
    b = ro.hand_rgb64(g['rgb'], is_r, is_l, g['G_rgb'])
    assert (np.abs(loss - g['rgb_loss32'].astype(np.float64)) <= 2 * b['E_loss']).all()
    assert (np.abs(grad - g['rgb_grad32'].astype(np.float64)) <= 2 * b['E_grad']).all()

    loss, grad = _check_hand_mean(g['verts'], g['face'], g['offset'], g['normal'], is_r, is_l, g['G_mean'], 'HandMeanReg')
    b = ro.hand_mean64(g['offset'], g['normal'], is_r, is_l, g['G_mean'])
    sure = ~b['unsure']
    assert sure.sum() >= sure.size - 2
    assert (np.abs(loss - g['mean_loss32'].astype(np.float64))[sure] <= 2 * b['E_loss'][sure]).all()
    assert (np.abs(grad[:, hand] - g['mean_grad32'][:, hand].astype(np.float64))[sure] <= 2 * b['E_grad'][sure]).all()
    assert np.isfinite(grad).all() and np.abs(grad[0, hand[3]]).max() > 1e10, 'the zero row: g * n / eps, finite'
    # without normal=: the class computes them itself, in a fixed order (the same bits on every call)
    reg = HandMeanReg(g['face'])
    o = _t(g['offset'])
    own = reg(_t(g['verts']), o, _t(is_r), _t(is_l))
    assert torch.equal(own, reg(_t(g['verts']), o, _t(is_r), _t(is_l)))
    assert (np.abs(_n(own) - loss)[sure] <= 1e-5).all()


@pytest.mark.parametrize('B', [1, 3])
def test_hands_generated_two_chunks_and_a_vertex_in_both_masks(B):
    V, N = 1000, 300                                           # 300 rows: a full chunk of 256 and a part of one
    rng = np.random.RandomState(40 + B)
    perm = rng.permutation(V)
    is_r, is_l = np.zeros(V, dtype=bool), np.zeros(V, dtype=bool)
    is_r[perm[:N]] = True
    is_l[perm[N - 5:2 * N - 5]] = True                         # five vertices in both masks
    assert N > vr.CHUNK and int((is_r & is_l).sum()) == 5
    rgb = rng.uniform(0, 1, (B, V, 3)).astype(np.float32)
    _check_hand_rgb(rgb, is_r, is_l, rng.standard_normal((B, N, 3)).astype(np.float32), 'HandRGBReg B=%d' % B)
    rows = 25
    verts = np.stack([np.tile(np.arange(V // rows), rows) * 0.01, np.repeat(np.arange(rows), V // rows) * 0.01,
                      rng.uniform(-4e-3, 4e-3, V)], 1).astype(np.float32)
    face = ro.grid_faces(rows, V // rows)
    normal = _n(vertex_normals(_t(verts), face))[0]
    offset = (rng.standard_normal((B, V, 3)) * 0.01).astype(np.float32)
    hand = np.nonzero(is_r | is_l)[0]
    offset[0, hand[::7]] = 0.0
    H = hand.size
    _check_hand_mean(verts, face, offset, normal, is_r, is_l, rng.standard_normal((B, H)).astype(np.float32),
                     'HandMeanReg B=%d' % B)


def test_get_arm_gives_the_same_masks_on_every_call_and_the_reference_expression():
    rows, cols = 30, 40
    V = rows * cols
    rng = np.random.RandomState(5)
    verts = np.stack([np.tile(np.arange(cols), rows) * 0.01, rng.uniform(-2e-2, 2e-2, V),
                      np.repeat(np.arange(rows), cols) * -0.01], 1).astype(np.float32)       # normals scatter around +y
    face = ro.grid_faces(rows, cols)
    weight = rng.uniform(0, 1, (V, 7)).astype(np.float32)
    tv, tw = _t(verts), _t(weight)
    normal = vertex_normals(tv, face)
    up1, lo1 = get_arm(tv, tw, face, [1, 2, 4, 5])
    up2, lo2 = get_arm(tv, tw, face, [1, 2, 4, 5])
    up3, lo3 = get_arm(tv, tw, face, [1, 2, 4, 5], normal=normal)
    assert up1.dtype == torch.bool and tuple(up1.shape) == (V,)
    assert torch.equal(up1, up2) and torch.equal(lo1, lo2) and torch.equal(up1, up3) and torch.equal(lo1, lo3)
    is_arm = np.isin(weight.argmax(1), [1, 2, 4, 5])
    ny = _n(normal)[0, :, 1].astype(np.float64)
    assert np.array_equal(_n(up1), is_arm & (ny > np.cos(np.pi / 3))) and np.array_equal(_n(lo1), is_arm & (ny <= np.cos(np.pi / 3)))
    assert 0 < int(up1.sum()) < int(is_arm.sum())


def test_one_captured_graph_replays_the_eager_bits(golden):
    mesh, up, lo = _t(golden['b_mesh']), _t(golden['b_is_upper']), _t(golden['b_is_lower'])
    V = mesh.shape[0]
    rng = np.random.RandomState(9)
    perm = rng.permutation(V)
    is_r, is_l = torch.zeros(V, dtype=torch.bool, device=DEV), torch.zeros(V, dtype=torch.bool, device=DEV)
    is_r[_t(perm[:300])] = True
    is_l[_t(perm[300:600])] = True
    rgb = _t(golden['b_rgb']).requires_grad_(True)
    offset = _t((rng.standard_normal((2, V, 3)) * 0.01).astype(np.float32)).requires_grad_(True)
    normal = torch.nn.functional.normalize(_t(rng.standard_normal((V, 3)).astype(np.float32)), dim=1)
    hand_rgb, hand_mean = HandRGBReg(), HandMeanReg(None)

    def step():
        plan = arm_neighbors(mesh, up, lo)
        a = arm_rgb_loss(plan, rgb)
        h = hand_rgb(rgb, is_r, is_l)
        m = hand_mean(mesh, offset, is_r, is_l, normal=normal)
        g_rgb, g_off = torch.autograd.grad([a.sum(), h.sum(), m.sum()], [rgb, offset])
        return a, h, m, g_rgb, g_off

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()                                             # builds the hand tables: the one synchronisation
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    with torch.no_grad():
        rgb.copy_(_t(golden['b_rgb'][::-1].copy()))
        offset.mul_(-1.5)
        mesh.copy_(_t(golden['b_mesh'] * np.float32(1.25)))
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    for name, got, want in zip(('arm', 'hand rgb', 'hand mean', 'dL/drgb', 'dL/doffset'), outs, eager):
        _same_bits(_n(got), _n(want), 'replayed ' + name)
    p = ro.arm_plan32(_n(mesh), golden['b_is_upper'], golden['b_is_lower'])
    _same_bits(_n(outs[0]), ro.arm_loss32(p, _n(rgb))[0], 'replayed arm loss against the oracle')
