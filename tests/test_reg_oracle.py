"""The CPU oracles of the arm and hand regularisers (tests/reg_oracle.py) against the reference's own classes.

tests/golden/ref_regs.npz holds what the reference's ``ArmRGBReg``, ``HandRGBReg`` and ``HandMeanReg`` returned, run
unchanged in float32 and, on the same numbers, in float64 (tests/golden/make_golden_regs.py).  The float32 oracle -- what
the kernels must give bit for bit -- has to lie within the derived bound of the reference's float64 run, and so has the
reference's own float32 run: the bound is checked against the reference's recorded error, not chosen."""
import os

import numpy as np
import pytest

from tests import reg_oracle as ro

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_regs.npz')


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(GOLDEN))


def _case(golden, case):
    return {k[2:]: v for k, v in golden.items() if k.startswith(case + '_')}


@pytest.mark.parametrize('case', ['a', 'b', 'c', 'd'])
def test_arm_oracle_reproduces_the_reference_within_the_derived_bound(golden, case):
    g = _case(golden, case)
    lo = g['is_lower']
    lower = np.nonzero(lo)[0]
    p = ro.arm_plan32(g['mesh'], g['is_upper'], lo)
    assert p['k'] == int(g['k']) == {'a': 21, 'b': 50, 'c': 21, 'd': 50}[case]
    assert np.array_equal(p['n_valid'], g['n_valid'])
    loss32, d32 = ro.arm_loss32(p, g['rgb'])
    G_dense = np.zeros_like(g['rgb'])
    G_dense[:, lower] = g['G']
    grad32 = ro.arm_grad32(p, d32, G_dense)
    b = ro.arm_forward64(p, g['rgb'], g['G'])
    tied = g['tied_rows']
    assert tied.size == (3 if case == 'd' else 0)
    untied = np.ones(lower.size, dtype=bool)
    untied[tied] = False
    in64 = untied.copy()
    in64[g['f64_skip']] = False                      # case c: the float64 run compares |dx| == 0.01f with the double 0.01
    assert g['f64_skip'].size == (1 if case == 'c' else 0)
    # the reference's float64 run on the same neighbour sets is the oracle's float64 value ...
    assert np.allclose(b['loss'][:, in64], g['loss64'][:, in64], rtol=1e-12, atol=0)
    assert np.allclose(b['grad'][:, in64], g['grad64'][:, lower][:, in64], rtol=1e-12, atol=0)
    # ... the reference's own float32 error stays within the bound, and so does the oracle's
    ref_err = np.abs(g['loss32'] - g['loss64'])[:, in64]
    ora_err = np.abs(loss32[:, lower] - b['loss'])[:, untied]
    assert (ref_err <= b['E_loss'][:, in64]).all() and (ora_err <= b['E_loss'][:, untied]).all()
    assert ref_err.max() > 0.02 * b['E_loss'][:, in64].max(), 'the bound is within two orders of the recorded error'
    assert (np.abs(g['loss32'] - loss32[:, lower])[:, untied] <= 2 * b['E_loss'][:, untied]).all()
    assert (np.abs(g['grad32'][:, lower] - b['grad'])[:, in64] <= b['E_grad'][:, in64]).all()
    assert (np.abs(grad32[:, lower] - b['grad'])[:, untied] <= b['E_grad'][:, untied]).all()
    assert not grad32[:, ~lo].any() and not g['grad32'][:, ~lo].any()
    # a wrong neighbour set is no rounding matter: swapping the k-th neighbour for the (k+1)-th moves the target by
    # about |rgb| / k against a bound of (k + 1) u |rgb|: a ratio of 1 / (k (k + 1) u), 6 500 at k = 50
    k = p['k']
    wide = ro.arm_plan32(g['mesh'], g['is_upper'], lo, top_k=k + 1)
    rows = np.nonzero((wide['nbr'][:, k] >= 0) & untied)[0]
    wrong = dict(p, nbr=p['nbr'].copy())
    wrong['nbr'][rows, k - 1] = wide['nbr'][rows, k]
    moved = np.abs(ro.arm_loss32(wrong, g['rgb'])[1] - d32)[:, lower[rows]]
    assert np.median(moved) > 1e-3 and np.median(moved) > 1e3 * np.median(b['E_d'])
    if case == 'd':      # the tied rows: the oracle takes the lower index; the reference's choice is topk's own
        for row in tied:
            a, c = p['nbr'][row, k - 1], wide['nbr'][row, k]
            assert a < c and (g['mesh'][a] == g['mesh'][c]).all()


def test_arm_threshold_decides_as_the_float32_comparison_of_the_reference(golden):
    g = _case(golden, 'c')
    p = ro.arm_plan32(g['mesh'], g['is_upper'], g['is_lower'])
    rows, ustar = g['probe_rows'], int(g['ustar'])
    lower = np.nonzero(g['is_lower'])[0]
    dx = np.abs(g['mesh'][lower[rows], 0] - g['mesh'][ustar, 0])
    thr = np.float32(0.01)
    assert dx.tolist() == [np.nextafter(thr, np.float32(0))] * 2 + [np.nextafter(thr, np.float32(1))] * 2 + [thr]
    has = (p['nbr'][rows, :p['k']] == ustar).any(1)
    assert has.tolist() == [True, True, False, False, False]
    # and the reference agrees on all five rows (they are among the rows compared above): taking u* into the exact
    # row's set, as a double comparison would, moves its loss far outside the bound
    b = ro.arm_forward64(p, g['rgb'])
    loss32 = ro.arm_loss32(p, g['rgb'])[0][:, lower]
    assert (np.abs(loss32 - g['loss32'])[:, rows] <= 2 * b['E_loss'][:, rows]).all()
    assert (np.abs(g['loss64'] - g['loss32'])[:, rows[-1]] > 100 * b['E_loss'][:, rows[-1]]).any()


def test_arm_k_zero_is_nan_on_both_sides():
    import torch
    mesh, up, lo = ro.two_tube_arms(4, 12, seed=3)
    far = np.nonzero(lo)[0][0]
    mesh[far, 0] = 5.0                                   # one lower vertex without a valid partner: n_min = 0
    p = ro.arm_plan32(mesh, up, lo)
    assert p['k'] == 0 and p['n_min'] == 0
    rgb = np.random.RandomState(1).uniform(0, 1, (1, mesh.shape[0], 3)).astype(np.float32)
    loss, d = ro.arm_loss32(p, rgb)
    assert np.isnan(loss[:, lo]).all() and not loss[:, ~lo].any()
    assert np.isnan(ro.arm_grad32(p, d, np.ones_like(rgb))[:, lo]).all()
    # the reference's expression at top_k = 0: the mean over an empty set
    t = torch.from_numpy(rgb)
    idx = torch.zeros((int(lo.sum()), 0), dtype=torch.int64)
    ref = (t[:, torch.from_numpy(lo), :] - t[:, idx.view(-1), :].view(1, int(lo.sum()), 0, 3).mean(2)) ** 2
    assert torch.isnan(ref).all()


def test_hand_oracles_reproduce_the_reference_within_the_derived_bounds(golden):
    g = _case(golden, 'h')
    is_r, is_l = g['is_rhand'], g['is_lhand']
    assert int(is_r.sum()) == int(is_l.sum()) == 17 and not (is_r & is_l).any()
    hand = np.nonzero(is_r | is_l)[0]
    loss32, means32 = ro.hand_rgb32(g['rgb'], is_r, is_l)
    grad32 = ro.hand_rgb_grad32(g['rgb'], means32, g['G_rgb'], is_r, is_l)
    b = ro.hand_rgb64(g['rgb'], is_r, is_l, g['G_rgb'])
    assert np.allclose(b['loss'], g['rgb_loss64'], rtol=1e-12, atol=1e-18)
    assert np.allclose(b['grad'], g['rgb_grad64'], rtol=1e-12, atol=1e-18)
    for got_loss, got_grad in ((g['rgb_loss32'], g['rgb_grad32']), (loss32, grad32)):
        assert (np.abs(got_loss - b['loss']) <= b['E_loss']).all()
        assert (np.abs(got_grad - b['grad']) <= b['E_grad']).all()
    assert np.abs(g['rgb_loss32'] - g['rgb_loss64']).max() > 0.01 * b['E_loss'].max()
    assert not grad32[:, ~(is_r | is_l)].any()

    mloss32 = ro.hand_mean32(g['offset'], g['normal'], is_r, is_l)
    mgrad32 = ro.hand_mean_grad32(g['offset'], g['normal'], g['G_mean'], is_r, is_l)
    m = ro.hand_mean64(g['offset'], g['normal'], is_r, is_l, g['G_mean'])
    sure = ~m['unsure']
    assert sure.sum() >= sure.size - 2
    # (the reference's float64 run rounds eps and the normals differently: compared through the bounds, not exactly)
    for got_loss, got_grad in ((g['mean_loss32'], g['mean_grad32']), (mloss32, mgrad32)):
        assert (np.abs(got_loss - m['loss'])[sure] <= m['E_loss'][sure]).all()
        assert (np.abs(got_grad[:, hand] - m['grad'])[sure] <= m['E_grad'][sure]).all()
        assert not got_grad[:, ~(is_r | is_l)].any()
    # the three special rows: exactly zero (the gradient g * n / eps passes and is finite), norm 1e-13 (divided by eps),
    # against the normal (clamped: no loss, no gradient)
    z, tiny, neg = hand[3], hand[5], hand[7]
    assert not g['offset'][0, z].any() and mloss32[0, 3] == 0
    want = g['G_mean'][0, 3] * g['normal'][z] / np.float32(1e-12)
    assert np.allclose(mgrad32[0, z], want, rtol=1e-6) and np.abs(mgrad32[0, z]).max() > 1e10 and np.isfinite(mgrad32).all()
    assert np.allclose(g['mean_grad32'][0, z], want, rtol=1e-6)
    assert 0 < np.linalg.norm(g['offset'][1, tiny]) < 1e-12 and abs(mloss32[1, 5]) < 0.11
    assert mloss32[0, 7] == 0 and not mgrad32[0, neg].any() and not g['mean_grad32'][0, neg].any()


def test_two_level_mean_is_the_stated_order():
    rng = np.random.RandomState(2)
    rows = rng.uniform(0, 1, (2, 600, 3)).astype(np.float32)
    got = ro.two_level_mean32(rows)
    want = np.zeros((2, 3), dtype=np.float32)
    for c0 in (0, 256, 512):
        p = np.float32(0) * want
        for i in range(c0, min(c0 + 256, 600)):
            p = (p + rows[:, i]).astype(np.float32)
        want = (want + p).astype(np.float32)
    assert np.array_equal(got, (want / np.float32(600)).astype(np.float32))
    R = 256 + 3
    assert (np.abs(got - rows.astype(np.float64).mean(1)) <= R * ro.U * np.abs(rows).sum(1) / 600).all()
    idx, rank = ro.index_tables(np.array([0, 1, 1, 0, 1], dtype=bool))
    assert idx.tolist() == [1, 2, 4] and rank.tolist() == [-1, 0, 1, -1, 2]
