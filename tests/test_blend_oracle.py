"""CPU tests of the blend-shape oracles (tests/blend_oracle.py): the float64 oracle equals autograd of the two reference
expressions written in torch float64, the float32 op-by-op oracle lies within the derived bound of it, the bound is the
stated function of the inputs, and the plan has the properties the header promises.  The reference's own code, exec'd
unchanged, is the golden (tests/golden/ref_blend.npz); the float64 oracle reproduces it."""
import os

import numpy as np
import pytest
import torch

import exavatar_release_amd.blend_shapes as bs
from tests import blend_oracle as bo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_blend.npz')
CASES = [(1, 1, 'all'), (1, 5, 'none'), (50, 65, 'random'), (63, 200, 'one'), (486, 64, 'random'), (512, 33, 'all'),
         (7, 700, 'random')]


def _plan(c):
    return bo.plan(c['dirs'], bo.pose_keep(c['mask']))


@pytest.mark.parametrize('K,V,coverage', CASES)
def test_float64_oracle_equals_autograd_of_the_reference_expressions(K, V, coverage):
    c = bo.random_case(K, V, coverage, seed=K + V)
    table, cols, inv = _plan(c)
    # module.py:485-493 in torch float64
    dirs = torch.from_numpy(c['dirs']).double()
    mask = torch.from_numpy(c['mask'])[:, None].double()
    base = torch.from_numpy(c['base']).double().view(V, 3).requires_grad_(True)
    coef = torch.from_numpy(c['coef']).double().view(1, K).requires_grad_(True)
    offset = torch.matmul(coef, dirs).view(V, 3)
    masked = base * (1 - mask)
    combined = masked + offset * mask
    G1, G2 = torch.from_numpy(c['g_out']).double().view(V, 3), torch.from_numpy(c['g_masked']).double().view(V, 3)
    gcoef, gbase = torch.autograd.grad([combined, masked], [coef, base], [G1, G2])
    f = bo.forward64(c['coef'], table, cols, inv, c['base'])
    b = bo.backward64(table, cols, inv, c['g_out'], c['g_masked'])
    tiny = 1e-12
    assert np.abs(f['out'] - combined.detach().numpy().reshape(-1)).max() <= tiny * max(1.0, np.abs(f['out']).max())
    assert np.array_equal(f['masked'], masked.detach().numpy().reshape(-1))           # zeros compare equal
    assert np.abs(b['dcoef'] - gcoef.numpy().reshape(-1)).max() <= tiny * max(1.0, np.abs(b['dcoef']).max())
    assert np.array_equal(b['dbase'], gbase.numpy().reshape(-1))
    # module.py:537 in torch float64, on the same matrix as [V, 3, K] with the uncovered rows zero
    e = (c['dirs'] * bo.pose_keep(c['mask'])[None, :]).T.reshape(V, 3, K)
    full, keep = bo.expr_full(e)
    et, ec, ei = bo.plan(full, keep)
    expr = torch.from_numpy(c['coef']).double().requires_grad_(True)
    off = (expr[None, None, :] * torch.from_numpy(e).double()).sum(2)
    gexpr, = torch.autograd.grad(off, expr, G1)
    f2 = bo.forward64(c['coef'], et, ec, ei)
    b2 = bo.backward64(et, ec, ei, c['g_out'])
    assert f2['masked'] is None
    assert np.abs(f2['out'] - off.detach().numpy().reshape(-1)).max() <= tiny * max(1.0, np.abs(f2['out']).max())
    assert np.abs(b2['dcoef'] - gexpr.numpy()).max() <= tiny * max(1.0, np.abs(b2['dcoef']).max())


@pytest.mark.parametrize('K,V,coverage', CASES)
def test_float32_oracle_lies_within_the_derived_bound(K, V, coverage):
    c = bo.random_case(K, V, coverage, seed=3 * K + V)
    table, cols, inv = _plan(c)
    out, masked = bo.forward32(c['coef'], table, cols, inv, c['base'])
    dcoef, dbase = bo.backward32(table, cols, inv, c['g_out'], c['g_masked'])
    assert out.dtype == masked.dtype == dcoef.dtype == dbase.dtype == np.float32
    f = bo.forward64(c['coef'], table, cols, inv, c['base'])
    b = bo.backward64(table, cols, inv, c['g_out'], c['g_masked'])
    assert (np.abs(out - f['out']) <= f['E_out']).all()
    assert np.array_equal(masked, f['masked'])
    assert (np.abs(dcoef - b['dcoef']) <= b['E_dcoef']).all()
    assert (np.abs(dbase - b['dbase']) <= b['E_dbase']).all()
    # uncovered outputs are copies, covered masked outputs +0.0
    unc = inv < 0
    assert np.array_equal(out[unc], c['base'][unc]) and not np.signbit(masked[~unc]).any() and (f['E_out'][unc] == 0).all()
    # without a base: +0.0 where uncovered, the same sums where covered
    out0, none = bo.forward32(c['coef'], table, cols, inv)
    assert none is None and not out0[unc].any() and not np.signbit(out0[unc]).any()
    assert np.array_equal(out0[~unc], out[~unc])
    # without g_masked dL/dbase is g_out where uncovered
    assert np.array_equal(bo.backward32(table, cols, inv, c['g_out'])[1][unc], c['g_out'][unc])


def test_the_bound_is_the_stated_function_of_the_inputs():
    assert bo.U == 2.0 ** -24 and bo.gamma(486) == 486 * bo.U / (1 - 486 * bo.U)
    c = bo.random_case(50, 40, 'random', seed=9)
    table, cols, inv = _plan(c)
    f = bo.forward64(c['coef'], table, cols, inv)
    want = bo.gamma(50) * (np.abs(c['coef'].astype(np.float64))[:, None] * np.abs(c['dirs'].astype(np.float64))).sum(0)
    assert np.allclose(f['E_out'][cols], want[cols], rtol=1e-12, atol=0)
    b = bo.backward64(table, cols, inv, c['g_out'])
    g = c['g_out'].astype(np.float64)[cols]
    want = bo.gamma(cols.size) * (np.abs(c['dirs'].astype(np.float64)[:, cols]) * np.abs(g)[None, :]).sum(1)
    assert np.allclose(b['E_dcoef'], want, rtol=1e-12, atol=0)


def test_the_summation_order_depends_on_k_alone():
    """The same column gives the same bits whatever stands next to it: alone, among 64, among 5 000."""
    K = 486
    rng = np.random.RandomState(2)
    dirs = rng.standard_normal((K, 3 * 5000)).astype(np.float32)
    coef = rng.standard_normal(K).astype(np.float32)
    j = 3 * 1234 + 1
    results = []
    for V in (5000, 1235):
        for mask in (np.ones(V, bool), np.arange(V) == 1234, np.arange(V) % 3 == 1):
            t, cols, inv = bo.plan(dirs[:, :3 * V], bo.pose_keep(mask))
            results.append(bo.forward32(coef, t, cols, inv)[0][j])
    assert len(set(np.array(results, dtype=np.float32).view(np.uint32).tolist())) == 1


@pytest.mark.parametrize('coverage', bo.COVERAGES)
@pytest.mark.parametrize('V', [1, 2, 63, 64, 65, 1000])
def test_plan_properties(V, coverage):
    c = bo.random_case(5, V, coverage, seed=V)
    table, cols, inv = _plan(c)
    N, M = cols.size, 3 * V
    assert N == 3 * int(c['mask'].sum()) and (coverage != 'none' or N == 0) and (coverage != 'all' or N == M)
    assert table.dtype == np.float32 and cols.dtype == np.int32 and inv.dtype == np.int32
    assert table.shape == (5, (N + 3) // 4 * 4) and table.shape[1] % 4 == 0 and table.shape[1] - N < 4
    assert (np.diff(cols) > 0).all()                                         # ascending
    assert inv.shape == (M,) and np.array_equal(inv[cols], np.arange(N))     # inverse to each other ...
    assert ((inv >= 0).sum() == N) and (inv >= -1).all() and (inv < max(N, 1)).all()
    assert np.array_equal(cols[inv[inv >= 0]], np.flatnonzero(inv >= 0))     # ... both ways
    assert not table[:, N:].any()                                            # pad columns are zero
    assert np.array_equal(table[:, :N], c['dirs'][:, cols])
    # the three channels of every masked vertex, whole vertices only
    assert np.array_equal((inv >= 0).reshape(V, 3), np.repeat(c['mask'][:, None], 3, 1))
    # the module's own plan (make_table, on the CPU) is the oracle's
    got = bs.make_table(torch.from_numpy(c['dirs']), torch.from_numpy(bo.pose_keep(c['mask'])))
    assert all(np.array_equal(a.numpy(), b) and a.numpy().dtype == b.dtype for a, b in zip(got, (table, cols, inv)))


def test_expression_plan_keeps_the_vertices_whose_row_has_a_non_zero():
    rng = np.random.RandomState(4)
    V, Ke = 50, 6
    e = rng.standard_normal((V, 3, Ke)).astype(np.float32)
    live = rng.rand(V) < 0.3
    e[~live] = 0
    one = int(np.flatnonzero(~live)[0])
    e[one, 2, 4] = 1e-30                     # a single non-zero entry keeps all three channels of its vertex
    live[one] = True
    e[np.flatnonzero(live)[1], 0, :] = 0      # a zero channel of a live vertex stays (whole vertices)
    full, keep = bo.expr_full(e)
    assert full.shape == (Ke, 3 * V) and np.array_equal(keep, np.repeat(live, 3))
    assert np.array_equal(full[:, 3 * 7 + 1], e[7, 1, :])
    table, cols, inv = bo.plan(full, keep)
    assert cols.size == 3 * live.sum()


def test_float64_oracle_reproduces_the_reference_golden():
    z = np.load(GOLDEN)
    for name in z['pose_cases']:
        p = str(name) + '_'
        table, cols, inv = bo.plan(z[p + 'pose_dirs'], bo.pose_keep(z[p + 'pose_mask']))
        f = bo.forward64(z[p + 'pose_feat'], table, cols, inv, z[p + 'mean_offset_offset'])
        b = bo.backward64(table, cols, inv, z[p + 'G_combined'], z[p + 'G_masked'])
        assert np.abs(f['out'] - z[p + 'combined'].reshape(-1)).max() <= 1e-15
        assert np.array_equal(f['masked'], z[p + 'masked'].reshape(-1))
        assert np.array_equal(b['dbase'], z[p + 'grad_mean_offset_offset'].reshape(-1))
    assert z['smplx_pose_feat'].shape == (1, 486)
    full, keep = bo.expr_full(z['expr_expr_dirs'])
    assert 0 < keep.sum() < keep.size
    table, cols, inv = bo.plan(full, keep)
    f = bo.forward64(z['expr_expr'], table, cols, inv)
    b = bo.backward64(table, cols, inv, z['expr_G'])
    assert np.abs(f['out'] - z['expr_offset'].reshape(-1)).max() <= 1e-15
    assert np.abs(b['dcoef'] - z['expr_grad_expr']).max() <= 1e-13
