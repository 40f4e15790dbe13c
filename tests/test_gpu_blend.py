"""The HIP blend-shape offsets (exavatar_release_amd.BlendShapes / blend_offsets) on the GPU.

The outputs, dL/dbase and dL/dcoef must equal the float32 oracle tests/blend_oracle.py BIT FOR BIT: the header fixes
every rounding, the K-segments of the forward and the two-level sum of the backward.  (Where no column covers an output
the result is a copy or a zero, and -0.0 counts as +0.0 there; covered elements are compared by their bits alone.)
Against the reference's own code (the golden, float64) the results stay within one derived bound; against the reference
expressions run by PyTorch on the same device -- on the uncompacted tables -- within two, since both sides are float32.
The backward repeats bit for bit, a captured graph replays with new inputs, and nothing changes under
``config.poison``.  torch.autograd.gradcheck is of no use in float32; the float64 oracle, which
tests/test_blend_oracle.py checks against autograd, stands in for it.

The full-size coverage shares are assumptions: SMPL-X's hands are 2 x 778 of its 10 475 vertices and the face-expression
set is recalled as roughly a quarter of the mesh, which puts the pose mask near 40 % of the upsampled mesh; 15 % is
taken for the vertices with a non-zero expression row.  The licensed SMPL-X assets are not part of this repository, so
neither share is checked against them."""
import os

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd.blend_shapes import BlendShapes, BlendTable, blend_offsets, make_table
from tests import blend_oracle as bo

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_blend.npz')
V_FULL = 167281      # the reference's upsampled human mesh


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want, what, zero_sign_free=None):
    """Bit equality; where ``zero_sign_free`` (uncovered elements) -0.0 counts as +0.0."""
    got, want = np.asarray(got, dtype=np.float32).reshape(-1), np.asarray(want, dtype=np.float32).reshape(-1)
    assert got.shape == want.shape, what
    bad = _bits(got) != _bits(want)
    if zero_sign_free is not None:
        bad &= ~(zero_sign_free & (got == 0) & (want == 0))
    assert not bad.any(), '%s: %d of %d elements differ in their bits' % (what, int(bad.sum()), bad.size)


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _device_plan(plan):
    return BlendTable(*[_t(a) for a in plan])


def _run(plan, coef, base, g_out, g_masked):
    """blend_offsets on the device with gradients -> numpy (out, masked, dcoef, dbase)."""
    c = _t(coef).requires_grad_(True)
    if base is None:
        out = blend_offsets(c, plan)
        dcoef, = torch.autograd.grad(out, c, _t(g_out))
        return out.detach().cpu().numpy(), None, dcoef.cpu().numpy(), None
    b = _t(base).requires_grad_(True)
    out, masked = blend_offsets(c, plan, b)
    dcoef, dbase = torch.autograd.grad([out, masked], [c, b], [_t(g_out), _t(g_masked)])
    return out.detach().cpu().numpy(), masked.detach().cpu().numpy(), dcoef.cpu().numpy(), dbase.cpu().numpy()


def _check_against_oracle(c, plan_np, plan_dev, what, with_base=True):
    table, cols, inv = plan_np
    unc = inv < 0
    base = c['base'] if with_base else None
    g_masked = c['g_masked'] if with_base else None
    out, masked, dcoef, dbase = _run(plan_dev, c['coef'], base, c['g_out'], g_masked)
    out32, masked32 = bo.forward32(c['coef'], table, cols, inv, base)
    dcoef32, dbase32 = bo.backward32(table, cols, inv, c['g_out'], g_masked)
    _same_bits(out, out32, what + ' out', unc)
    _same_bits(dcoef, dcoef32, what + ' dL/dcoef')
    if with_base:
        _same_bits(masked, masked32, what + ' masked', unc)
        _same_bits(dbase, dbase32, what + ' dL/dbase', unc)
        assert not masked[~unc].any() and not np.signbit(masked[~unc]).any()         # +0.0 where covered
    else:
        assert not out[unc].any() and not np.signbit(out[unc]).any()                 # +0.0 where uncovered


@pytest.mark.parametrize('K', [1, 50, 486, 512])
@pytest.mark.parametrize('V', [1, 63, 64, 65, 4097])
def test_forward_and_backward_equal_the_fp32_oracle_bit_for_bit(V, K):
    for coverage in bo.COVERAGES:                                  # none, one vertex, random 40 %, all
        c = bo.random_case(K, V, coverage, seed=7 * V + K)
        plan_np = bo.plan(c['dirs'], bo.pose_keep(c['mask']))
        plan_dev = make_table(_t(c['dirs']), _t(bo.pose_keep(c['mask'])))
        for got, want in zip(plan_dev, plan_np):                   # the plan built on the device is the oracle's
            assert np.array_equal(got.cpu().numpy(), want)
        for with_base in (True, False):
            _check_against_oracle(c, plan_np, plan_dev, 'K=%d V=%d %s base=%s' % (K, V, coverage, with_base), with_base)


def test_within_one_bound_of_the_reference_golden():
    z = np.load(GOLDEN)
    for name in z['pose_cases']:
        p = str(name) + '_'
        V = z[p + 'pose_mask'].shape[0]
        m = BlendShapes(_t(z[p + 'pose_dirs']), torch.zeros(V, 3, 1, device=DEV), _t(z[p + 'pose_mask']))
        moo = _t(z[p + 'mean_offset_offset']).requires_grad_(True)
        combined, masked = m.pose_offsets(_t(z[p + 'pose_feat']), moo)
        grad, = torch.autograd.grad([combined, masked], moo, [_t(z[p + 'G_combined']), _t(z[p + 'G_masked'])])
        plan = bo.plan(z[p + 'pose_dirs'], bo.pose_keep(z[p + 'pose_mask']))
        f = bo.forward64(z[p + 'pose_feat'], *plan, z[p + 'mean_offset_offset'])
        b = bo.backward64(*plan, z[p + 'G_combined'], z[p + 'G_masked'])
        err = np.abs(combined.detach().cpu().numpy().astype(np.float64) - z[p + 'combined']).reshape(-1)
        gerr = np.abs(grad.cpu().numpy().astype(np.float64) - z[p + 'grad_mean_offset_offset']).reshape(-1)
        print('golden %s: combined max err %.3e (max bound %.3e), grad max err %.3e (max bound %.3e)'
              % (name, err.max(), f['E_out'].max(), gerr.max(), b['E_dbase'].max()))
        assert (err <= f['E_out']).all(), name
        assert np.array_equal(masked.detach().cpu().numpy().astype(np.float64), z[p + 'masked']), name    # zeros compare equal
        assert (gerr <= b['E_dbase']).all(), name
    V = z['expr_expr_dirs'].shape[0]
    m = BlendShapes(torch.zeros(1, 3 * V, device=DEV), _t(z['expr_expr_dirs']), torch.zeros(V, dtype=torch.bool, device=DEV))
    expr = _t(z['expr_expr']).requires_grad_(True)
    off = m.expr_offsets(expr)
    grad, = torch.autograd.grad(off, expr, _t(z['expr_G']))
    plan = bo.plan(*bo.expr_full(z['expr_expr_dirs']))
    f = bo.forward64(z['expr_expr'], *plan)
    b = bo.backward64(*plan, z['expr_G'])
    err = np.abs(off.detach().cpu().numpy().astype(np.float64) - z['expr_offset']).reshape(-1)
    gerr = np.abs(grad.cpu().numpy().astype(np.float64) - z['expr_grad_expr'])
    print('golden expr: offset max err %.3e (max bound %.3e), grad max err %.3e (max bound %.3e)'
          % (err.max(), f['E_out'].max(), gerr.max(), b['E_dcoef'].max()))
    assert (err <= f['E_out']).all() and (gerr <= b['E_dcoef']).all()
    assert not off.detach().cpu().numpy().reshape(-1)[plan[2] < 0].any()


@pytest.fixture(scope='module')
def full_size():
    """V = 167 281: pose_dirs [486, 3 V] (976 MB) with 40 % of the vertices masked, expr_dirs [V, 3, 50] non-zero on 15 %.
    Generated on the device in fp32; the oracle works on the compact tables the module built, and the module's plan is
    checked against the oracle's plan of the full tables."""
    g = torch.Generator(device=DEV).manual_seed(1)
    V = V_FULL
    pose_dirs = torch.randn(486, 3 * V, generator=g, device=DEV) * 0.02
    sel = torch.rand(V, generator=g, device=DEV)
    pose_mask = sel < 0.4
    expr_dirs = torch.randn(V, 3, 50, generator=g, device=DEV) * 0.05
    expr_dirs *= (torch.rand(V, generator=g, device=DEV) < 0.15)[:, None, None]
    m = BlendShapes(pose_dirs, expr_dirs, pose_mask)
    rnd = lambda *s: torch.randn(*s, generator=g, device=DEV)      # noqa: E731
    data = dict(pose_feat=rnd(1, 486) * 0.3, moo=rnd(V, 3) * 0.01, expr=rnd(50), G1=rnd(V, 3), G2=rnd(V, 3))
    return m, pose_dirs, expr_dirs, pose_mask, data


def test_full_size_plan_equals_the_oracle_plan(full_size):
    m, pose_dirs, expr_dirs, pose_mask, _ = full_size
    assert not m.state_dict() and m.pose_table.device.type == 'cuda'
    N = 3 * int(pose_mask.sum())
    assert 0.39 < N / (3.0 * V_FULL) < 0.41 and m.pose_table.shape == (486, (N + 3) // 4 * 4)
    mask = pose_mask.cpu().numpy()
    cols = np.flatnonzero(bo.pose_keep(mask)).astype(np.int32)
    assert np.array_equal(m.pose_cols.cpu().numpy(), cols)
    inv = np.full(3 * V_FULL, -1, dtype=np.int32)
    inv[cols] = np.arange(cols.size, dtype=np.int32)
    assert np.array_equal(m.pose_inv.cpu().numpy(), inv)
    assert torch.equal(m.pose_table[:, :N], pose_dirs[:, m.pose_cols.long()]) and not m.pose_table[:, N:].any()
    want = bo.plan(*bo.expr_full(expr_dirs.cpu().numpy()))
    for got, w in zip(m.expr_plan, want):
        assert np.array_equal(got.cpu().numpy(), w)
    assert 0.14 < want[1].size / (3.0 * V_FULL) < 0.16


def test_full_size_pose_correctives_equal_the_oracle_and_lie_within_twice_the_bound_of_torch(full_size):
    m, pose_dirs, _, pose_mask, d = full_size
    V = V_FULL
    plan = tuple(t.cpu().numpy() for t in m.pose_plan)
    unc = plan[2] < 0
    moo = d['moo'].clone().requires_grad_(True)
    combined, masked = m.pose_offsets(d['pose_feat'], moo)
    grad, = torch.autograd.grad([combined, masked], moo, [d['G1'], d['G2']])
    feat, base = d['pose_feat'].cpu().numpy(), d['moo'].cpu().numpy().reshape(-1)
    out32, masked32 = bo.forward32(feat, *plan, base)
    _same_bits(combined.detach().cpu().numpy(), out32, 'full-size combined', unc)
    _same_bits(masked.detach().cpu().numpy(), masked32, 'full-size masked', unc)
    g1, g2 = d['G1'].cpu().numpy().reshape(-1), d['G2'].cpu().numpy().reshape(-1)
    dcoef32, dbase32 = bo.backward32(*plan, g1, g2)
    _same_bits(grad.cpu().numpy(), dbase32, 'full-size dL/dmean_offset_offset', unc)
    # the functional form with a coefficient gradient (the reference detaches the pose; a caller need not)
    coef = d['pose_feat'].reshape(-1).clone().requires_grad_(True)
    o2, _ = blend_offsets(coef, m.pose_plan, d['moo'])
    dcoef, = torch.autograd.grad(o2, coef, d['G1'].reshape(-1))
    assert torch.equal(o2.view(V, 3), combined)
    _same_bits(dcoef.cpu().numpy(), dcoef32, 'full-size dL/dcoef')
    # module.py:484-493 by PyTorch on the same device, against the uncompacted 976 MB pose_dirs
    ref_moo = d['moo'].clone().requires_grad_(True)
    mask = pose_mask[:, None].float()
    ref_offset = torch.matmul(d['pose_feat'].detach(), pose_dirs).view(V, 3)
    ref_masked = ref_moo * (1 - mask)
    ref_combined = ref_masked + ref_offset * mask
    ref_grad, = torch.autograd.grad([ref_combined, ref_masked], ref_moo, [d['G1'], d['G2']])
    f = bo.forward64(feat, *plan, base)
    b = bo.backward64(*plan, g1, g2)
    err = np.abs(combined.detach().cpu().numpy().astype(np.float64) - ref_combined.detach().cpu().numpy()).reshape(-1)
    own = np.abs(combined.detach().cpu().numpy().astype(np.float64).reshape(-1) - f['out'])
    gerr = np.abs(grad.cpu().numpy().astype(np.float64) - ref_grad.cpu().numpy()).reshape(-1)
    print('torch on the device, pose: combined max diff %.3e, own max err %.3e (max bound %.3e); grad max diff %.3e'
          % (err.max(), own.max(), f['E_out'].max(), gerr.max()))
    assert (own <= f['E_out']).all()
    assert (err <= 2 * f['E_out']).all()
    assert np.array_equal(masked.detach().cpu().numpy(), ref_masked.detach().cpu().numpy())          # zeros compare equal
    assert (gerr <= 2 * b['E_dbase']).all()
    own = np.abs(dcoef.cpu().numpy().astype(np.float64) - b['dcoef'])
    assert (own <= b['E_dcoef']).all()


def test_full_size_expression_offsets_equal_the_oracle_and_lie_within_twice_the_bound_of_torch(full_size):
    m, _, expr_dirs, _, d = full_size
    plan = tuple(t.cpu().numpy() for t in m.expr_plan)
    unc = plan[2] < 0
    expr = d['expr'].clone().requires_grad_(True)
    off = m.expr_offsets(expr)
    grad, = torch.autograd.grad(off, expr, d['G1'])
    e, g1 = d['expr'].cpu().numpy(), d['G1'].cpu().numpy().reshape(-1)
    out32, _ = bo.forward32(e, *plan)
    dcoef32, _ = bo.backward32(*plan, g1)
    _same_bits(off.detach().cpu().numpy(), out32, 'full-size expression offset', unc)
    _same_bits(grad.cpu().numpy(), dcoef32, 'full-size dL/dexpr')
    # module.py:537 by PyTorch on the same device, on the full expr_dirs
    ref_expr = d['expr'].clone().requires_grad_(True)
    ref = (ref_expr[None, None, :] * expr_dirs).sum(2)
    ref_grad, = torch.autograd.grad(ref, ref_expr, d['G1'])
    f = bo.forward64(e, *plan)
    b = bo.backward64(*plan, g1)
    err = np.abs(off.detach().cpu().numpy().astype(np.float64) - ref.detach().cpu().numpy()).reshape(-1)
    gerr = np.abs(grad.cpu().numpy().astype(np.float64) - ref_grad.cpu().numpy())
    own = np.abs(off.detach().cpu().numpy().astype(np.float64).reshape(-1) - f['out'])
    gown = np.abs(grad.cpu().numpy().astype(np.float64) - b['dcoef'])
    print('torch on the device, expr: offset max diff %.3e, own max err %.3e (max bound %.3e); grad max diff %.3e, own '
          'max err %.3e (min bound %.3e)' % (err.max(), own.max(), f['E_out'].max(), gerr.max(), gown.max(), b['E_dcoef'].min()))
    assert (own <= f['E_out']).all() and (gown <= b['E_dcoef']).all()
    assert (err <= 2 * f['E_out']).all()
    assert (gerr <= 2 * b['E_dcoef']).all()


def test_backward_repeats_bit_for_bit(full_size):
    m, _, _, _, d = full_size
    grads = []
    for _ in range(3):
        expr = d['expr'].clone().requires_grad_(True)
        coef = d['pose_feat'].reshape(-1).clone().requires_grad_(True)
        moo = d['moo'].clone().requires_grad_(True)
        off = m.expr_offsets(expr)
        out, masked = blend_offsets(coef, m.pose_plan, moo)
        g = torch.autograd.grad([off, out, masked], [expr, coef, moo], [d['G1'], d['G1'].reshape(-1), d['G2'].reshape(-1)])
        grads.append([x.cpu().numpy() for x in g])
    for again in grads[1:]:
        for a, b, what in zip(again, grads[0], ('dL/dexpr', 'dL/dcoef', 'dL/dbase')):
            _same_bits(a, b, 'repeated ' + what)


def test_graph_capture_replays_forward_and_backward_with_new_inputs(full_size):
    m, _, _, _, d = full_size
    V = V_FULL
    expr = d['expr'].clone().requires_grad_(True)
    feat = d['pose_feat'].clone()
    moo = d['moo'].clone().requires_grad_(True)
    G1, G2 = d['G1'].clone(), d['G2'].clone()

    def step():
        combined, masked = m.pose_offsets(feat, moo)
        off = m.expr_offsets(expr)
        g_expr, g_moo = torch.autograd.grad([combined, masked, off], [expr, moo], [G1, G2, G1])
        return combined, masked, off, g_expr, g_moo

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    g = torch.Generator(device=DEV).manual_seed(77)
    with torch.no_grad():
        expr.copy_(torch.randn(50, generator=g, device=DEV))
        feat.copy_(torch.randn(1, 486, generator=g, device=DEV) * 0.3)
        moo.copy_(torch.randn(V, 3, generator=g, device=DEV) * 0.01)
        G1.copy_(torch.randn(V, 3, generator=g, device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    for a, b, what in zip(captured, eager, ('combined', 'masked', 'expr offset', 'dL/dexpr', 'dL/dmean_offset_offset')):
        _same_bits(a.detach().cpu().numpy(), b.detach().cpu().numpy(), 'replayed ' + what)
    plan = tuple(t.cpu().numpy() for t in m.pose_plan)
    out32, _ = bo.forward32(feat.cpu().numpy(), *plan, moo.detach().cpu().numpy().reshape(-1))
    _same_bits(captured[0].detach().cpu().numpy(), out32, 'replayed combined against the oracle', plan[2] < 0)
    eplan = tuple(t.cpu().numpy() for t in m.expr_plan)
    _same_bits(captured[3].cpu().numpy(), bo.backward32(*eplan, G1.cpu().numpy().reshape(-1))[0], 'replayed dL/dexpr')


def test_results_are_the_same_with_poisoned_workspaces():
    """``config.poison`` (what EXA_TEST_POISON=1 sets for the whole suite) fills the backward's workspace with 0xFF first."""
    c = bo.random_case(50, 4097, 'random', seed=5)
    plan_np = bo.plan(c['dirs'], bo.pose_keep(c['mask']))
    plan_dev = _device_plan(plan_np)
    plain = _run(plan_dev, c['coef'], c['base'], c['g_out'], c['g_masked'])
    exa.config.poison = True
    poisoned = _run(plan_dev, c['coef'], c['base'], c['g_out'], c['g_masked'])
    for a, b, what in zip(plain, poisoned, ('out', 'masked', 'dL/dcoef', 'dL/dbase')):
        _same_bits(a, b, 'poisoned ' + what)
    _check_against_oracle(c, plan_np, plan_dev, 'poisoned')


def test_python_surface_on_the_device():
    rng = np.random.RandomState(3)
    V = 30
    pose_dirs, expr_dirs = rng.standard_normal((18, 3 * V)).astype(np.float32), rng.standard_normal((V, 3, 5)).astype(np.float32)
    mask = rng.rand(V) < 0.5
    cpu = BlendShapes(torch.from_numpy(pose_dirs), torch.from_numpy(expr_dirs), torch.from_numpy(mask))
    m = cpu.to(DEV)                                               # .to() moves the compact tables
    assert m.pose_table.is_cuda and m.expr_inv.is_cuda and not m.state_dict()
    feat, moo, expr = torch.randn(18, device=DEV), torch.randn(V, 3, device=DEV), torch.randn(5, device=DEV)
    a = m.pose_offsets(feat, moo)
    b = m.pose_offsets(feat.view(1, 18).clone().requires_grad_(True), moo)       # [1, Kp]; detached as in the reference
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].shape == (V, 3) and not b[0].requires_grad
    assert m.expr_offsets(expr).shape == (V, 3)
    with pytest.raises(ValueError, match='float32'):
        m.expr_offsets(expr.double())
    with pytest.raises(ValueError, match=r'coef must be \[K\] or \[1, K\]'):
        m.expr_offsets(torch.randn(6, device=DEV))
    with pytest.raises(ValueError, match=r'coef must be \[K\] or \[1, K\]'):
        m.pose_offsets(torch.randn(2, 9, device=DEV), moo)
    with pytest.raises(ValueError, match='base must have M'):
        blend_offsets(feat, m.pose_plan, moo[:-1])
    with pytest.raises(ValueError, match='not on the device of coef'):
        blend_offsets(feat, cpu_plan(pose_dirs, mask))
    with pytest.raises(RuntimeError, match='no CPU path'):
        m.expr_offsets(expr.cpu())
    # a non-contiguous base is made contiguous
    wide = torch.randn(V, 6, device=DEV)
    assert torch.equal(m.pose_offsets(feat, wide[:, ::2])[0], m.pose_offsets(feat, wide[:, ::2].contiguous())[0])
    assert exa.BlendShapes is BlendShapes


def cpu_plan(pose_dirs, mask):
    return make_table(torch.from_numpy(pose_dirs), torch.from_numpy(bo.pose_keep(mask)))
