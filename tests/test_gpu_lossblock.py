"""The composed training loss block: every HIP loss module in ONE autograd graph against the reference's own block.

Every module has its own oracle, fixture and GPU test, fed by hand-made leaves.  Here ``tests/loss_case.wire_losses``
writes ``Model.forward``'s training branch (reference ``avatar/main/model.py:195-258``) twice -- ``'dropin'`` as
INTEGRATION.md section 5's drop-in lines give it, ``'fused'`` with ``PhotometricLoss``, ``weight=`` inside the six
``LaplacianReg`` calls and ``arm_neighbors`` / ``arm_rgb_loss`` with the ``plan.count`` formula -- and the results are
compared with ``tests/golden/ref_lossblock_w{0,1}.npz``: what the reference's block, exec'd unchanged in float64 by
``tests/golden/make_golden_lossblock.py``, gives for the same inputs with and without the warm-up, every term's mean,
their sum and autograd's gradient of the sum to every leaf.

No tolerance is a number chosen here.  A gradient may be off by ``FACTOR`` = 4 times what the reference's own float32
run is off against its float64 run (relative L2 and norm-scaled max over the stored entries, floored at 2^-24 of the
norm), as in ``tests/test_gpu_human_chain.py``.  A scalar term's own float32 error is one draw and no scale: its scale is
derived from the float64 run and the modules' stated arithmetic (``loss_case.term_scale``), the
generator asserts that the reference's float32 scalars stay within it, and the HIP scalar is held within 4 times it.  A
dropped or moved constant changes a term by a tenth or more against a scale of 1e-7 of it."""
import os

import numpy as np
import pytest
import torch

from tests import helpers
from tests import loss_case as lc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FACTOR = lc.FACTOR
FLOOR = 2.0 ** -24
CASES = [(v, w) for v in ('dropin', 'fused') for w in (False, True)]


@pytest.fixture(scope='module')
def golden(golden_dir):
    return {w: np.load(os.path.join(golden_dir, 'ref_lossblock_w%d.npz' % w)) for w in (0, 1)}


@pytest.fixture(scope='module')
def model():
    return lc.HipLoss(lc.build_case(), DEV)


def run_block(m, variant, is_warmup):
    """One forward + backward: (terms name -> 0-dim tensor, gradients leaf -> tensor or None, the arm masks)."""
    terms = lc.wire_losses(m, variant, is_warmup)
    grads = torch.autograd.grad(terms['total'], list(m.leaves.values()), allow_unused=True)
    return terms, dict(zip(m.leaves, grads)), m.arm


@pytest.fixture(scope='module')
def runs(model):
    """The four cases, run once and shared."""
    return {c: run_block(model, *c) for c in CASES}


def recorded(g, key):
    return max(float(g[key + '#rel_l2']), FLOOR), max(float(g[key + '#rel_max']), FLOOR)


def ratio(g, leaf, got, ref=None):
    """(HIP error) / (the reference's own float32 error) of one gradient: the largest of the L2 figure and the max figure
    over the stored entries, and the full tensor's norm against the stored norm.  With ``ref`` (a tensor): the same
    figures of ``got`` against it over the full tensor."""
    key = 'grad/' + leaf
    rel_l2, rel_max = recorded(g, key)
    got = got.detach().cpu().double().numpy()
    if ref is None:
        want, full_norm = g[key], float(g[key + '#norm'])
        e = lc.take_sample(leaf, got) - want
    else:
        want = ref.detach().cpu().double().numpy()
        full_norm = float(np.linalg.norm(want))
        e = got - want
    assert e.shape == want.shape, (leaf, e.shape, want.shape)
    norm, n = float(np.linalg.norm(want)), want.size
    assert norm > 0 and full_norm > 0, leaf
    l2 = float(np.linalg.norm(e)) / (rel_l2 * norm)
    mx = float(np.abs(e).max()) / (rel_max * norm / np.sqrt(n))
    full = abs(float(np.linalg.norm(got)) - full_norm) / (rel_l2 * full_norm)
    return max(l2, mx, full)


def check_ratios(tag, res):
    worst = sorted(res.items(), key=lambda kv: -kv[1])
    for k, r in worst:
        print('%s %-40s ratio %.3f' % (tag, k, r))
    helpers.record_stats('lossblock/' + tag, {'max_ratio': worst[0][1], 'at': worst[0][0], 'ratios': res})
    bad = [(k, round(r, 2)) for k, r in worst if not r <= FACTOR]
    assert not bad, '%s: HIP error above %g x the scale: %s' % (tag, FACTOR, bad)


def bits_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


@pytest.mark.parametrize('variant,is_warmup', CASES)
def test_terms_and_gradients_match_the_reference_block(golden, runs, variant, is_warmup):
    g = golden[int(is_warmup)]
    tag = '%s_w%d' % (variant, is_warmup)
    terms, grads, _ = runs[(variant, is_warmup)]
    assert tuple(terms) == (lc.FUSED_TERMS if variant == 'fused' else lc.DROPIN_TERMS) + ('total',)
    res = {}
    for k, v in terms.items():
        assert v.dim() == 0 and v.dtype == torch.float32, k
        res['term/' + k] = abs(float(v.detach().double()) - lc.term_value(g, k)) / lc.term_scale(g, variant, k)
    unreached = set(str(s) for s in g['unreached']) - {''}
    assert unreached == {'rgb_offset'}
    for k, gr in grads.items():
        if k in unreached:
            assert gr is None or not bool(gr.any()), 'leaf %s cannot be reached and has a gradient' % k
            continue
        assert gr is not None, 'leaf %s got no gradient' % k
        assert tuple(gr.shape) == tuple(lc.build_case()[k].shape) and gr.dtype == torch.float32, k
        res['grad/' + k] = ratio(g, k, gr)
    check_ratios(tag, res)


@pytest.mark.parametrize('is_warmup', [False, True])
def test_the_fused_block_equals_the_drop_in_block(golden, runs, is_warmup):
    g = golden[int(is_warmup)]
    (fused, gf, _), (drop, gd, _) = runs[('fused', is_warmup)], runs[('dropin', is_warmup)]
    res = {}
    for k in lc.FUSED_TERMS + ('total',):
        want = sum(float(drop[p].detach().double()) for p in lc.FUSED_PAIRS.get(k, (k,)))
        res['term/' + k] = abs(float(fused[k].detach().double()) - want) / lc.term_scale(g, 'fused', k)
    for k in gd:
        if gd[k] is None or gf[k] is None:
            assert gd[k] is None and gf[k] is None, k
            continue
        res['grad/' + k] = ratio(g, k, gf[k], gd[k])
    check_ratios('fused_vs_dropin_w%d' % is_warmup, res)


def test_the_block_gives_the_same_bits_twice(model, runs):
    for case in CASES:
        terms, grads, arm = runs[case]
        terms2, grads2, arm2 = run_block(model, *case)
        assert [k for k in terms if not bits_equal(terms[k], terms2[k])] == [], case
        assert [k for k in grads if not bits_equal(grads[k], grads2[k])] == [], case
        assert torch.equal(arm[0], arm2[0]) and torch.equal(arm[1], arm2[1])


def test_get_arm_returns_the_fixtures_masks(golden, model, runs):
    for case in CASES:
        up, lo = runs[case][2]
        assert up.dtype == torch.bool and np.array_equal(up.cpu().numpy(), golden[0]['arm/is_upper']), case
        assert np.array_equal(lo.cpu().numpy(), golden[0]['arm/is_lower']), case
    plan = model.plan
    assert int(plan.k) == int(golden[0]['arm/k']) == lc.K_ARM and int(plan.count) == lc.L_ARM
    assert int(plan.upper_count) == lc.U_ARM
    assert np.array_equal(plan.n_valid[:lc.L_ARM].cpu().numpy(), golden[0]['arm/n_valid'])
