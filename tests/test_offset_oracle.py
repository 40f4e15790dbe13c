"""CPU tests of tests/offset_oracle.py, the restatement the GPU test holds the offset regularisers' kernels against: its
maps and gradients equal the torch expressions of the reference's lines on the CPU bit for bit, its float32 means lie within
the bound their summation depth gives of the float64 means, and on the loss block's case they lie within the fixtures'
scales of what the reference's own block gives."""
import os

import numpy as np
import pytest
import torch

from tests import loss_case as lc
from tests import offset_oracle as oo

U24 = 2.0 ** -24
SIZES = [(1, 1, 1, 0), (1, 255, 55, 24), (1, 256, 55, 24), (1, 257, 3, 1), (3, 1000, 300, 140), (1, 65537, 55, 24)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, what
    assert np.array_equal(bits(a), bits(b)), what


def torch_terms(c, leaves=()):
    """The reference's four expressions on CPU tensors: (the maps, the leaves name -> tensor)."""
    t = {k: torch.from_numpy(np.array(v)) for k, v in c.items()}
    for k in leaves:
        t[k].requires_grad_(True)
    wm, ws = t['wm'].reshape(1, -1, 1), t['ws'].reshape(1, -1, 1)
    r, l = t['jo'][t['pr'].tolist()], t['jo'][t['pl'].tolist()]
    out = ((t['mo'] ** 2 + t['moo'] ** 2) * wm, (t['sc'] ** 2 + t['so'] ** 2) * ws, (t['jo'] - t['ref']) ** 2 * t['wj'],
           torch.abs(r[:, 0] + l[:, 0]) + torch.abs(r[:, 1] - l[:, 1]) + torch.abs(r[:, 2] - l[:, 2]))
    return out, {k: t[k] for k in leaves}


LEAVES = ('mo', 'moo', 'sc', 'so', 'jo')


@pytest.mark.parametrize('B,V,J,P', SIZES)
@pytest.mark.parametrize('ch', [1, 3])
def test_the_maps_equal_the_torch_expressions(B, V, J, P, ch):
    c = oo.make_case(10 + ch, B, V, J, P, ch)
    want, _ = torch_terms(c)
    for name, got, w in zip(oo.TERMS, oo.maps(*oo.args(c)), want):
        same_bits(got, w.numpy(), name)


@pytest.mark.parametrize('B,V,J,P', SIZES[:5])
@pytest.mark.parametrize('ch', [1, 3])
@pytest.mark.parametrize('mean', [False, True])
def test_the_gradients_equal_cpu_autograd(B, V, J, P, ch, mean):
    c = oo.make_case(20 + ch, B, V, J, P, ch)
    terms, leaves = torch_terms(c, LEAVES)
    rs = np.random.RandomState(5)
    if mean:
        live = [k for k in range(4) if terms[k].numel()]
        coef = [np.float32(rs.uniform(0.5, 2.0)) if k in live else None for k in range(4)]
        total = sum(terms[k].mean() * float(coef[k]) for k in live)
        got = oo.grads(*oo.args(c), g_means=coef, reciprocal=False)       # the CPU divides by N
    else:
        cot = [rs.standard_normal(t.shape).astype(np.float32) for t in terms]
        total = sum((t * torch.from_numpy(g)).sum() for t, g in zip(terms, cot))
        got = oo.grads(*oo.args(c), g_maps=cot)
    want = torch.autograd.grad(total, [leaves[k] for k in LEAVES])
    for k, w in zip(LEAVES, want):
        if k == 'so' and ch == 1:
            # bit for bit on every row with a weight; where the weight is 0 (the cavity's) all three addends are zeros, and
            # torch starts its three-channel sum from +0 in some lanes and not in others: that zero's sign is torch's own
            live = c['ws'] != 0
            same_bits(got[k][:, live], w.numpy()[:, live], 'dL/dso')
            assert not got[k][:, ~live].any() and not w.numpy()[:, ~live].any()
        else:
            same_bits(got[k], w.numpy(), 'dL/d' + k)


def test_a_term_without_a_cotangent_reaches_nothing():
    c = oo.make_case(3, 2, 40, 55, 24)
    g = oo.grads(*oo.args(c), g_means=[None, None, None, 1.0])
    assert all(g[k] is None for k in ('mo', 'moo', 'sc', 'so'))
    paired = np.zeros(55, bool)
    paired[c['pr']] = paired[c['pl']] = True
    assert not g['jo'][~paired].any() and np.abs(g['jo'][paired]).min() > 0
    g = oo.grads(*oo.args(c), g_means=[1.0, None, None, None])
    assert g['jo'] is None and g['sc'] is None and g['mo'] is not None


def test_sign_of_zero_is_zero():
    c = oo.make_case(4, 1, 8, 6, 2)
    jo = np.array(c['jo'])
    r, l = int(c['pr'][0]), int(c['pl'][0])
    jo[l, 0] = -jo[r, 0]                                          # x_R + x_L == 0 exactly
    jo[l, 1] = jo[r, 1]
    c['jo'] = jo
    g = oo.grads(*oo.args(c), g_maps=[None, None, None, np.ones(2, np.float32)])['jo']
    assert g[r, 0] == 0 and g[l, 0] == 0 and g[r, 1] == 0 and g[l, 1] == 0
    assert abs(g[r, 2]) == 1 and g[l, 2] == -g[r, 2]
    terms, leaves = torch_terms(c, ('jo',))
    assert np.array_equal(torch.autograd.grad(terms[3].sum(), leaves['jo'])[0].numpy(), g)


@pytest.mark.parametrize('B,V,J,P', SIZES)
def test_the_means_lie_within_their_depth_of_float64(B, V, J, P):
    c = oo.make_case(30, B, V, J, P)
    got, exact = oo.means32(oo.maps(*oo.args(c))), oo.means64(*oo.args(c))
    for k, d in enumerate(oo.mean_depth(B, V, J, P)):
        if np.isnan(exact[k]):
            assert np.isnan(got[k]) and P == 0 and k == 3
            continue
        assert exact[k] >= 0
        if exact[k] == 0:                                         # (one vertex, and its weight drawn 0)
            assert got[k] == 0
            continue
        rel = abs(float(got[k]) - exact[k]) / exact[k]
        print('%s B %d V %d: rel %.3g bound %.3g' % (oo.TERMS[k], B, V, rel, (d + 2) * U24))
        assert rel <= (d + 2) * U24, (oo.TERMS[k], rel, d)


def test_blocks_and_depth():
    assert [oo.blocks(*s) for s in ((1, 1), (1, 256), (1, 257), (2, 3202), (1, 65537), (0, 5), (5, 0), (-1, 5))] \
        == [1, 1, 2, 26, 257, 0, 0, 0]
    assert oo.mean_depth(1, 65537, 55, 24) == [2 + 9 + 2 + 9, 2 + 9 + 2 + 9, 1 + 9, 1 + 9]
    assert oo.mean_depth(1, 100, 300, 140)[2:] == [4 + 9, 1 + 9]


@pytest.mark.parametrize('warmup', [0, 1])
def test_the_means_of_the_loss_blocks_case_lie_within_the_fixtures_scales(golden_dir, warmup):
    """Both fixtures: the warm-up's ``scale_wo_clamp`` is the same pre-clamp scale the other branch reads."""
    g = np.load(os.path.join(golden_dir, 'ref_lossblock_w%d.npz' % warmup))
    c = oo.block_case()
    got = oo.means32(oo.maps(*oo.args(c)))
    for k, name in enumerate(oo.TERMS):
        ratio = abs(float(got[k]) - lc.term_value(g, name)) / lc.term_scale(g, 'fused', name)
        print('w%d %-22s %.3f scales' % (warmup, name, ratio))
        assert ratio <= lc.FACTOR, (name, ratio)
