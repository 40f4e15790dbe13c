"""The offset regularisers on the device: ``OffsetRegs`` against its CPU restatement (tests/offset_oracle.py) bit for bit, in
map mode and in mean mode, at the sizes where the kernels' work split changes; against the torch expressions of the
reference's lines on the device; and against the reference's own block (tests/golden/ref_lossblock_w{0,1}.npz).

The one figure that is not an equality: the gradient of a ``[B, V, 1]`` ``scale_offset`` against torch's.  Both add the three
products ``g_c w (2 so)`` of a row; the header adds ``(g0 w + g1 w) + g2 w`` and multiplies once, torch's device sum has an
order of its own.  Three float32 additions and a product differ by at most ``4 * 2^-24 * sum_c |g_c w| |2 so|``."""
import os
import sys

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from tests import loss_case as lc
from tests import offset_oracle as oo
from tests import test_gpu_lossblock as block

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U24 = 2.0 ** -24
module = sys.modules['exavatar_release_amd.offset_regs']
LEAVES = ('mo', 'moo', 'sc', 'so', 'jo')
# B, V, J, pairs, channels of scale_offset: one row; one short of a workgroup, a whole one, one more; three batch elements;
# the loss block's shape; one partial more than the reduction has threads; more joints than one trip of the workgroup; none
SIZES = [(1, 1, 55, 24, 1), (1, 255, 55, 24, 3), (1, 256, 55, 24, 1), (1, 257, 1, 0, 1), (3, 1000, 300, 140, 3),
         (3, 1000, 300, 140, 1), (2, 3202, 55, 24, 1), (1, 65537, 55, 24, 1), (0, 7, 55, 24, 1), (2, 0, 55, 24, 3)]


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # (a copy: the cases are read-only)


def _n(t):
    return t.detach().cpu().numpy()


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = (got.view(np.int32) != want.view(np.int32)) & ~(np.isnan(got) & np.isnan(want))      # (a NaN's payload is free)
    assert not bad.any(), '%s: %d of %d elements differ, first at %s' % (what, bad.sum(), bad.size, np.argwhere(bad)[0])


def offset_view(a):
    """The array as a contiguous device view that starts 4 bytes into its storage (no 16-byte alignment)."""
    flat = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
    flat[1:] = _t(a).reshape(-1)
    return flat[1:].view(a.shape)


def build(c, grad=LEAVES, view=False):
    """(the module, the five inputs name -> device tensor) of an oracle case."""
    put = offset_view if view else _t
    m = exa.OffsetRegs(put(c['wm']), put(c['ws']).reshape(1, -1, 1), put(c['ref']), put(c['wj']),
                       (c['pr'].tolist(), c['pl'].tolist()))
    x = {k: put(c[k]).requires_grad_(k in grad) for k in LEAVES}
    return m, x


def run(m, x, reduce):
    return m(x['mo'], x['moo'], x['sc'], x['so'], x['jo'], reduce=reduce)


COEF = (np.float32(1.25), np.float32(0.75), np.float32(3.0), np.float32(0.5))


def mean_total(out, terms=range(4)):
    """sum_k COEF[k] mean_k: the cotangent of mean k is COEF[k], formed on the device."""
    return sum(out[oo.TERMS[k]] * float(COEF[k]) for k in terms)


def check_against_the_oracle(c, view=False):
    a = oo.args(c)
    want_maps = oo.maps(*a)
    # ---- map mode
    m, x = build(c, view=view)
    out = run(m, x, None)
    assert tuple(out) == oo.TERMS
    for name, w in zip(oo.TERMS, want_maps):
        same_bits(_n(out[name]), w, 'map ' + name)
    rs = np.random.RandomState(7)
    cot = [rs.standard_normal(w.shape).astype(np.float32) for w in want_maps]
    got = torch.autograd.grad([out[k] for k in oo.TERMS], [x[k] for k in LEAVES], [_t(g) for g in cot])
    want = oo.grads(*a, g_maps=cot)
    for k, g in zip(LEAVES, got):
        same_bits(_n(g), want[k], 'map mode dL/d' + k)
    # ---- mean mode
    m, x = build(c, view=view)
    out = run(m, x, 'mean')
    assert tuple(out) == oo.TERMS
    base = out[oo.TERMS[0]]._base
    assert base is not None and base.shape == (4,)
    assert all(out[k].dim() == 0 and out[k].data_ptr() == base.data_ptr() + 4 * i for i, k in enumerate(oo.TERMS))
    same_bits(_n(base), oo.means32(want_maps), 'means')
    got = torch.autograd.grad(mean_total(out), [x[k] for k in LEAVES])
    want = oo.grads(*a, g_means=COEF)
    for k, g in zip(LEAVES, got):
        same_bits(_n(g), want[k], 'mean mode dL/d' + k)


@pytest.mark.parametrize('B,V,J,P,ch', SIZES)
def test_maps_means_and_gradients_equal_the_oracle(B, V, J, P, ch):
    check_against_the_oracle(oo.make_case(100 + V, B, V, J, P, ch))


def test_views_at_a_four_byte_offset_give_the_same_bits():
    check_against_the_oracle(oo.make_case(41, 2, 777, 55, 24, 1), view=True)


def test_the_empty_terms():
    """No pairs: an empty map, a NaN mean and a joint gradient that is the other term's alone; no rows: the same for the
    vertex terms, as torch's expressions give."""
    c = oo.make_case(5, 1, 257, 1, 0)
    m, x = build(c)
    out = run(m, x, None)
    assert out['joint_offset_sym_reg'].shape == (0,)
    g, = torch.autograd.grad(out['joint_offset_sym_reg'].sum(), x['jo'])
    assert g.shape == (1, 3) and not bool(g.any())
    out = run(m, x, 'mean')
    assert bool(torch.isnan(out['joint_offset_sym_reg'])) and not bool(torch.isnan(out['joint_offset_reg']))
    g, = torch.autograd.grad(out['joint_offset_sym_reg'] + out['joint_offset_reg'], x['jo'])
    same_bits(_n(g), oo.grads(*oo.args(c), g_means=[None, None, 1.0, 1.0])['jo'], 'dL/djo without pairs')
    c = oo.make_case(6, 2, 0, 55, 24, 3)
    m, x = build(c)
    out = run(m, x, 'mean')
    assert bool(torch.isnan(out['gaussian_mean_reg'])) and bool(torch.isnan(out['gaussian_scale_reg']))
    assert run(m, x, None)['gaussian_scale_reg'].shape == (2, 0, 3)


# ---- against torch on the device --------------------------------------------------------------------------------------------
def torch_terms(m, x):
    """The reference's lines with constant weights and device index tensors (the `fused` form of tests/loss_case.py)."""
    wm, ws = m.mean_weight.reshape(1, -1, 1), m.scale_weight.reshape(1, -1, 1)
    r, l = x['jo'].index_select(0, m.pair_right.long()), x['jo'].index_select(0, m.pair_left.long())
    return {'gaussian_mean_reg': (x['mo'] ** 2 + x['moo'] ** 2) * wm, 'gaussian_scale_reg': (x['sc'] ** 2 + x['so'] ** 2) * ws,
            'joint_offset_reg': (x['jo'] - m.joint_offset_ref) ** 2 * m.joint_weight,
            'joint_offset_sym_reg': torch.abs(r[:, 0] + l[:, 0]) + torch.abs(r[:, 1] - l[:, 1]) + torch.abs(r[:, 2] - l[:, 2])}


@pytest.mark.parametrize('B,V,J,P,ch', [(3, 1000, 300, 140, 1), (3, 1000, 300, 140, 3), (2, 3202, 55, 24, 1)])
def test_map_mode_equals_the_torch_expressions_on_the_device(B, V, J, P, ch):
    c = oo.make_case(200 + ch, B, V, J, P, ch)
    m, x = build(c)
    got, want = run(m, x, None), torch_terms(m, x)
    rs = np.random.RandomState(8)
    cot = [_t(rs.standard_normal(tuple(want[k].shape)).astype(np.float32)) for k in oo.TERMS]
    for k in oo.TERMS:
        same_bits(_n(got[k]), _n(want[k]), 'map ' + k)
    leaves = [x[k] for k in LEAVES]
    g_got = torch.autograd.grad([got[k] for k in oo.TERMS], leaves, cot)
    g_want = torch.autograd.grad([want[k] for k in oo.TERMS], leaves, cot)
    for k, a, b in zip(LEAVES, g_got, g_want):
        if k == 'so' and ch == 1:
            gw = np.abs(_n(cot[1]).astype(np.float64) * c['ws'].astype(np.float64).reshape(1, -1, 1)).sum(2, keepdims=True)
            bound = 4 * U24 * gw * np.abs(2 * c['so'].astype(np.float64))
            err = np.abs(_n(a).astype(np.float64) - _n(b).astype(np.float64))
            print('dL/dso [B, V, 1]: worst error / bound %.3f' % float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), 'dL/dso: %g above the bound' % float((err - bound).max())
        else:
            same_bits(_n(a), _n(b), 'dL/d' + k)


def test_the_symmetric_reg_module_is_the_references():
    c = oo.make_case(9, 1, 1, lc.J, 24)
    reg = exa.JointOffsetSymmetricReg(lc.JOINTS_NAME).to(DEV)
    right, left = exa.symmetric_joint_pairs(lc.JOINTS_NAME)
    jo = _t(c['jo']).requires_grad_(True)
    got = reg(jo)
    want = torch.abs(jo[right, 0] + jo[left, 0]) + torch.abs(jo[right, 1] - jo[left, 1]) + torch.abs(jo[right, 2] - jo[left, 2])
    same_bits(_n(got), _n(want), 'JointOffsetSymmetricReg')
    cot = _t(np.random.RandomState(3).standard_normal(24).astype(np.float32))
    same_bits(_n(torch.autograd.grad(got, jo, cot)[0]), _n(torch.autograd.grad(want, jo, cot)[0]), 'its gradient')
    lazy = exa.JointOffsetSymmetricReg(lc.JOINTS_NAME)          # never moved: the tables follow the input
    same_bits(_n(lazy(jo)), _n(want), 'JointOffsetSymmetricReg, tables moved on first use')


# ---- against the reference's block ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def golden(golden_dir):
    return {w: np.load(os.path.join(golden_dir, 'ref_lossblock_w%d.npz' % w)) for w in (0, 1)}


def test_the_loss_blocks_terms_stay_within_the_fixtures_scales(golden):
    case, c = lc.build_case(), oo.block_case()
    masks = [_t(np.array(case[k])) for k in lc.MASKS]
    w = exa.loss_weights(*masks, joint_part=lc.JOINT_PART, joint_num=lc.J)
    same_bits(_n(w['gaussian_mean_reg']).reshape(-1), c['wm'], 'loss_weights on the device')
    m = exa.OffsetRegs(w['gaussian_mean_reg'], w['gaussian_scale_reg'], _t(c['ref']), w['joint_offset_reg'],
                       exa.symmetric_joint_pairs(lc.JOINTS_NAME))
    x = {k: _t(c[k]).requires_grad_(True) for k in LEAVES}
    out = run(m, x, 'mean')
    grad, = torch.autograd.grad(out['joint_offset_reg'] + out['joint_offset_sym_reg'], x['jo'])
    for warmup in (0, 1):          # the warm-up's scale_wo_clamp is the pre-clamp scale the other branch reads
        g = golden[warmup]
        for name in oo.TERMS:
            ratio = abs(float(out[name].detach().double()) - lc.term_value(g, name)) / lc.term_scale(g, 'fused', name)
            print('w%d %-22s %.3f scales' % (warmup, name, ratio))
            assert ratio <= lc.FACTOR, (warmup, name, ratio)
        r = block.ratio(g, 'joint_offset', grad)
        print('w%d grad/joint_offset ratio %.3f' % (warmup, r))
        assert r <= block.FACTOR, (warmup, r)


# ---- other behaviour ------------------------------------------------------------------------------------------------------
def test_every_subset_of_requires_grad():
    c = oo.make_case(11, 2, 300, 55, 24)
    want = oo.grads(*oo.args(c), g_means=COEF)
    for mask in range(32):
        grad = [k for i, k in enumerate(LEAVES) if mask >> i & 1]
        m, x = build(c, grad=grad)
        out = run(m, x, 'mean')
        total = mean_total(out)
        assert total.requires_grad == bool(grad)
        if grad:
            for k, g in zip(grad, torch.autograd.grad(total, [x[k] for k in grad])):
                same_bits(_n(g), want[k], 'dL/d%s alone with %s' % (k, grad))
    cot = [np.random.RandomState(2).standard_normal(w.shape).astype(np.float32) for w in oo.maps(*oo.args(c))]
    want = oo.grads(*oo.args(c), g_maps=cot)
    for grad in (['so'], ['mo', 'jo'], ['moo', 'sc']):
        m, x = build(c, grad=grad)
        out = run(m, x, None)
        got = torch.autograd.grad([out[k] for k in oo.TERMS], [x[k] for k in grad], [_t(g) for g in cot])
        for k, g in zip(grad, got):
            same_bits(_n(g), want[k], 'map mode dL/d%s alone with %s' % (k, grad))


@pytest.mark.parametrize('reduce', [None, 'mean'])
def test_one_output_alone(reduce):
    c = oo.make_case(12, 2, 300, 55, 24, 3)
    for k, name in enumerate(oo.TERMS):
        m, x = build(c)
        y = run(m, x, reduce)[name]
        got = torch.autograd.grad(y.sum(), [x[n] for n in LEAVES], allow_unused=True)
        one = [np.float32(1) if j == k else None for j in range(4)]
        if reduce == 'mean':
            want = oo.grads(*oo.args(c), g_means=one)
        else:
            want = oo.grads(*oo.args(c), g_maps=[None if o is None else np.ones(w.shape, np.float32)
                                                 for o, w in zip(one, oo.maps(*oo.args(c)))])
        for n, g in zip(LEAVES, got):
            if want[n] is None:
                assert g is None, '%s alone reaches %s' % (name, n)
            else:
                same_bits(_n(g), want[n], '%s alone: dL/d%s' % (name, n))


def test_the_same_bits_twice_and_the_functional_form():
    c = oo.make_case(13, 3, 1000, 300, 140)
    m, x = build(c)
    runs = []
    for _ in range(2):
        out = run(m, x, 'mean')
        runs.append([_n(out[oo.TERMS[0]]._base)] + [_n(g) for g in torch.autograd.grad(mean_total(out), [x[k] for k in LEAVES])])
    for a, b in zip(*runs):
        same_bits(a, b, 'second call')
    out = exa.offset_regs(x['mo'], x['moo'], x['sc'], x['so'], x['jo'], _t(c['wm']), _t(c['ws']).reshape(-1, 1), _t(c['ref']),
                          _t(c['wj']), (c['pr'].tolist(), c['pl'].tolist()))
    same_bits(_n(out[oo.TERMS[0]]._base), runs[0][0], 'offset_regs()')
    with pytest.raises(ValueError, match='offset_regs: scale is not on the device of joint_offset'):
        run(m, dict(x, sc=x['sc'].detach().cpu()), 'mean')
    with pytest.raises(ValueError, match='offset_regs: mean_weight is not on the device of joint_offset'):
        exa.OffsetRegs(_t(c['wm']).cpu(), _t(c['ws']).cpu(), _t(c['ref']).cpu(), _t(c['wj']).cpu(), None)(
            x['mo'], x['moo'], x['sc'], x['so'], x['jo'])


@pytest.mark.parametrize('reduce', [None, 'mean'])
def test_two_launches_forward_and_one_backward(monkeypatch, reduce):
    calls = []
    real = module.launch

    def counting(abi, name, *args):
        calls.append(name)
        return real(abi, name, *args)
    monkeypatch.setattr(module, 'launch', counting)
    c = oo.make_case(14, 2, 3202, 55, 24)
    m, x = build(c)
    out = run(m, x, reduce)
    assert calls == ['exa_mesh_offset_regs_vertex_forward', 'exa_mesh_offset_regs_joint_forward']
    del calls[:]
    torch.autograd.grad(sum(out[k].sum() for k in oo.TERMS), [x[k] for k in LEAVES])
    assert calls == ['exa_mesh_offset_regs_backward']


def test_one_captured_graph_replays_the_eager_bits():
    c = oo.make_case(15, 2, 3202, 55, 24)
    m, x = build(c)
    leaves = [x[k] for k in LEAVES]

    def step():
        out = run(m, x, 'mean')
        return (out[oo.TERMS[0]]._base,) + torch.autograd.grad(mean_total(out), leaves)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    with torch.no_grad():
        x['mo'].mul_(-1.5)
        x['so'].add_(0.25)
        x['sc'].mul_(2.0)
        x['jo'].copy_(x['jo'].flip(0))
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    for name, got, want in zip(('means',) + LEAVES, outs, eager):
        same_bits(_n(got), _n(want), 'replayed ' + name)
    changed = dict(c, **{k: _n(x[k]) for k in LEAVES})
    same_bits(_n(outs[0]), oo.means32(oo.maps(*oo.args(changed))), 'replayed means against the oracle')
