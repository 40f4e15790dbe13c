"""GPU tests of the fused MLP (csrc/mlp.hip behind include/exa_mlp.h) over the whole contract its C ABI accepts, where
tests/test_gpu_mlp.py runs the four reference nets: 1 and 4 trunk layers, 1, 2 and 4 groups, 3 and 4 heads up to the full
32 columns, per-row widths at the edges of the 8-column k step and the 128-column LDS slab, 1 and 1024 shared columns,
row counts at the edges of the wave, the workgroup and the backward's chunk (tests/mlp_cases.py: ``CASES``, ``SWEEP_N``;
DESIGN.md section 8f names the kernel branch each one pins), degenerate rows, non-finite rows, and the C ABI called
directly for what autograd never passes: NULL cotangents, NULL gradient outputs and a padded ``ld_w0``.

Everything is held to tests/mlp_oracle.py bit for bit; tests/test_mlp_oracle.py holds the oracle to PyTorch's float64
expression on the same cases."""
import ctypes

import numpy as np
import pytest
import torch

import mlp_cases as mc
import mlp_oracle as mo
from mlp_cases import bits_equal

pytestmark = pytest.mark.gpu

TWO_LAYERS = dict(L=2, K0=24, S=0, G=4, heads=(3, 1), N=200)


def fused(cs):
    import exavatar_release_amd as exa
    tr, heads = cs.modules('cuda')
    return exa.FusedMLP(tr, heads=heads)


def check_case(cs, **kw):
    mc.check_against_oracle(fused(cs), cs.blocks('cuda'), cs.G.cuda(), ref=cs.oracle(), **kw)


@pytest.mark.parametrize('name', sorted(mc.CASES))
def test_bit_exact_over_the_contract(name):
    check_case(mc.case(name))


@pytest.mark.parametrize('N', mc.SWEEP_N)
def test_bit_exact_row_count_sweep(N):
    check_case(mc.case(mc.sweep(N)))


@pytest.mark.parametrize('what', ['params_only', 'x_only'])
@pytest.mark.parametrize('name', ['four_heads_full', 'slab_plus_one'])
def test_bit_exact_partial_gradients_wide(name, what):
    check_case(mc.case(name), need_x=what == 'x_only', need_params=what == 'params_only')


# ---- degenerate rows

def _saved(cs):
    """The oracle's per-layer xhat, rstd and y of ``cs`` (fp32)."""
    return mo.forward(cs.oracle_net(), cs.x.numpy(), keep=True)[1]


def test_zero_variance_group():
    """Group 1 of the second layer sees a constant: its rows of W_1 are zero and its bias is 0.5, so every z is 0.5, the
    mean is 0.5, var = 0, rstd = 1 / sqrt(eps), xhat = +0 and y = beta."""
    cs = mc.Case(TWO_LAYERS, seed=11)
    with torch.no_grad():
        cs.trunk[3].weight[32:64].zero_()
        cs.trunk[3].bias[32:64].fill_(0.5)
    s = _saved(cs)[1]
    assert (s['rstd'][:, 1] == np.float32(1) / np.sqrt(np.float32(cs.trunk[4].eps))).all()
    assert not s['xhat'][:, 32:64].any() and s['xhat'][:, :32].any()
    _, g = cs.oracle()
    assert g['layers'][1]['W'][32:64].any(), 'the constant group still gets a weight gradient (dZ = rstd (e - m1))'
    check_case(cs)


def test_fully_dead_layer():
    """The last layer's beta is -20 (|xhat gamma| <= 1.5 sqrt(31)): every pre-ReLU value is negative, the activation is
    +0, dY = +0, m1 = m2 = +0 and every gradient upstream of the heads' biases is zero."""
    cs = mc.Case(TWO_LAYERS, seed=12)
    with torch.no_grad():
        cs.trunk[4].bias.fill_(-20.0)
    assert (_saved(cs)[1]['y'] < 0).all()
    _, g = cs.oracle()
    for gl in g['layers']:
        assert not any(gl[k].any() for k in ('W', 'b', 'gamma', 'beta'))
    assert not g['x'].any() and not g['Wh'].any() and g['bh'].all()
    check_case(cs)


def test_zero_cotangent_rows_between_live_rows():
    cs = mc.Case(TWO_LAYERS, seed=13)
    G = cs.G.clone()
    G[1::3] = 0.0
    _, g = mc.check_against_oracle(fused(cs), cs.blocks('cuda'), G.cuda())
    assert not g['x'][1::3].any() and g['x'][0::3].all()


@pytest.mark.parametrize('rows', [(5, 37), (5, 21)])
def test_non_finite_rows_stay_in_their_rows(rows):
    """A NaN in one row and a +Inf in another, forward only.  A row is one accumulator column: lanes r and r + 32 of its
    wave hold its channels, and lane half h loads the input columns k with (k >> 2) & 1 == h.  The NaN sits in column 2
    (half 0: lane 5 of wave 0) and the Inf in column 5 (half 1), so both lane halves carry a non-finite operand: with
    rows (5, 21) in one wave (lanes 5 and 53), with rows (5, 37) at the same column of two neighbouring waves (lane 5 of
    wave 0, lane 37 of wave 1).  Every other row must keep the bits it has with the two rows zeroed, and must equal the
    oracle; the two rows are NaN in every head column (every z takes a NaN or Inf term, the group mean is NaN, relu
    passes NaN)."""
    cs = mc.case(dict(TWO_LAYERS, N=130), seed=14)
    fm = fused(cs)
    a, b = rows
    x = cs.x.clone()
    x[a, 2] = float('nan')
    x[b, 5] = float('inf')
    x0 = x.clone()
    x0[[a, b]] = 0.0
    with torch.no_grad():
        bad = torch.cat(fm(x.cuda()), 1).cpu().numpy()
        clean = torch.cat(fm(x0.cuda()), 1).cpu().numpy()
    others = np.ones(cs.N, bool)
    others[[a, b]] = False
    assert np.isfinite(clean).all()
    assert bits_equal(bad[others], clean[others])
    assert np.isnan(bad[[a, b]]).all()
    assert bits_equal(clean, mo.forward(cs.oracle_net(), x0.numpy()))
    assert np.isnan(mo.forward(cs.oracle_net(), x.numpy())[[a, b]]).all()


# ---- the C ABI, called directly

SENTINEL = -777.25          # what an output nobody asked for, and the guard bands around every output, must still hold
GUARD = 64


class AbiNet:
    """The exa_mlp_net of a Case on the GPU, and exa_mlp_forward / exa_mlp_backward through ctypes: raw pointers, a
    caller-owned workspace sized by exa_mlp_workspace_size, the current stream.  ``ld_pad`` extra columns per row of
    W_0, filled with NaN."""

    def __init__(self, cs, ld_pad=0):
        from exavatar_release_amd import _lib
        from exavatar_release_amd.mlp import parse_structure
        self.lib, self.abi, self.cs = _lib.load(), _lib.MLP, cs
        dev = torch.device('cuda:0')
        layers, hs = parse_structure(cs.trunk, cs.heads)
        K0, S = len(cs.per_row), len(cs.shared)
        W = layers[0][0].weight.detach()
        W0 = torch.full((mc.HIDDEN, K0 + ld_pad), float('nan'))
        W0[:, :K0] = W[:, cs.per_row]
        t = {'W0': W0, 'Wh': torch.cat([h.weight.detach() for h in hs]), 'bh': torch.cat([h.bias.detach() for h in hs])}
        if S:
            t['Ws'], t['p'] = W[:, cs.shared], cs.p
        for l, (lin, gn) in enumerate(layers):
            if l > 0:
                t['W%d' % l] = lin.weight.detach()
            t['b%d' % l], t['gamma%d' % l], t['beta%d' % l] = lin.bias.detach(), gn.weight.detach(), gn.bias.detach()
        self.t = t = {k: v.clone().contiguous().to(dev) for k, v in t.items()}
        n = self.net = _lib.ExaMlpNet()
        n.n_layers, n.in_width, n.shared_width, n.groups = len(layers), K0, S, layers[0][1].num_groups
        n.n_heads = len(hs)
        for k, h in enumerate(hs):
            n.head_width[k] = h.out_features
        n.ld_w0, n.ld_ws = K0 + ld_pad, S
        for l, (lin, gn) in enumerate(layers):
            n.eps[l] = gn.eps
            n.W[l] = t['W%d' % l].data_ptr()
            n.b[l], n.gamma[l], n.beta[l] = (t['%s%d' % (k, l)].data_ptr() for k in ('b', 'gamma', 'beta'))
        if S:
            n.Ws, n.shared = t['Ws'].data_ptr(), t['p'].data_ptr()
        n.Wh, n.bh = t['Wh'].data_ptr(), t['bh'].data_ptr()
        self.widths = [h.out_features for h in hs]
        self.K0, self.S, self.N, self.dev = K0, S, cs.N, dev
        self.x = cs.x.contiguous().to(dev)
        count = ctypes.c_int64()
        self.abi.check(self.lib.exa_mlp_param_count(ctypes.byref(n), ctypes.byref(count)))
        self.count = int(count.value)
        self.ws_bytes = _lib.size_query(self.abi, 'exa_mlp_workspace_size', ctypes.byref(n), self.N)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def forward(self):
        outs = [torch.full((self.N, w), float('nan'), device=self.dev) for w in self.widths]
        ptrs = (ctypes.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        self.abi.check(self.lib.exa_mlp_forward(ctypes.byref(self.net), self.N, self.x.data_ptr(), ptrs, self._stream()))
        torch.cuda.synchronize()
        return torch.cat(outs, 1).cpu().numpy()

    def backward(self, gouts, want=('x', 'params', 'ws'), poison=False):
        """exa_mlp_backward with the cotangents ``gouts`` (device tensors, None = NULL) and NULL for every output not in
        ``want``.  The outputs are sections of one arena pre-filled with SENTINEL, GUARD floats apart: the call must
        leave every float outside the sections it was given untouched.  Returns {name: numpy array}."""
        sizes = {'x': self.N * self.K0, 'params': self.count, 'ws': mc.HIDDEN * self.S}
        off, o = {}, GUARD
        for k in ('x', 'params', 'ws'):
            off[k] = o
            o += sizes[k] + GUARD
        arena = torch.full((o,), SENTINEL, device=self.dev)
        ws = torch.empty(max(self.ws_bytes, 1), dtype=torch.uint8, device=self.dev).fill_(255 if poison else 0)
        gptrs = (ctypes.c_void_p * len(gouts))(*[g.data_ptr() if g is not None else None for g in gouts])
        ptr = {k: arena.data_ptr() + 4 * off[k] if (k in want and sizes[k]) else None for k in sizes}
        self.abi.check(self.lib.exa_mlp_backward(ctypes.byref(self.net), self.N, self.x.data_ptr(), gptrs, ptr['x'],
                                                 ptr['params'], ptr['ws'], ws.data_ptr(), self.ws_bytes, self._stream()))
        torch.cuda.synchronize()
        a = arena.cpu().numpy()
        written = np.zeros(o, bool)
        res = {}
        for k in sizes:
            if ptr[k] is not None:
                written[off[k]:off[k] + sizes[k]] = True
                res[k] = a[off[k]:off[k] + sizes[k]].copy()
        assert (a[~written] == np.float32(SENTINEL)).all(), 'the call wrote outside the outputs it was given'
        for k, v in res.items():
            assert not (v == np.float32(SENTINEL)).any(), 'grad_%s is not fully written' % k
        return res

    def cotangents(self, G=None):
        G = self.cs.G if G is None else G
        outs, o = [], 0
        for w in self.widths:
            outs.append(G[:, o:o + w].contiguous().to(self.dev))
            o += w
        return outs


def _flat_params(g):
    """The oracle's parameter gradients in the flat layout of exa_mlp_param_count."""
    parts = []
    for gl in g['layers']:
        parts += [gl['W'].ravel(), gl['b'], gl['gamma'], gl['beta']]
    return np.concatenate(parts + [g['Wh'].ravel(), g['bh']])


ABI_SPEC = dict(L=2, K0=20, S=0, G=4, heads=(5, 2, 1), N=300)


@pytest.fixture(scope='module')
def abi():
    """The three-head net, its AbiNet and the call that asks for everything."""
    cs = mc.case(ABI_SPEC, seed=21)
    net = AbiNet(cs)
    return cs, net, net.forward(), net.backward(net.cotangents(), want=('x', 'params'))


@pytest.fixture(scope='module')
def abi_shared():
    cs = mc.case(dict(ABI_SPEC, S=6), seed=22)
    net = AbiNet(cs)
    return cs, net, net.backward(net.cotangents())


def test_abi_full_call_equals_oracle(abi):
    cs, net, out, full = abi
    ref_out, g = cs.oracle()
    assert net.count == 128 * 20 + 3 * 128 + 128 * 128 + 3 * 128 + 8 * 128 + 8
    assert bits_equal(out, ref_out)
    assert bits_equal(full['x'].reshape(cs.N, -1), g['x'])
    assert bits_equal(full['params'], _flat_params(g))


def test_abi_shared_columns_equal_oracle(abi_shared):
    """Straight from the C ABI no autograd addition stands between the kernel and the comparison: the signs of zeros of
    W_0's and Ws' gradients are compared as they are."""
    cs, net, full = abi_shared
    _, g = cs.oracle()
    assert bits_equal(full['x'].reshape(cs.N, -1), g['x'])
    assert bits_equal(full['params'], _flat_params(g))
    assert bits_equal(full['ws'].reshape(mc.HIDDEN, -1), g['Ws'])


def test_abi_null_cotangent_is_a_zero_cotangent(abi):
    cs, net, _, _ = abi
    gouts = net.cotangents()
    null = net.backward([gouts[0], None, gouts[2]], want=('x', 'params'))
    zero = net.backward([gouts[0], torch.zeros_like(gouts[1]), gouts[2]], want=('x', 'params'))
    assert bits_equal(null['x'], zero['x']) and bits_equal(null['params'], zero['params'])
    G = cs.G.clone()
    G[:, 5:7] = 0.0
    g = mo.backward(cs.oracle_net(), cs.x.numpy(), G.numpy())
    assert bits_equal(null['x'].reshape(cs.N, -1), g['x']) and bits_equal(null['params'], _flat_params(g))


@pytest.mark.parametrize('want', ['x', 'params'])
def test_abi_null_outputs(abi, want):
    """grad_params = NULL or grad_x = NULL: the output asked for has the bits of the call that asks for both, and nothing
    is written where the other one would be (AbiNet.backward checks the arena)."""
    cs, net, _, full = abi
    got = net.backward(net.cotangents(), want=(want,))
    assert list(got) == [want] and bits_equal(got[want], full[want])


def test_abi_shared_gradient_alone(abi_shared):
    cs, net, full = abi_shared
    got = net.backward(net.cotangents(), want=('ws',))
    assert list(got) == ['ws'] and bits_equal(got['ws'], full['ws'])


def test_abi_padded_w0_rows(abi):
    """ld_w0 = K0 + 5 with NaN in the five padding columns of every row of W_0: the stagings of W_0 and of its transpose
    read columns below in_width only, so forward and backward have the bits of the contiguous call."""
    cs, net, out, full = abi
    padded = AbiNet(cs, ld_pad=5)
    assert padded.net.ld_w0 == 25 and bool(torch.isnan(padded.t['W0'][:, 20:]).all())
    assert bits_equal(padded.forward(), out)
    got = padded.backward(padded.cotangents(), want=('x', 'params'))
    assert bits_equal(got['x'], full['x']) and bits_equal(got['params'], full['params'])


def test_abi_poisoned_workspace(abi, abi_shared):
    """The backward reads no byte of its workspace that it has not written: 0xFF instead of zeros changes nothing."""
    cs, net, _, full = abi
    got = net.backward(net.cotangents(), want=('x', 'params'), poison=True)
    assert bits_equal(got['x'], full['x']) and bits_equal(got['params'], full['params'])
    cs, net, full = abi_shared
    got = net.backward(net.cotangents(), poison=True)
    assert all(bits_equal(got[k], full[k]) for k in ('x', 'params', 'ws'))
