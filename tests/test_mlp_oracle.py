"""CPU tests of the fused MLP's numpy restatement (tests/mlp_oracle.py) and of FusedMLP's structure checks.

* ``fma32`` is the correctly rounded fmaf: it equals libm's ``fmaf`` (through ctypes) on random inputs, on ties and
  near-ties, and on signed-zero, subnormal and overflow cases.
* Run in float64, the oracle equals PyTorch's float64 nn.Sequential + autograd to 1e-12 -- outputs, the per-row input
  gradient and every parameter gradient, with a shared (folded) block and with a trailing Linear -- and equals the
  reference's own make_linear_layers, executed (tests/golden/ref_mlp.npz, made by tests/golden/make_golden_mlp.py:
  geo_offset_net and rgb_offset_net, the two with a shared block, one with heads and one with a trailing Linear).
* Over the whole contract of include/exa_mlp.h (every entry of ``mlp_cases.CASES``: 1 and 4 layers, 1, 2 and 4 groups,
  1-4 heads up to 32 wide, 1-256 per-row and 0-1024 shared columns) the float64 oracle equals PyTorch's float64
  expression to the same 1e-12, and the fp32 oracle lies within the bound tests/test_gpu_mlp.py holds FusedMLP to.  With
  the GPU tests, which hold the kernels to the fp32 oracle bit for bit, that gives the kernels a float64 reference there.
* ``parse_structure`` accepts the four reference nets and refuses the unsupported ones, naming the layer."""
import ctypes
import ctypes.util
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import mlp_cases as mc
import mlp_oracle as mo
from exavatar_release_amd.mlp import parse_structure

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_mlp.npz')


def _libm_fmaf():
    name = ctypes.util.find_library('m') or 'libm.so.6'
    libm = ctypes.CDLL(name)
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    return libm.fmaf


def _check_fma(a, b, c):
    fmaf = _libm_fmaf()
    a, b, c = (np.asarray(v, np.float32).ravel() for v in (a, b, c))
    got = mo.fma32(a, b, c)
    want = np.array([fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    same = (got.view(np.int32) == want.view(np.int32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), list(zip(a[~same][:5], b[~same][:5], c[~same][:5]))


def test_fma32_random():
    rng = np.random.default_rng(0)
    a = rng.standard_normal(4000).astype(np.float32) * np.float32(2.0) ** rng.integers(-20, 20, 4000)
    b = rng.standard_normal(4000).astype(np.float32) * np.float32(2.0) ** rng.integers(-20, 20, 4000)
    c = rng.standard_normal(4000).astype(np.float32) * np.float32(2.0) ** rng.integers(-40, 40, 4000)
    _check_fma(a, b, c)


def test_fma32_ties_and_near_ties():
    one = np.float32(1)
    u = np.float32(2.0 ** -24)
    a, b, c = [], [], []
    for k in range(1, 40):
        # (1 + k 2^-23)(1 + small) + c puts the exact result on or next to a rounding boundary
        x = one + np.float32(k) * np.float32(2.0 ** -23)
        for y in (one + np.float32(2.0 ** -23), one - u, one + np.float32(3 * 2.0 ** -23)):
            for z in (np.float32(0), -one, one, np.float32(2.0 ** -25), -np.float32(2.0 ** -25), np.float32(1.5)):
                a.append(x)
                b.append(y)
                c.append(z)
    # exact halfway cases: 1 + 2^-24 (ties to even, down) and 1 + 3 * 2^-24 (up)
    a += [one, one, one + np.float32(2.0 ** -23)]
    b += [one, one, one]
    c += [np.float32(2.0 ** -24), np.float32(3 * 2.0 ** -24), np.float32(2.0 ** -24)]
    _check_fma(a, b, c)


def test_fma32_zeros_subnormals_overflow():
    tiny = np.float32(1.4e-45)
    big = np.float32(3.0e38)
    vals = [np.float32(0), -np.float32(0), tiny, -tiny, np.float32(1e-38), np.float32(1e-20), np.float32(1),
            -np.float32(1), big, -big, np.float32(np.inf), -np.float32(np.inf), np.float32(np.nan)]
    a, b, c = np.meshgrid(vals, vals, vals, indexing='ij')
    _check_fma(a, b, c)


def _trunk(widths, trailing=0, groups=4):
    mods = []
    for a, b in zip(widths[:-1], widths[1:]):
        mods += [nn.Linear(a, b), nn.GroupNorm(groups, b), nn.ReLU(inplace=True)]
    if trailing:
        mods.append(nn.Linear(widths[-1], trailing))
    return nn.Sequential(*mods)


def _affine(seq):
    for m in seq:
        if isinstance(m, nn.GroupNorm):
            with torch.no_grad():
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)


def _close(a, b, what, tol=1e-12):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()), what


@pytest.mark.parametrize('case', ['geo', 'rgb_offset'])
def test_oracle_float64_equals_torch(case):
    torch.manual_seed(7)
    N = 1100                      # more than two chunks, the last one ragged
    if case == 'geo':
        net = _trunk([96, 128, 128, 128])
        heads = [nn.Linear(128, 3), nn.Linear(128, 1)]
        per_row, shared = list(range(96)), []
    else:
        net = _trunk([225, 128, 128, 128], trailing=3)
        heads = []
        per_row, shared = list(range(96)) + [222, 223, 224], list(range(96, 222))
    _affine(net)
    net.double()
    for h in heads:
        h.double()
    layers, hs = parse_structure(net, heads or None)
    x = torch.randn(N, len(per_row), dtype=torch.float64)
    p = torch.randn(126, dtype=torch.float64)
    inp = torch.cat([x[:, :96], p[None].expand(N, 126), x[:, 96:]], 1) if shared else x
    inp = inp.clone().requires_grad_(True)
    h = net(inp)
    out = torch.cat([hd(h) for hd in heads], 1) if heads else h
    G = torch.randn_like(out)
    out.backward(G)
    onet = mo.net_from_modules(layers, hs, per_row, shared, p.numpy() if shared else None, np.float64)
    o = mo.forward(onet, x.numpy(), np.float64)
    g = mo.backward(onet, x.numpy(), G.numpy(), np.float64)
    _close(o, out.detach().numpy(), 'outputs')
    _close(g['x'], inp.grad.numpy()[:, per_row], 'input gradient')
    for l, (lin, gn) in enumerate(layers):
        W = lin.weight.grad.numpy()
        _close(g['layers'][l]['W'], W[:, per_row] if l == 0 else W, 'W_%d' % l)
        _close(g['layers'][l]['b'], lin.bias.grad.numpy(), 'b_%d' % l)
        _close(g['layers'][l]['gamma'], gn.weight.grad.numpy(), 'gamma_%d' % l)
        _close(g['layers'][l]['beta'], gn.bias.grad.numpy(), 'beta_%d' % l)
    if shared:
        _close(g['Ws'], layers[0][0].weight.grad.numpy()[:, shared], 'shared columns')
    _close(g['Wh'], np.concatenate([hd.weight.grad.numpy() for hd in hs]), 'head weights')
    _close(g['bh'], np.concatenate([hd.bias.grad.numpy() for hd in hs]), 'head biases')


@pytest.mark.parametrize('name', sorted(mc.CASES))
def test_oracle_float64_equals_torch_over_the_contract(name):
    """Every entry of mlp_cases.CASES: outputs, the per-row input gradient and every parameter gradient (layer 0's weight
    over its per-row and its shared columns, the heads stacked) against PyTorch's float64 nn.Sequential + autograd."""
    cs = mc.case(name)
    want = mc.torch_expression(cs.trunk, cs.heads, cs.full_input(torch.float64), cs.G, torch.float64)
    got = mc.oracle_as_expression(cs, np.float64)
    got, want = mc.flat(got), mc.flat(want, cs.per_row)
    assert [k for k, _ in got] == [k for k, _ in want] and len(got) == 4 + 4 * cs.spec['L']
    for (what, a), (_, b) in zip(got, want):
        _close(a, b, '%s %s' % (name, what))


@pytest.mark.parametrize('name', sorted(mc.CASES))
def test_oracle_fp32_within_the_fp32_expression_bound(name):
    """Every entry of mlp_cases.CASES: the fp32 oracle against the float64 expression, under the bound of
    tests/test_gpu_mlp.py's ``_bound_check``, per result tensor, with e64 the float64 value and the fp32 expression run
    on the CPU:
        max |oracle_fp32 - e64| <= 16 * max |torch_fp32 - e64| + 64 * 2^-24 * rms(e64)"""
    cs = mc.case(name)
    e64 = mc.flat(mc.torch_expression(cs.trunk, cs.heads, cs.full_input(torch.float64), cs.G, torch.float64), cs.per_row)
    t32 = mc.flat(mc.torch_expression(cs.trunk, cs.heads, cs.full_input(), cs.G, torch.float32), cs.per_row)
    o32 = mc.flat(mc.oracle_as_expression(cs, np.float32))
    for (what, a64), (_, a32), (_, ao) in zip(e64, t32, o32):
        assert a64.shape == a32.shape == ao.shape, what
        a64 = a64.astype(np.float64)
        err_t = float(np.abs(a32.astype(np.float64) - a64).max())
        err_o = float(np.abs(ao.astype(np.float64) - a64).max())
        bound = 16 * err_t + 64 * 2.0 ** -24 * float(np.sqrt(np.mean(a64 ** 2)))
        print('%s %s: oracle error %.3g, fp32 expression error %.3g, bound %.3g' % (name, what, err_o, err_t, bound))
        assert err_o <= bound, '%s %s: oracle error %g > bound %g (fp32 expression error %g)' % (name, what, err_o,
                                                                                             bound, err_t)


def test_oracle_float64_equals_reference_golden():
    """Every case of tests/golden/ref_mlp.npz: what the reference's own make_linear_layers computed in float64."""
    z = np.load(GOLDEN)
    cases = sorted({k.split('/')[0] for k in z.files})
    assert cases == ['geo_offset', 'rgb_offset']
    for case in cases:
        f = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(case + '/')}
        L = int(f['n_layers'])
        per_row = [int(c) for c in f['per_row_cols']]
        shared = [int(c) for c in f['shared_cols']]
        net = {'layers': []}
        for l in range(L):
            W = f['W%d' % l].astype(np.float64)
            net['layers'].append({'W': W[:, per_row] if l == 0 else W, 'b': f['b%d' % l], 'gamma': f['gamma%d' % l],
                                  'beta': f['beta%d' % l], 'G': int(f['groups']), 'eps': float(f['eps'])})
        if shared:
            net['Ws'] = f['W0'].astype(np.float64)[:, shared]
            net['p'] = f['p']
        net['Wh'], net['bh'] = f['Wh'], f['bh']
        o = mo.forward(net, f['x'], np.float64)
        g = mo.backward(net, f['x'], f['gout'], np.float64)
        _close(o, f['out'], case + ' outputs')
        _close(g['x'], f['grad_x'][:, per_row], case + ' input gradient')
        for l in range(L):
            # layer 0's oracle gradient comes as the per-row and the shared columns: put both back into the full layout
            mine = g['layers'][l]['W']
            if l == 0:
                full = np.zeros(f['W0'].shape)
                full[:, per_row] = mine
                full[:, shared] = g['Ws']
                mine = full
            _close(mine.ravel()[f['grad_W%d_idx' % l]], f['grad_W%d_val' % l], '%s W_%d' % (case, l))
            for k in ('b', 'gamma', 'beta'):
                _close(g['layers'][l][k], f['grad_%s%d' % (k, l)], '%s %s_%d' % (case, k, l))
        _close(g['Wh'], f['grad_Wh'], case + ' head weights')
        _close(g['bh'], f['grad_bh'], case + ' head biases')


def test_structure_accepts_the_reference_nets():
    geo = _trunk([96, 128, 128, 128])
    layers, hs = parse_structure(geo, heads=(nn.Sequential(nn.Linear(128, 3)), nn.Sequential(nn.Linear(128, 1))))
    assert len(layers) == 3 and [h.out_features for h in hs] == [3, 1]
    layers, hs = parse_structure(_trunk([222, 128, 128, 128]), heads=(nn.Linear(128, 3), nn.Linear(128, 1)))
    assert len(layers) == 3 and layers[0][0].in_features == 222
    layers, hs = parse_structure(_trunk([96, 128, 128, 128], trailing=3))
    assert len(layers) == 3 and [h.out_features for h in hs] == [3]
    layers, hs = parse_structure(_trunk([225, 128, 128, 128], trailing=3))
    assert layers[0][0].in_features == 225 and hs[0].out_features == 3


@pytest.mark.parametrize('build, heads, match', [
    (lambda: _trunk([96, 64, 64]), None, 'layer 0 .*64 wide'),
    (lambda: _trunk([96, 128], groups=8), (nn.Linear(128, 3),), 'layer 1 \\(GroupNorm\\)'),
    (lambda: nn.Sequential(nn.Linear(96, 128), nn.GroupNorm(4, 128), nn.ReLU(), nn.Linear(128, 128),
                           nn.GroupNorm(1, 128), nn.ReLU(), nn.Linear(128, 3)), None, 'layer 4 \\(GroupNorm\\) has 1 groups'),
    (lambda: nn.Sequential(nn.Linear(96, 128), nn.GroupNorm(4, 128), nn.Tanh()), (nn.Linear(128, 3),), 'layer 2'),
    (lambda: nn.Sequential(nn.Linear(96, 128), nn.ReLU()), (nn.Linear(128, 3),), 'layer 0'),
    (lambda: _trunk([96, 128, 128, 128, 128, 128]), (nn.Linear(128, 3),), 'at most 4'),
    (lambda: _trunk([96, 128]), None, '1 .. 4 heads'),
    (lambda: _trunk([96, 128]), (nn.Linear(128, 30), nn.Linear(128, 3)), 'at most 32'),
    (lambda: _trunk([96, 128]), (nn.Sequential(nn.Linear(128, 8), nn.ReLU()),), 'head 0'),
    (lambda: _trunk([96, 128], trailing=3), (nn.Linear(128, 3),), 'heads= is given as well'),
    (lambda: nn.Sequential(nn.Linear(96, 128, bias=False), nn.GroupNorm(4, 128), nn.ReLU()), (nn.Linear(128, 3),),
     'layer 0 \\(Linear\\) has no bias'),
])
def test_structure_refuses_unsupported(build, heads, match):
    with pytest.raises(ValueError, match=match):
        parse_structure(build(), heads)


def test_cpu_tensors_are_refused():
    import exavatar_release_amd as exa
    fm = exa.FusedMLP(_trunk([8, 128], trailing=3))
    with pytest.raises(RuntimeError, match='ROCm device only'):
        fm(torch.randn(4, 8))
