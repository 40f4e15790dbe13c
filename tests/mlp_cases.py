"""Case builder of the fused MLP's tests: one table of nets over the contract of include/exa_mlp.h, built the same way
for the CPU tests (tests/test_mlp_oracle.py: the numpy oracle against PyTorch) and the GPU tests
(tests/test_gpu_mlp_contract.py, tests/test_gpu_mlp.py: FusedMLP against the oracle, bit for bit).

``CASES`` names the nets (DESIGN.md section 8f lists the kernel branch each one pins); ``sweep(N)`` is the cheap net of the
row-count sweep ``SWEEP_N``.  ``case(spec)`` builds, from a seed, the nn.Sequential trunk with non-trivial GroupNorm
affines, the head Linears, the column layout, the per-row input ``x``, the shared row ``p`` and the cotangent ``G``, all on
the CPU in float32.  With a shared block, the block sits in the middle of the first layer's columns: the per-row columns
are then two blocks, and FusedMLP gathers their weight columns with a concatenation.

``check_against_oracle`` is the GPU comparison both GPU test files use."""
import copy

import numpy as np
import torch
import torch.nn as nn

import mlp_oracle as mo

HIDDEN = 128

# name -> L trunk layers, K0 per-row columns, S shared columns, G groups, head widths, N rows
CASES = {
    'min': dict(L=1, K0=1, S=0, G=1, heads=(1,), N=33),
    'four_heads_full': dict(L=4, K0=7, S=1, G=2, heads=(8, 8, 8, 8), N=129),
    'wide_in': dict(L=1, K0=256, S=0, G=4, heads=(32,), N=513),
    'slab_plus_one': dict(L=4, K0=129, S=1024, G=1, heads=(9, 1, 5), N=65),
    'one_slab': dict(L=2, K0=128, S=3, G=2, heads=(17, 15), N=641),
    'g1_three': dict(L=3, K0=96, S=0, G=1, heads=(3, 1), N=200),
    'g2_three': dict(L=3, K0=96, S=0, G=2, heads=(3, 1), N=200),
}

# rows against the wave (32), the workgroup (128) and the backward's chunk (512): one below, at and one above
SWEEP_N = (31, 32, 33, 127, 128, 511, 512, 1024, 1025)


def sweep(N):
    return dict(L=2, K0=8, S=0, G=4, heads=(3, 1), N=N)


def trunk(widths, trailing=0, groups=4):
    """nn.Sequential of Linear -> GroupNorm(groups, 128) -> ReLU layers over ``widths``, then a plain Linear(128,
    trailing) when ``trailing`` (the structure make_linear_layers(..., use_gn=True) builds)."""
    mods = []
    for a, b in zip(widths[:-1], widths[1:]):
        mods += [nn.Linear(a, b), nn.GroupNorm(groups, b), nn.ReLU(inplace=True)]
    if trailing:
        mods.append(nn.Linear(widths[-1], trailing))
    return nn.Sequential(*mods)


def randomise_affines(seq):
    """Non-trivial GroupNorm weights and biases (the default 1 and 0 would hide a swapped or dropped affine)."""
    for m in seq:
        if isinstance(m, nn.GroupNorm):
            with torch.no_grad():
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)


class Case:
    """One net and its data, on the CPU in float32.

    trunk, heads     the modules (heads: a list of Linears)
    segments         the first layer's column blocks in order: ('row' | 'shared', first column, end column)
    per_row, shared  the first layer's per-row and shared column indices (lists)
    x [N, K0], p [S] or None, G [N, nh]"""

    def __init__(self, spec, seed=0):
        self.spec = dict(spec)
        L, K0, S, G, heads, N = (spec[k] for k in ('L', 'K0', 'S', 'G', 'heads', 'N'))
        torch.manual_seed(seed)
        self.trunk = trunk([K0 + S] + [HIDDEN] * L, groups=G)
        randomise_affines(self.trunk)
        self.heads = [nn.Linear(HIDDEN, w) for w in heads]
        if S and K0 >= 2:
            ka = K0 // 2
            self.segments = [('row', 0, ka), ('shared', ka, ka + S), ('row', ka + S, K0 + S)]
        elif S:
            self.segments = [('row', 0, K0), ('shared', K0, K0 + S)]
        else:
            self.segments = [('row', 0, K0)]
        self.per_row = [c for kind, a, b in self.segments if kind == 'row' for c in range(a, b)]
        self.shared = [c for kind, a, b in self.segments if kind == 'shared' for c in range(a, b)]
        g = torch.Generator().manual_seed(seed + 1)
        self.x = torch.randn(N, K0, generator=g)
        self.p = torch.randn(S, generator=g) if S else None
        self.G = torch.randn(N, sum(heads), generator=g)
        self._ref = {}

    @property
    def N(self):
        return self.spec['N']

    def modules(self, device='cpu', dtype=torch.float32):
        """A copy of (trunk, heads) on ``device`` in ``dtype``."""
        return (copy.deepcopy(self.trunk).to(device=device, dtype=dtype),
                [copy.deepcopy(h).to(device=device, dtype=dtype) for h in self.heads])

    def full_input(self, dtype=torch.float32):
        """[N, K0 + S]: what the nn.Sequential itself takes (the shared row repeated per row)."""
        x, cols, o = self.x.to(dtype), [], 0
        for kind, a, b in self.segments:
            if kind == 'row':
                cols.append(x[:, o:o + b - a])
                o += b - a
            else:
                cols.append(self.p.to(dtype)[None].expand(self.N, b - a))
        return torch.cat(cols, 1)

    def blocks(self, device):
        """The input blocks as FusedMLP takes them: [N, c] per row, [S] shared."""
        out, o = [], 0
        for kind, a, b in self.segments:
            if kind == 'row':
                out.append(self.x[:, o:o + b - a].contiguous().to(device))
                o += b - a
            else:
                out.append(self.p.to(device))
        return out

    def oracle_net(self, dtype=np.float32):
        from exavatar_release_amd.mlp import parse_structure
        layers, hs = parse_structure(self.trunk, self.heads)
        return mo.net_from_modules(layers, hs, self.per_row, self.shared,
                                   self.p.numpy() if self.shared else None, dtype)

    def oracle(self, dtype=np.float32):
        """(outputs, gradients) of tests/mlp_oracle.py in ``dtype``: computed once per case and shared; read only."""
        key = np.dtype(dtype).name
        if key not in self._ref:
            net = self.oracle_net(dtype)
            x = self.x.numpy().astype(dtype)
            self._ref[key] = (mo.forward(net, x, dtype), mo.backward(net, x, self.G.numpy().astype(dtype), dtype))
        return self._ref[key]


_built = {}


def case(name_or_spec, seed=0):
    """The Case of a name of ``CASES`` or of a spec dict; built once per (spec, seed) and shared between tests."""
    spec = CASES[name_or_spec] if isinstance(name_or_spec, str) else name_or_spec
    key = (tuple(sorted((k, v) for k, v in spec.items())), seed)
    if key not in _built:
        _built[key] = Case(spec, seed)
    return _built[key]


def torch_expression(trunk_mod, heads, xin, G, dtype, device='cpu'):
    """The reference expression -- the nn.Sequential and the head Linears with autograd -- on copies of the modules in
    ``dtype`` on ``device``.  ``xin`` [N, K0 + S] is the full input.  Returns a dict of CPU tensors: 'out' [N, nh], 'x'
    (the gradient of the full input), 'layers' (a list of dicts W, b, gamma, beta), 'Wh', 'bh' (the heads stacked)."""
    from exavatar_release_amd.mlp import parse_structure
    tr = copy.deepcopy(trunk_mod).to(device=device, dtype=dtype)
    hs = [copy.deepcopy(h).to(device=device, dtype=dtype) for h in heads]
    layers, hs = parse_structure(tr, hs or None)
    xi = xin.to(device=device, dtype=dtype).clone().requires_grad_(True)
    out = tr(xi)
    if heads:
        out = torch.cat([h(out) for h in hs], 1)
    out.backward(G.to(device=device, dtype=dtype))

    def c(t):
        return t.detach().cpu()
    return {'out': c(out), 'x': c(xi.grad),
            'layers': [{'W': c(lin.weight.grad), 'b': c(lin.bias.grad), 'gamma': c(gn.weight.grad),
                        'beta': c(gn.bias.grad)} for lin, gn in layers],
            'Wh': torch.cat([c(h.weight.grad) for h in hs]), 'bh': torch.cat([c(h.bias.grad) for h in hs])}


def oracle_as_expression(cs, dtype):
    """The oracle's results of ``cs`` laid out as ``torch_expression`` returns them (numpy; the input gradient over the
    per-row columns only, layer 0's weight gradient over all of its columns)."""
    out, g = cs.oracle(dtype)
    layers = []
    for l, gl in enumerate(g['layers']):
        W = gl['W']
        if l == 0:
            W = np.zeros((HIDDEN, len(cs.per_row) + len(cs.shared)), W.dtype)
            W[:, cs.per_row] = gl['W']
            if cs.shared:
                W[:, cs.shared] = g['Ws']
        layers.append({'W': W, 'b': gl['b'], 'gamma': gl['gamma'], 'beta': gl['beta']})
    return {'out': out, 'x': g['x'], 'layers': layers, 'Wh': g['Wh'], 'bh': g['bh']}


def flat(res, per_row=None):
    """[(name, array)] of a ``torch_expression`` / ``oracle_as_expression`` result, in one fixed order; with ``per_row``
    the input gradient is cut to those columns."""
    def a(t):
        return t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    x = a(res['x'])
    items = [('outputs', a(res['out'])), ('input gradient', x[:, per_row] if per_row is not None else x)]
    for l, gl in enumerate(res['layers']):
        items += [('%s_%d' % (k, l), a(gl[k])) for k in ('W', 'b', 'gamma', 'beta')]
    return items + [('Wh', a(res['Wh'])), ('bh', a(res['bh']))]


# ---- the GPU comparison

def params_of(fm):
    ps = []
    for lin, gn in fm.layers:
        ps += [lin.weight, lin.bias, gn.weight, gn.bias]
    for h in fm.heads:
        ps += [h.weight, h.bias]
    return ps


def zero_grads(fm):
    for p in params_of(fm):
        p.grad = None


def bits_equal(a, b):
    a = np.ascontiguousarray(np.asarray(a, np.float32))
    b = np.ascontiguousarray(np.asarray(b, np.float32))
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def layout_of(blocks):
    """(per-row columns, shared columns, per-row blocks' [a, b) ranges within x) of a list of FusedMLP input blocks: a
    1-D block is shared, a 2-D block per row."""
    col, xcol, rows, shared, ranges = 0, 0, [], [], []
    for b in blocks:
        w = b.shape[-1]
        if b.dim() == 1:
            shared.extend(range(col, col + w))
            ranges.append(None)
        else:
            rows.extend(range(col, col + w))
            ranges.append((xcol, xcol + w))
            xcol += w
        col += w
    return rows, shared, ranges


def run_fused(fm, blocks, G, wrt=()):
    """Forward + backward of FusedMLP ``fm`` on the GPU over ``blocks`` (device tensors), the cotangent ``G`` [N, nh] cut
    by head.  The blocks whose index is in ``wrt`` are leaves that require grad.  Returns (outputs [N, nh] numpy, the
    list of the blocks' gradients: a tensor, or None where none was asked for)."""
    zero_grads(fm)
    leaves = [b.clone().requires_grad_(True) if k in wrt else b for k, b in enumerate(blocks)]
    outs = fm(*leaves)
    outs = outs if isinstance(outs, tuple) else (outs,)
    out = torch.cat(outs, 1)
    gl, off = [], 0
    for o in outs:
        gl.append(G[:, off:off + o.shape[1]])
        off += o.shape[1]
    if out.requires_grad:
        torch.autograd.backward(list(outs), gl)
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), [leaf.grad if k in wrt else None for k, leaf in enumerate(leaves)]


def check_against_oracle(fm, blocks, G, need_x=True, need_params=True, wrt=None, ref=None):
    """FusedMLP ``fm`` over ``blocks`` against tests/mlp_oracle.py, bit for bit: the outputs, the gradient of every
    per-row block in ``wrt`` (default: all of them) when ``need_x``, and every parameter gradient when ``need_params``
    (without it the parameters do not require grad and must get none).  ``ref``: the oracle's (outputs, gradients) of the
    same net and data when the caller has them already.  Returns the oracle's (outputs, gradients)."""
    rows, shared, ranges = layout_of(blocks)
    N = max(b.shape[0] for b in blocks if b.dim() == 2)
    if wrt is None:
        wrt = [k for k, r in enumerate(ranges) if r is not None]
    if not need_params:
        for p in params_of(fm):
            p.requires_grad_(False)
    try:
        out, gx = run_fused(fm, blocks, G, wrt if need_x else ())
    finally:
        for p in params_of(fm):
            p.requires_grad_(True)
    xin = np.concatenate([b.cpu().numpy() for b in blocks if b.dim() == 2], 1).astype(np.float32)
    if ref is None:
        p = np.concatenate([b.cpu().numpy() for b in blocks if b.dim() == 1]) if shared else None
        net = mo.net_from_modules(fm.layers, fm.heads, rows, shared, p)
        ref_out = mo.forward(net, xin)
    else:
        ref_out = ref[0]
    assert bits_equal(out, ref_out), 'forward differs from the oracle (max %g)' % np.abs(out - ref_out).max()
    if N == 0 and not need_params and not need_x:
        return ref_out, None
    g = mo.backward(net, xin, G.cpu().numpy()) if ref is None else ref[1]
    for k in wrt:
        if need_x:
            a, b = ranges[k]
            assert bits_equal(gx[k].cpu().numpy(), g['x'][:, a:b]), 'the gradient of input block %d differs' % k
        else:
            assert gx[k] is None
    if need_params:
        for l, (lin, gn) in enumerate(fm.layers):
            W = lin.weight.grad.cpu().numpy()
            want = g['layers'][l]['W']
            if l == 0 and (shared or rows != list(range(rows[0], rows[-1] + 1))):
                # layer 0's weight gets its gradient through several column views: autograd adds their zero-filled
                # slice gradients, which turns an exact -0 into +0 and changes nothing else
                want = want + np.float32(0)
            assert bits_equal(W[:, rows] if l == 0 else W, want), 'grad W_%d differs' % l
            if shared and l == 0:
                assert bits_equal(W[:, shared], g['Ws'] + np.float32(0)), 'grad of the shared columns differs'
            assert bits_equal(lin.bias.grad.cpu(), g['layers'][l]['b']), 'grad b_%d differs' % l
            assert bits_equal(gn.weight.grad.cpu(), g['layers'][l]['gamma']), 'grad gamma_%d differs' % l
            assert bits_equal(gn.bias.grad.cpu(), g['layers'][l]['beta']), 'grad beta_%d differs' % l
        Wh = np.concatenate([h.weight.grad.cpu().numpy() for h in fm.heads])
        bh = np.concatenate([h.bias.grad.cpu().numpy() for h in fm.heads])
        assert bits_equal(Wh, g['Wh']) and bits_equal(bh, g['bh']), 'head gradients differ'
    else:
        assert all(p.grad is None for p in params_of(fm))
    return ref_out, g
