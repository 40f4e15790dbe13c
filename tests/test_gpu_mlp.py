"""GPU tests of exavatar_release_amd.FusedMLP (include/exa_mlp.h) on the four MLPs of ExAvatar's HumanGaussian.

The forward and every gradient must equal tests/mlp_oracle.py (the header restated in numpy) bit for bit; a row's bits
must not depend on N or on its position; repeated calls and graph replays must give the same bits; and at the
reference's size the result must agree with PyTorch's fp32 nn.Sequential + autograd within a stated bound."""
import copy

import pytest
import torch
import torch.nn as nn

import mlp_cases as mc
import mlp_oracle as mo
from mlp_cases import bits_equal, params_of, trunk, zero_grads

pytestmark = pytest.mark.gpu

TRI, POSE, NORMAL = 96, 126, 3          # triplane feature (3 x 32), body pose 6d (21 x 6), normal


def reference_nets(seed=0):
    """The four nets at their real widths, with non-trivial GroupNorm affines; name -> (trunk, heads, blocks) where
    blocks lists the input blocks as 'tri' / 'pose' / 'normal'."""
    torch.manual_seed(seed)
    nets = {
        'geo': (trunk([TRI, 128, 128, 128]), (nn.Sequential(nn.Linear(128, 3)), nn.Sequential(nn.Linear(128, 1))),
                ('tri',)),
        'geo_offset': (trunk([TRI + POSE, 128, 128, 128]), (nn.Sequential(nn.Linear(128, 3)),
                                                              nn.Sequential(nn.Linear(128, 1))), ('tri', 'pose')),
        'rgb': (trunk([TRI, 128, 128, 128], trailing=3), None, ('tri',)),
        'rgb_offset': (trunk([TRI + POSE + NORMAL, 128, 128, 128], trailing=3), None, ('tri', 'pose', 'normal')),
    }
    for tr, heads, _ in nets.values():
        for m in tr:
            if isinstance(m, nn.GroupNorm):
                with torch.no_grad():
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.uniform_(-0.2, 0.2)
        tr.cuda()
        for h in heads or ():
            h.cuda()
    return nets


def inputs(N, seed=1):
    """The input blocks: 'pose' is the shared [126] row (folded into the bias), 'pose_rows' the same row repeated per row
    as the reference builds it ([N, 126], a per-row block: the first layer then reads 222 or 225 columns per row)."""
    g = torch.Generator().manual_seed(seed)
    x = {'tri': torch.randn(N, TRI, generator=g).cuda(), 'pose': torch.randn(POSE, generator=g).cuda(),
         'normal': torch.nn.functional.normalize(torch.randn(N, NORMAL, generator=g), dim=1).cuda()}
    x['pose_rows'] = x['pose'][None].expand(N, POSE).contiguous()
    return x


def block_args(x, tri, blocks):
    return [tri if b == 'tri' else x[b] for b in blocks]


def unfolded(blocks):
    return tuple('pose_rows' if b == 'pose' else b for b in blocks)


def run(fm, blocks, x, G, need_x=True):
    """Forward + backward on the GPU; returns (outs [N, nh] numpy, the gradient of tri_feat)."""
    out, grads = mc.run_fused(fm, [x[b] for b in blocks], G, wrt=(blocks.index('tri'),) if need_x else ())
    return out, grads[blocks.index('tri')]


def check_against_oracle(fm, blocks, x, G, need_x=True, need_params=True):
    """mlp_cases.check_against_oracle over the named blocks; 'pose' is the shared (1-D) block, tri_feat the leaf."""
    mc.check_against_oracle(fm, [x[b] for b in blocks], G, need_x, need_params, wrt=(blocks.index('tri'),))


def make(name, nets):
    import exavatar_release_amd as exa
    tr, heads, blocks = nets[name]
    return exa.FusedMLP(tr, heads=heads), blocks


@pytest.fixture(scope='module')
def nets():
    return reference_nets()


@pytest.mark.parametrize('name', ['geo', 'geo_offset', 'rgb', 'rgb_offset'])
def test_bit_exact_reference_nets(nets, name):
    fm, blocks = make(name, nets)
    N = 2000
    x = inputs(N)
    nh = sum(h.out_features for h in fm.heads)
    G = torch.randn(N, nh, generator=torch.Generator().manual_seed(5)).cuda()
    check_against_oracle(fm, blocks, x, G)


@pytest.mark.parametrize('name', ['geo_offset', 'rgb_offset'])
def test_bit_exact_pose_per_row(nets, name):
    """The pose repeated per row, as the reference builds it: 222 / 225 per-row columns, so the first layer's second
    LDS slab, the input gradient's second slab and weight-gradient tiles 4-7 all run."""
    fm, blocks = make(name, nets)
    N = 1300
    x = inputs(N, seed=17)
    nh = sum(h.out_features for h in fm.heads)
    G = torch.randn(N, nh, generator=torch.Generator().manual_seed(17)).cuda()
    check_against_oracle(fm, unfolded(blocks), x, G)


@pytest.mark.parametrize('N', [0, 1, 63, 64, 65, 1100])
def test_bit_exact_ragged(nets, N):
    fm, blocks = make('rgb_offset', nets)
    x = inputs(N, seed=N + 7)
    G = torch.randn(N, 3, generator=torch.Generator().manual_seed(N)).cuda()
    check_against_oracle(fm, blocks, x, G)
    if N == 0:
        for p in params_of(fm):
            assert bool((p.grad == 0).all()) and not bool(torch.signbit(p.grad).any()), 'N = 0 must give +0 gradients'


@pytest.mark.parametrize('what', ['params_only', 'x_only'])
def test_bit_exact_partial_gradients(nets, what):
    fm, blocks = make('geo_offset', nets)
    N = 777
    x = inputs(N, seed=3)
    G = torch.randn(N, 4, generator=torch.Generator().manual_seed(3)).cuda()
    check_against_oracle(fm, blocks, x, G, need_x=what == 'x_only', need_params=what == 'params_only')


def test_bit_exact_under_poison(nets):
    import exavatar_release_amd as exa
    fm, blocks = make('geo', nets)
    N = 1500
    x = inputs(N, seed=11)
    G = torch.randn(N, 4, generator=torch.Generator().manual_seed(11)).cuda()
    old = exa.config.poison
    exa.config.poison = True
    try:
        check_against_oracle(fm, blocks, x, G)
    finally:
        exa.config.poison = old


@pytest.mark.parametrize('groups', [1, 2])
def test_bit_exact_other_group_counts(groups):
    import exavatar_release_amd as exa
    torch.manual_seed(groups)
    tr = trunk([40, 128, 128], trailing=5, groups=groups).cuda()
    fm = exa.FusedMLP(tr)
    N = 600
    g = torch.Generator().manual_seed(groups)
    x = torch.randn(N, 40, generator=g).cuda().requires_grad_(True)
    G = torch.randn(N, 5, generator=g).cuda()
    out = fm(x)
    out.backward(G)
    net = mo.net_from_modules(fm.layers, fm.heads, list(range(40)))
    xn = x.detach().cpu().numpy()
    assert bits_equal(out.detach().cpu(), mo.forward(net, xn))
    ref = mo.backward(net, xn, G.cpu().numpy())
    assert bits_equal(x.grad.cpu(), ref['x'])
    for l, (lin, gn) in enumerate(fm.layers):
        assert bits_equal(lin.weight.grad.cpu(), ref['layers'][l]['W'])
        assert bits_equal(lin.bias.grad.cpu(), ref['layers'][l]['b'])
        assert bits_equal(gn.weight.grad.cpu(), ref['layers'][l]['gamma'])
        assert bits_equal(gn.bias.grad.cpu(), ref['layers'][l]['beta'])
    assert bits_equal(fm.heads[0].weight.grad.cpu(), ref['Wh'])
    assert bits_equal(fm.heads[0].bias.grad.cpu(), ref['bh'])


def test_rows_independent_of_batch(nets):
    fm, blocks = make('geo_offset', nets)
    N = 3000
    x = inputs(N, seed=21)
    torch.set_grad_enabled(False)
    try:
        full = torch.cat(fm(x['tri'], x['pose']), 1)
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(2)).cuda()
        permuted = torch.cat(fm(x['tri'][perm].contiguous(), x['pose']), 1)
        part = torch.cat(fm(x['tri'][1234:1301].contiguous(), x['pose']), 1)
    finally:
        torch.set_grad_enabled(True)
    assert bits_equal(permuted.cpu(), full[perm].cpu())
    assert bits_equal(part.cpu(), full[1234:1301].cpu())


def test_repeated_calls_identical(nets):
    fm, blocks = make('rgb_offset', nets)
    N = 5000
    x = inputs(N, seed=4)
    G = torch.randn(N, 3, generator=torch.Generator().manual_seed(4)).cuda()
    res = []
    for _ in range(3):
        out, gx = run(fm, blocks, x, G)
        res.append([out, gx.cpu().numpy()] + [p.grad.cpu().numpy() for p in params_of(fm)])
    for r in res[1:]:
        assert all(bits_equal(a, b) for a, b in zip(r, res[0]))


def test_graph_capture_replays_new_inputs(nets):
    fm, blocks = make('geo', nets)
    N = 1000
    tri = torch.randn(N, TRI, device='cuda', requires_grad=True)
    G = torch.randn(N, 4, device='cuda')
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                           # warm up the allocator outside the capture
        for _ in range(2):
            zero_grads(fm)
            tri.grad = None
            o = torch.cat(fm(tri), 1)
            o.backward(G)
    torch.cuda.current_stream().wait_stream(s)
    zero_grads(fm)
    tri.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = torch.cat(fm(tri), 1)
        o.backward(G)
    # new inputs and new parameters, then replay and compare with an eager call
    with torch.no_grad():
        tri.copy_(torch.randn(N, TRI, generator=torch.Generator().manual_seed(9)).cuda())
        G.copy_(torch.randn(N, 4, generator=torch.Generator().manual_seed(10)).cuda())
        fm.layers[1][0].weight.mul_(0.9)
        fm.heads[0].bias.add_(0.1)
    graph.replay()
    torch.cuda.synchronize()
    got = [o.detach().clone(), tri.grad.clone()] + [p.grad.clone() for p in params_of(fm)]
    zero_grads(fm)
    t2 = tri.detach().clone().requires_grad_(True)
    o2 = torch.cat(fm(t2), 1)
    o2.backward(G)
    want = [o2.detach(), t2.grad] + [p.grad for p in params_of(fm)]
    for a, b in zip(got, want):
        assert bits_equal(a.cpu(), b.cpu())


def _torch_expression(fm, xin, G, device, dtype):
    """The reference expression -- the nn.Sequential (and head Linears) with autograd -- on a copy of the modules in
    ``dtype`` on ``device``.  Returns [outputs, grad tri_feat, grads of params_of order] in float64 on the CPU."""
    from exavatar_release_amd.mlp import parse_structure
    tr = copy.deepcopy(fm.trunk).to(device, dtype)
    trailing = isinstance(tr[-1], nn.Linear)
    heads = [] if trailing else [copy.deepcopy(h).to(device, dtype) for h in fm.heads]
    layers, hs = parse_structure(tr, heads or None)
    ps = [t for lin, gn in layers for t in (lin.weight, lin.bias, gn.weight, gn.bias)] + \
        [t for h in hs for t in (h.weight, h.bias)]
    xi = xin.to(device, dtype).requires_grad_(True)
    h = tr(xi)
    out = h if trailing else torch.cat([hd(h) for hd in heads], 1)
    out.backward(G.to(device, dtype))
    return [t.detach().cpu().double() for t in [out, xi.grad[:, :TRI]] + [p.grad for p in ps]]


def _bound_check(fm, blocks, N, seed):
    """FusedMLP against the reference expression in fp32, both measured against the same expression in float64.
    Bound, per result tensor (outputs, tri_feat's gradient, every parameter gradient), with e64 the float64 value:
        max |fused - e64| <= 16 * max |torch_fp32 - e64| + 64 * 2^-24 * rms(e64)
    i.e. FusedMLP's error is at most a small multiple of the first-order rounding error the fp32 expression itself
    makes on the same data, plus a floor of 64 units of fp32 rounding at the tensor's scale.  The factor allows for the
    summation shapes: the fused backward sums rows sequentially in chunks of 512 (first-order error growing with the
    chunk length), where PyTorch's reductions are tree-shaped (growing with its logarithm).

    The float64 expression runs on the CPU.  The fp32 expression runs on the GPU, except for the GroupNorm weight and
    bias gradients: PyTorch-ROCm's GroupNorm backward on [N, C] input gives wrong affine gradients on this platform (in
    fp32 and fp64 alike; its input gradient is right), so for those two the fp32 expression is taken on the CPU."""
    x = inputs(N, seed)
    xin = torch.cat([x[b] if b != 'pose' else x['pose'][None].expand(N, POSE) for b in blocks], 1).cpu()
    nh = sum(h.out_features for h in fm.heads)
    G = torch.randn(N, nh, generator=torch.Generator().manual_seed(seed))
    r64 = _torch_expression(fm, xin, G, 'cpu', torch.float64)
    r32 = _torch_expression(fm, xin, G, 'cuda', torch.float32)
    r32cpu = _torch_expression(fm, xin, G, 'cpu', torch.float32)
    for k in range(2, len(r32) - 2 * len(fm.heads)):
        if (k - 2) % 4 in (2, 3):                       # gamma_l, beta_l
            r32[k] = r32cpu[k]
    zero_grads(fm)
    tri = x['tri'].clone().requires_grad_(True)
    outs = fm(*block_args(x, tri, blocks))
    outs = outs if isinstance(outs, tuple) else (outs,)
    out = torch.cat(outs, 1)
    out.backward(G.cuda())
    rf = [t.detach().cpu().double() for t in [out, tri.grad] + [p.grad for p in params_of(fm)]]
    for k, (a64, a32, af) in enumerate(zip(r64, r32, rf)):
        err_t = float((a32 - a64).abs().max())
        err_f = float((af - a64).abs().max())
        bound = 16 * err_t + 64 * 2.0 ** -24 * float(a64.pow(2).mean().sqrt())
        assert err_f <= bound, 'result %d: FusedMLP error %g > bound %g (fp32 expression error %g)' % (k, err_f, bound,
                                                                                                       err_t)


@pytest.mark.parametrize('pose', ['folded', 'per_row'])
@pytest.mark.parametrize('name', ['geo_offset', 'rgb_offset'])
def test_reference_expression_at_full_size(nets, name, pose):
    fm, blocks = make(name, nets)
    _bound_check(fm, blocks if pose == 'folded' else unfolded(blocks), 167_000, seed=31)


def test_training_loop_reproducible():
    """TriplaneFeatures -> FusedMLP -> loss -> Adam, run twice from the same state: bit-identical parameters."""
    import exavatar_release_amd as exa

    def train():
        torch.manual_seed(123)
        N = 4000
        pos = (torch.rand(N, 3) * 2 - 1).cuda()
        is_face = torch.zeros(N, dtype=torch.bool, device='cuda')
        is_face[:500] = True
        tf = exa.TriplaneFeatures(pos, is_face)
        planes = torch.nn.Parameter(torch.randn(3, 32, 128, 128, device='cuda') * 0.1)
        planes_face = torch.nn.Parameter(torch.randn(3, 32, 128, 128, device='cuda') * 0.1)
        tr = trunk([TRI, 128, 128, 128], trailing=3).cuda()
        fm = exa.FusedMLP(tr)
        target = torch.rand(N, 3, device='cuda')
        opt = torch.optim.Adam(list(tr.parameters()) + [planes, planes_face], lr=1e-3)
        for _ in range(5):
            opt.zero_grad()
            loss = (fm(tf(planes, planes_face)) - target).abs().mean()
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        return [p.detach().cpu().numpy() for p in tr.parameters()] + [planes.detach().cpu().numpy()]

    a, b = train(), train()
    assert all(bits_equal(x, y) for x, y in zip(a, b))
