"""The HIP mesh Laplacian regulariser (exavatar_release_amd.LaplacianReg / mesh_laplacian_loss) on the GPU.

The loss, d and dL/dout must equal the float32 oracle tests/lap_oracle.py BIT FOR BIT: the header fixes every rounding,
the order of the slots and the order of every vertex's incoming sum.  Against the reference's own class (the golden) the
results stay within twice the float64 oracle's derived bound -- both sides lie within one bound of the exact value.  The
backward repeats bit for bit; the PyTorch expression it replaces (gather, multiply, sum; an ``index_put_`` scatter-add
backward in an order of PyTorch's choosing), run on the same device, agrees within the bound and is deliberately NOT
compared bit for bit.
A captured graph replays with new inputs.  torch.autograd.gradcheck is of no use in float32; the float64 oracle, which
tests/test_lap_oracle.py checks against autograd, stands in for it."""
import os

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd.mesh_reg import LaplacianReg, mesh_laplacian_loss
from tests import lap_oracle as lo

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_lap.npz')
GRID = 409           # 409 x 409 = 167 281 vertices: the size of the reference's upsampled human mesh


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want, what):
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape, what
    bad = got != want
    assert not bad.any(), '%s: %d of %d elements differ in their bits' % (what, int(bad.sum()), bad.size)


def _data(B, Bt, V, C, seed):
    rng = np.random.RandomState(seed)
    return dict(out=rng.standard_normal((B, V, C)).astype(np.float32),
                target=rng.standard_normal((Bt, V, C)).astype(np.float32),
                G=rng.standard_normal((B, V, C)).astype(np.float32),
                weight=rng.uniform(0, 50, size=V).astype(np.float32))


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(fn, out, target, weight, G):
    """fn(out, target, weight) -> (loss, d) on the device; returns numpy (loss, d, dL/dout)."""
    x = _t(out).requires_grad_(True)
    loss, d = fn(x, _t(target), _t(weight))
    grad, = torch.autograd.grad(loss, x, _t(G))
    return loss.detach().cpu().numpy(), d.cpu().numpy(), grad.cpu().numpy()


def _check_against_oracle(fn, idx, w, c, with_target, weighted, what):
    target = c['target'] if with_target else None
    weight = c['weight'] if weighted else None
    loss, d, grad = _run(fn, c['out'], target, weight, c['G'])
    loss32, d32 = lo.forward32(c['out'], target, idx, w, weight)
    _same_bits(d, d32, what + ' d')
    _same_bits(loss, loss32, what + ' loss')
    _same_bits(grad, lo.backward32(d32, c['G'], idx, w, weight), what + ' dL/dout')


@pytest.mark.parametrize('K', [1, 10, 16])
@pytest.mark.parametrize('V', [1, 63, 64, 65, 4097])
def test_forward_and_backward_equal_the_fp32_oracle_bit_for_bit(V, K):
    """Random tables with general weights, padded slots, a vertex that hundreds of slots name and one that none does."""
    idx, w = lo.random_table(V, K, seed=31 * V + K, hub=True, orphan=True)
    if V * K >= 600:
        assert (idx == 0).sum() >= 100
    assert V == 1 or not (idx == V - 1).any()
    ti, tw = _t(idx), _t(w)

    def fn(x, target, weight):
        return mesh_laplacian_loss(x, target, ti, tw, weight, return_d=True)

    for C in (1, 3, 8):
        for B, Bt in ((1, 1), (2, 1), (2, 2)):
            c = _data(B, Bt, V, C, seed=V + 7 * C + B + Bt)
            for with_target in (False, True):
                if not with_target and Bt != B:
                    continue                               # without a target Bt plays no part
                for weighted in (False, True):
                    _check_against_oracle(fn, idx, w, c, with_target, weighted,
                                          'C=%d B=%d Bt=%d target=%s weight=%s' % (C, B, Bt, with_target, weighted))


@pytest.fixture(scope='module')
def big_grid():
    V = GRID * GRID
    reg = LaplacianReg(V, lo.grid_faces(GRID, GRID))
    return reg, reg.neighbor_idxs.cpu().numpy(), reg.neighbor_weights.cpu().numpy()


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('with_target', [False, True])
def test_the_167k_vertex_grid_equals_the_fp32_oracle_bit_for_bit(big_grid, with_target, weighted):
    reg, idx, w = big_grid
    V = idx.shape[0]
    assert V == 167281 and idx.shape[1] == 10 and (w[:, 6:] == 0).all() and (w[0, 2:] == 0).all()      # padded slots
    ti, tw = reg.neighbor_idxs, reg.neighbor_weights

    def fn(x, target, weight):
        return mesh_laplacian_loss(x, target, ti, tw, weight, return_d=True)

    c = _data(1, 1, V, 3, seed=167)
    _check_against_oracle(fn, idx, w, c, with_target, weighted, 'grid')
    # the module gives the functional form's loss, with every shape of weight it accepts
    x = _t(c['out'])
    target = _t(c['target']) if with_target else None
    want = fn(x, target, _t(c['weight']) if weighted else None)[0]
    if weighted:
        for shape in ((V,), (1, V, 1), (V, 1)):
            assert torch.equal(reg(x, target, _t(c['weight']).reshape(shape)), want)
    else:
        assert torch.equal(reg(x, target), want)


def test_a_large_fan_equals_the_fp32_oracle_bit_for_bit():
    """A 40 x 40 grid and a closed fan of 300 triangles: the hub keeps ten of its 300 neighbours, and 300 rows name it."""
    n, rim = 40, 300
    hub = n * n
    r = hub + 1 + np.arange(rim)
    face = np.concatenate([lo.grid_faces(n, n), np.stack([np.full(rim, hub), r, np.roll(r, -1)], 1)])
    V = hub + 1 + rim
    reg = LaplacianReg(V, face)
    idx, w = reg.neighbor_idxs.cpu().numpy(), reg.neighbor_weights.cpu().numpy()
    assert (idx == hub).sum() == rim and (w[hub] == np.float32(-0.1)).all()
    for B, Bt in ((1, 1), (2, 1)):
        c = _data(B, Bt, V, 3, seed=B)
        for with_target in (False, True):
            for weighted in (False, True):
                target = c['target'] if with_target else None
                weight = c['weight'] if weighted else None
                x = _t(c['out']).requires_grad_(True)
                loss = reg(x, _t(target), _t(weight))
                grad, = torch.autograd.grad(loss, x, _t(c['G']))
                loss32, d32 = lo.forward32(c['out'], target, idx, w, weight)
                _same_bits(loss.detach().cpu().numpy(), loss32, 'fan loss')
                _same_bits(grad.cpu().numpy(), lo.backward32(d32, c['G'], idx, w, weight), 'fan dL/dout')


def test_within_twice_the_bound_of_the_reference_golden():
    z = np.load(GOLDEN)
    V = z['neighbor_idxs'].shape[0]
    reg = LaplacianReg(V, z['face'])
    assert np.array_equal(reg.neighbor_idxs.cpu().numpy(), z['neighbor_idxs'])
    assert np.array_equal(reg.neighbor_weights.cpu().numpy(), z['neighbor_weights'])
    for name, target in (('none', None), ('target', z['target']), ('target1', z['target1'])):
        x = _t(z['out']).requires_grad_(True)
        loss = reg(x, _t(target))
        grad, = torch.autograd.grad(loss, x, _t(z['G']))
        f = lo.forward64(z['out'], target, z['neighbor_idxs'], z['neighbor_weights'])
        g64, E = lo.backward64(f['d'], f['E_d'], z['G'], z['neighbor_idxs'], z['neighbor_weights'])
        err = np.abs(loss.detach().cpu().numpy().astype(np.float64) - z['loss_' + name])
        gerr = np.abs(grad.cpu().numpy().astype(np.float64) - z['grad_' + name])
        print('golden %s: loss max err %.3e (max bound %.3e), grad max err %.3e (max bound %.3e)'
              % (name, err.max(), f['E_loss'].max(), gerr.max(), E.max()))
        assert (err <= 2 * f['E_loss']).all(), name
        assert (gerr <= 2 * E).all(), name


def _torch_reference(x, target, idx, w, weight):
    """The reference's expression (loss.py:118-131) with model.py's ``* weight``, as PyTorch runs it on the device."""
    def lap(y):
        return y + (y[:, idx] * w[None, :, :, None]).sum(2)

    loss = lap(x) ** 2 if target is None else (lap(x) - lap(target)) ** 2
    return loss if weight is None else loss * weight.view(1, -1, 1)


@pytest.mark.parametrize('with_target', [False, True])
def test_backward_repeats_bit_for_bit_and_agrees_with_the_torch_scatter_add_within_the_bound(big_grid, with_target):
    reg, idx, w = big_grid
    V = idx.shape[0]
    c = _data(1, 1, V, 3, seed=3)
    target = c['target'] if with_target else None
    x = _t(c['out']).requires_grad_(True)
    G, tt, tw = _t(c['G']), _t(target), _t(c['weight'])
    grads = [torch.autograd.grad(reg(x, tt, tw), x, G)[0].cpu().numpy() for _ in range(3)]
    for again in grads[1:]:
        _same_bits(again, grads[0], 'repeated backward')
    ref_loss = _torch_reference(x, tt, reg.neighbor_idxs, reg.neighbor_weights, tw)
    ref_grad, = torch.autograd.grad(ref_loss, x, G)
    f = lo.forward64(c['out'], target, idx, w, c['weight'])
    g64, E = lo.backward64(f['d'], f['E_d'], c['G'], idx, w, c['weight'])
    lerr = np.abs(reg(x, tt, tw).detach().cpu().numpy().astype(np.float64) - ref_loss.detach().cpu().numpy())
    gerr = np.abs(grads[0].astype(np.float64) - ref_grad.cpu().numpy())
    differ = int((_bits(grads[0]) != _bits(ref_grad.cpu().numpy())).sum())
    print('torch on the device, target=%s: loss max err %.3e (max bound %.3e), grad max err %.3e (max bound %.3e), '
          '%d of %d gradient elements differ in their bits' % (with_target, lerr.max(), f['E_loss'].max(), gerr.max(),
                                                              E.max(), differ, gerr.size))
    assert (lerr <= f['E_loss']).all()
    assert (gerr <= E).all()
    # and each side alone lies within the bound of the exact value
    assert (np.abs(grads[0] - g64) <= E).all() and (np.abs(ref_grad.cpu().numpy() - g64) <= E).all()


def test_graph_capture_replays_with_new_inputs(big_grid):
    reg, idx, w = big_grid
    V = idx.shape[0]
    c = _data(1, 1, V, 3, seed=11)
    x = _t(c['out']).requires_grad_(True)
    target, weight, G = _t(c['target']), _t(c['weight']), _t(c['G'])

    def step():
        l1 = reg(x, target, weight)
        l2 = reg(x, None, weight)
        return l1, l2, torch.autograd.grad([l1, l2], x, [G, G])[0]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        l1, l2, grad = step()
    new = _data(1, 1, V, 3, seed=12)
    with torch.no_grad():
        x.copy_(_t(new['out']))
        target.copy_(_t(new['target']))
        G.copy_(_t(new['G']))
    graph.replay()
    torch.cuda.synchronize()
    e1, e2, egrad = step()
    assert torch.equal(l1, e1) and torch.equal(l2, e2)
    _same_bits(grad.cpu().numpy(), egrad.cpu().numpy(), 'replayed dL/dout')
    loss32, d32 = lo.forward32(new['out'], new['target'], idx, w, c['weight'])
    _same_bits(l1.detach().cpu().numpy(), loss32, 'replayed loss')


def test_python_surface_on_the_device():
    face = lo.grid_faces(6, 7)
    V = 42
    reg = LaplacianReg(V, face)
    assert reg.neighbor_idxs.is_cuda and reg.neighbor_idxs.dtype == torch.int64
    x = torch.randn(2, V, 3, device=DEV)
    with pytest.raises(ValueError, match='data in the reference and gets no gradient'):
        reg(x, x.clone().requires_grad_(True))
    with pytest.raises(ValueError, match='data in the reference and gets no gradient'):
        reg(x, None, torch.ones(V, device=DEV, requires_grad=True))
    with pytest.raises(ValueError, match='float32'):
        reg(x.double(), None)
    with pytest.raises(ValueError, match=r'\[B, V, C\]'):
        reg(x[:, :41], None)
    with pytest.raises(ValueError, match=r'\[B, V, C\]'):
        reg(torch.randn(2, V, 9, device=DEV), None)
    with pytest.raises(ValueError, match=r'\[1, V, C\]'):
        reg(torch.randn(3, V, 3, device=DEV), x)
    with pytest.raises(ValueError, match='weight must be'):
        reg(x, None, torch.ones(V, 3, device=DEV))
    with pytest.raises(ValueError, match='outside'):
        mesh_laplacian_loss(x, None, torch.full((V, 2), V, dtype=torch.int64, device=DEV), torch.zeros(V, 2, device=DEV))
    # non-contiguous inputs are made contiguous; a zero batch is a no-op
    xt = torch.randn(3, V, 2, device=DEV).permute(2, 1, 0)
    assert torch.equal(reg(xt, None), reg(xt.contiguous(), None))
    assert reg(x[:0], None).shape == (0, V, 3)
    assert exa.LaplacianReg is LaplacianReg
