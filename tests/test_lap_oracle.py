"""CPU tests of the mesh Laplacian's oracles (tests/lap_oracle.py): the float32 restatement lies within the float64
restatement's derived bound, forward and backward; the float64 backward is torch.autograd's of the reference expression;
the reference golden (tests/golden/ref_lap.npz, the reference's own class run by make_golden_lap.py) lies within the
bound; and the transposed table is a permutation of all V * K slots in the stated order."""
import os

import numpy as np
import pytest
import torch

from tests import lap_oracle as lo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_lap.npz')


def _inputs(B, Bt, V, C, seed):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal((B, V, C)).astype(np.float32), rng.standard_normal((Bt, V, C)).astype(np.float32),
            rng.standard_normal((B, V, C)).astype(np.float32), rng.uniform(0, 50, size=V).astype(np.float32))


def _within(got, want, bound, what):
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err - bound).max())
    assert (err <= bound).all(), '%s: error exceeds the bound by %g (max error %g)' % (what, worst, float(err.max()))


@pytest.mark.parametrize('B,Bt,V,C,K', [(1, 1, 50, 3, 10), (2, 1, 300, 3, 10), (2, 2, 65, 8, 16), (1, 1, 7, 1, 1)])
@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('with_target', [False, True])
def test_fp32_oracle_lies_within_the_fp64_bound(B, Bt, V, C, K, weighted, with_target):
    idx, w = lo.random_table(V, K, seed=V + K)
    out, target, G, weight = _inputs(B, Bt, V, C, seed=B * 100 + C)
    target = target if with_target else None
    weight = weight if weighted else None
    loss, d = lo.forward32(out, target, idx, w, weight)
    f = lo.forward64(out, target, idx, w, weight)
    _within(d, f['d'], f['E_d'], 'd')
    _within(loss, f['loss'], f['E_loss'], 'loss')
    grad = lo.backward32(d, G, idx, w, weight)
    g64, E = lo.backward64(f['d'], f['E_d'], G, idx, w, weight)
    _within(grad, g64, E, 'dL/dout')
    assert float(E.max()) < 1e-2 * float(np.abs(g64).max())       # the bound is a rounding bound, not a loose one


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('with_target', [False, True])
def test_backward_is_autograd_of_the_reference_expression_in_float64(weighted, with_target):
    B, V, C, K = 2, 120, 3, 10
    idx, w = lo.random_table(V, K, seed=5)
    out, target, G, weight = _inputs(B, 1, V, C, seed=6)
    target = target if with_target else None
    weight = weight if weighted else None
    x = torch.from_numpy(out).double().requires_grad_(True)
    ti, tw = torch.from_numpy(idx), torch.from_numpy(w).double()

    def lap(y):        # the reference's compute_laplacian
        return y + (y[:, ti] * tw[None, :, :, None]).sum(2)

    loss = (lap(x) - lap(torch.from_numpy(target).double())) ** 2 if with_target else lap(x) ** 2
    if weighted:
        loss = loss * torch.from_numpy(weight).double().view(1, V, 1)
    (loss * torch.from_numpy(G).double()).sum().backward()
    f = lo.forward64(out, target, idx, w, weight)
    g64, E = lo.backward64(f['d'], f['E_d'], G, idx, w, weight)
    np.testing.assert_allclose(loss.detach().numpy(), f['loss'], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g64, x.grad.numpy(), rtol=1e-11, atol=1e-11)
    d32 = lo.forward32(out, target, idx, w, weight)[1]
    _within(lo.backward32(d32, G, idx, w, weight), x.grad.numpy(), E, 'dL/dout against autograd')


def test_reference_golden_lies_within_the_bound():
    z = np.load(GOLDEN)
    idx, w = z['neighbor_idxs'], z['neighbor_weights']
    for name, target in (('none', None), ('target', z['target']), ('target1', z['target1'])):
        f = lo.forward64(z['out'], target, idx, w)
        _within(z['loss_' + name], f['loss'], f['E_loss'], 'golden loss_' + name)
        g64, E = lo.backward64(f['d'], f['E_d'], z['G'], idx, w)
        _within(z['grad_' + name], g64, E, 'golden grad_' + name)
        # and the float32 oracle against the golden: both within one bound of the exact value
        loss32, d32 = lo.forward32(z['out'], target, idx, w)
        assert (np.abs(loss32.astype(np.float64) - z['loss_' + name]) <= 2 * f['E_loss']).all()
        assert (np.abs(lo.backward32(d32, z['G'], idx, w).astype(np.float64) - z['grad_' + name]) <= 2 * E).all()


def test_golden_hub_keeps_ten_neighbours_that_are_not_its_ten_smallest():
    z = np.load(GOLDEN)
    kept = z['neighbor_idxs'][int(z['hub'])].tolist()
    rim = sorted(z['rim'].tolist())
    assert len(rim) > 10 and set(kept) <= set(rim) and len(set(kept)) == 10
    assert sorted(kept) != rim[:10] and kept != sorted(kept)
    assert (z['neighbor_weights'][int(z['hub'])] == np.float32(-0.1)).all()
    valence = (z['neighbor_weights'] != 0).sum(1)
    assert {2, 3}.issubset(valence.tolist())


@pytest.mark.parametrize('V,K', [(1, 1), (9, 3), (200, 10), (64, 16)])
def test_transposed_table_is_a_permutation_in_the_stated_order(V, K):
    idx, _ = lo.random_table(V, K, seed=V)
    offsets, entries = lo.transpose(idx)
    assert offsets[0] == 0 and offsets[-1] == V * K and (np.diff(offsets) >= 0).all()
    assert sorted(entries.tolist()) == list(range(V * K))
    flat = idx.reshape(-1)
    for v in range(V):
        mine = entries[offsets[v]:offsets[v + 1]]
        assert (flat[mine] == v).all()
        assert (np.diff(mine) > 0).all()                  # ascending u * K + k = ascending u, then k
