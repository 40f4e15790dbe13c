"""CPU checks of the skinning oracle (tests/skin_oracle.py) -- the restatement the HIP skinning is held to bit for bit:
in float64 it equals the reference's own code (tests/golden/ref_skinning.npz, cut from module.py and executed) and the
autograd of the reference expression to 1e-12; in float32 it stays within its first-order bound K u sum|terms| of
float64 with at least a factor of 2 to spare; and it gives the known answers."""
import os

import numpy as np
import pytest
import torch

from tests import skin_oracle as so

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_skinning.npz')


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _case(V, Vw, J, S, seed, use_idx=True, cam=True, sparse=False, rigid=False, dtype=np.float64):
    rng = np.random.default_rng(seed)
    if sparse:
        W = np.zeros((Vw, J))
        for v in range(Vw):
            cols = rng.permutation(J)[:rng.integers(1, 5)]
            w = rng.random(cols.size) + 0.05
            W[v, cols] = w / w.sum()
    else:
        W = rng.random((Vw, J))
    if rigid:
        T = np.zeros((J, 4, 4))
        for j in range(J):
            q, r = np.linalg.qr(rng.standard_normal((3, 3)))
            T[j, :3, :3] = q * np.sign(np.diag(r))[None, :]
            T[j, :3, 3] = 0.3 * rng.standard_normal(3)
        T[:, 3, 3] = 1
    else:
        T = rng.standard_normal((J, 4, 4))
    idx = rng.integers(0, Vw, V) if use_idx else None
    pts = [0.4 * rng.standard_normal((V, 3)) for _ in range(S)]
    G = [rng.standard_normal((V, 3)) for _ in range(S)]
    trans = 0.5 * rng.standard_normal(3)
    R = np.linalg.qr(rng.standard_normal((3, 3)))[0] if cam else None
    t = 0.7 * rng.standard_normal(3) if cam else None
    cast = lambda a: None if a is None else np.asarray(a, dtype)      # noqa: E731
    return dict(points=[cast(p) for p in pts], grads=[cast(g) for g in G], T=cast(T), weights=cast(W), idx=idx,
                trans=cast(trans), R=cast(R), t=cast(t))


def _oracle(c, dtype):
    Rinv = None if c['R'] is None else np.linalg.inv(np.asarray(c['R'], np.float64)).astype(dtype)
    fwd = so.forward(c['points'], c['T'], c['weights'], c['idx'], c['trans'], Rinv, c['t'], dtype)
    bwd = so.backward(c['points'], c['grads'], c['T'], c['weights'], c['idx'], Rinv, dtype)
    return fwd, bwd, Rinv


def test_float64_oracle_equals_the_reference_code_golden():
    z = np.load(GOLDEN)
    for name in z['cases']:
        p = str(name) + '_'
        V, Vw, J, S, use_idx, cam = (int(x) for x in z[p + 'dims'])
        pts = [z[p + 'points%d' % s] for s in range(S)]
        idx = z[p + 'idx'] if use_idx else None
        Rinv = np.linalg.inv(z[p + 'R']) if cam else None
        t = z[p + 't'] if cam else None
        fwd = so.forward(pts, z[p + 'T'], z[p + 'weights'], idx, z[p + 'trans'], Rinv, t, np.float64)
        gp, gT, gtr = so.backward(pts, [z[p + 'G%d' % s] for s in range(S)], z[p + 'T'], z[p + 'weights'], idx, Rinv,
                                  np.float64)
        for s in range(S):
            assert _rel(fwd[s], z[p + 'posed%d' % s]) <= 1e-12, (name, s)
            assert _rel(gp[s], z[p + 'grad_points%d' % s]) <= 1e-12, (name, s)
        assert _rel(gT, z[p + 'grad_T']) <= 1e-12, name
        assert np.all(z[p + 'grad_T'][:, 3, :] == 0) and np.all(gT[:, 3, :] == 0)
        assert _rel(gtr, z[p + 'grad_trans'].reshape(3)) <= 1e-12, name
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize('V,Vw,J,S,use_idx,cam,sparse', [(1000, 400, 55, 2, True, True, True), (257, 257, 1, 1, False, False, False),
                                                        (600, 90, 64, 4, True, False, False), (255, 255, 24, 3, False, True, True)])
def test_float64_oracle_is_autograd_of_the_reference_expression(V, Vw, J, S, use_idx, cam, sparse):
    c = _case(V, Vw, J, S, seed=V + J, use_idx=use_idx, cam=cam, sparse=sparse)
    fwd, (gp, gT, gtr), _ = _oracle(c, np.float64)
    tt = lambda a, g=False: None if a is None else torch.tensor(a, dtype=torch.float64, requires_grad=g)      # noqa: E731
    pts = [tt(p, True) for p in c['points']]
    T, trans = tt(c['T'], True), tt(c['trans'], True)
    idx = None if c['idx'] is None else torch.as_tensor(c['idx'])
    ref = so.reference_expression(pts, T, tt(c['weights']), idx, trans, tt(c['R']), tt(c['t']))
    grads = torch.autograd.grad(ref, [T, trans] + pts, [torch.tensor(g) for g in c['grads']])
    for s in range(S):
        assert _rel(fwd[s], ref[s].detach().numpy()) <= 1e-12
        assert _rel(gp[s], grads[2 + s].numpy()) <= 1e-12
    assert _rel(gT, grads[0].numpy()) <= 1e-12
    assert _rel(gtr, grads[1].numpy()) <= 1e-12


def _ratios(c, J, S):
    """max err / (u * magnitude) of the float32 oracle against float64 for the forward, the point gradients and the two
    sums, each with its K."""
    V = c['points'][0].shape[0]
    f32 = {k: (v if k == 'idx' else [np.asarray(x, np.float32) for x in v] if isinstance(v, list)
               else None if v is None else np.asarray(v, np.float32)) for k, v in c.items()}
    fwd32, (gp32, gT32, gtr32), Rinv32 = _oracle(f32, np.float32)
    # float64 evaluation of the same fp32 inputs (Rinv: the fp32 one both use)
    up = lambda a: None if a is None else np.asarray(a, np.float64)      # noqa: E731
    fwd64 = so.forward([up(p) for p in f32['points']], up(f32['T']), up(f32['weights']), c['idx'], up(f32['trans']),
                       up(Rinv32), up(f32['t']), np.float64)
    gp64, gT64, gtr64 = so.backward([up(p) for p in f32['points']], [up(g) for g in f32['grads']], up(f32['T']),
                                    up(f32['weights']), c['idx'], up(Rinv32), np.float64)
    mf, mgp, mT, mtr = so.magnitudes(f32['points'], f32['grads'], f32['T'], f32['weights'], c['idx'], f32['trans'],
                                     Rinv32, f32['t'])
    out = []
    for a, b, m, K in ([(fwd32[s], fwd64[s], mf[s], so.k_forward(J)) for s in range(S)] +
                       [(gp32[s], gp64[s], mgp[s], so.k_grad_points(J)) for s in range(S)] +
                       [(gT32, gT64, mT, so.k_grad_sums(V, S)), (gtr32, gtr64, mtr, so.k_grad_sums(V, S))]):
        err = np.abs(a.astype(np.float64) - b)
        assert np.all(err <= K * so.U * m + 1e-30), 'outside the first-order bound'
        out.append((float((err / (so.U * m + 1e-300)).max()), K))
    return out


@pytest.mark.parametrize('V,Vw,J,S,use_idx,cam,sparse,rigid', [(5000, 1500, 55, 2, True, True, True, True),
                                                              (3000, 3000, 64, 4, False, True, False, False),
                                                              (700, 700, 1, 1, False, False, False, False),
                                                              (2000, 300, 24, 3, True, False, False, True)])
def test_float32_oracle_is_within_its_bound_with_a_factor_two_to_spare(V, Vw, J, S, use_idx, cam, sparse, rigid):
    c = _case(V, Vw, J, S, seed=V * 3 + J, use_idx=use_idx, cam=cam, sparse=sparse, rigid=rigid)
    for ratio, K in _ratios(c, J, S):
        assert ratio <= K / 2, (ratio, K)


def test_known_answers():
    rng = np.random.default_rng(1)
    V, J = 300, 5
    x = rng.standard_normal((V, 3)).astype(np.float32)
    trans = rng.standard_normal(3).astype(np.float32)
    eye = np.tile(np.eye(4, dtype=np.float32), (J, 1, 1))
    # identity T with weights that sum to 1 exactly (dyadic) -> points + trans, bit for bit
    W = np.zeros((V, J), np.float32)
    W[:, 0], W[:, 2], W[:, 4] = 0.5, 0.25, 0.25
    out = so.forward([x], eye, W, None, trans)[0]
    assert np.array_equal(out, x + trans)
    # one-hot weights -> exactly that joint's transform, for every joint
    T = rng.standard_normal((J, 4, 4)).astype(np.float32)
    idx = rng.integers(0, J, V)
    onehot = np.eye(J, dtype=np.float32)
    A = so.blend(so.gather_weights(onehot, idx, V), T)
    assert np.array_equal(A, T[idx, :3, :])
    out = so.forward([x], T, onehot, idx, trans)[0]
    Tj = T[idx]
    want = np.stack([(((Tj[:, r, 0] * x[:, 0] + Tj[:, r, 1] * x[:, 1]) + Tj[:, r, 2] * x[:, 2]) + Tj[:, r, 3]) + trans[r]
                     for r in range(3)], 1)
    assert np.array_equal(out, want)
    # a pure translation: T = [I | d] -> (x + d) + trans; grad_x = g, grad_trans = sum g, grad_T[j, :3, 3] = sum_v w g
    d = rng.standard_normal((J, 3)).astype(np.float32)
    Tt = eye.copy()
    Tt[:, :3, 3] = d
    out = so.forward([x], Tt, onehot, idx, trans)[0]
    assert np.array_equal(out, (x + d[idx]) + trans)
    g = rng.standard_normal((V, 3)).astype(np.float32)
    gp, gT, gtr = so.backward([x], [g], Tt, onehot, idx, None, np.float64)
    assert np.array_equal(gp[0], g.astype(np.float64))
    assert np.allclose(gtr, g.astype(np.float64).sum(0), rtol=0, atol=1e-12)
    for j in range(J):
        assert np.allclose(gT[j, :3, 3], g[idx == j].astype(np.float64).sum(0), rtol=0, atol=1e-12)
        assert np.all(gT[j, 3] == 0)


def test_out_of_range_indices_give_nan_and_zero_weights_keep_nan_of_inf():
    rng = np.random.default_rng(2)
    V, Vw, J = 40, 10, 6
    W = rng.random((Vw, J)).astype(np.float32)
    idx = rng.integers(0, Vw, V)
    idx[[3, 17]] = [-1, Vw]
    T = rng.standard_normal((J, 4, 4)).astype(np.float32)
    x = rng.standard_normal((V, 3)).astype(np.float32)
    out = so.forward([x], T, W, idx)[0]
    bad = np.isnan(out).any(1)
    assert bad[3] and bad[17] and bad.sum() == 2
    _, gT, _ = so.backward([x], [np.ones((V, 3), np.float32)], T, W, idx)
    assert np.isnan(gT[:, :3]).all() and not gT[:, 3].any()
    # a zero weight on an infinite transform entry: 0 * inf = NaN, as the dense matmul gives
    W0 = np.zeros((Vw, J), np.float32)
    W0[:, 0] = 1
    Ti = T.copy()
    Ti[1, 0, 0] = np.inf
    out = so.forward([x], Ti, W0, idx.clip(0, Vw - 1))[0]
    assert np.isnan(out[:, 0]).all() and not np.isnan(out[:, 1:]).any()


def test_chunked_sum_is_the_sequential_sum_up_to_one_chunk():
    rng = np.random.default_rng(3)
    for V in (1, 255, 256):
        a = rng.standard_normal((V, 5)).astype(np.float32)
        seq = np.zeros(5, np.float32)
        for v in range(V):
            seq = seq + a[v]
        assert np.array_equal(so.chunked_sum(a), seq)
    a = rng.standard_normal((1000, 7)).astype(np.float32)
    parts = [np.zeros(7, np.float32) for _ in range(4)]
    for v in range(1000):
        parts[v // 256] = parts[v // 256] + a[v]
    want = np.zeros(7, np.float32)
    for p in parts:
        want = want + p
    assert np.array_equal(so.chunked_sum(a), want)
