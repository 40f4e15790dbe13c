"""tests/fit_oracle.py against the reference's own run of its classes (tests/golden/ref_fit_terms.npz, written by
tests/golden/make_golden_fit.py): the float32 forwards within the bounds the oracle file derives from the sums whose order
the reference leaves to torch -- and, for the symmetry term, BIT-EQUAL: torch adds its three products in the header's order
(found by this run; for the other three terms torch's order differs or sin / cos do, and equality is only printed) -- and the
oracle's error against the float64 run at most 4x the reference's own float32 error -- forwards and gradients, the
gradients without the elements whose sign decision lies within 1e-5 relative of zero in float64 (at most 1 % of them;
exact ties stay and must give 0)."""
import os

import numpy as np
import pytest

from tests import fit_oracle as fo

FACTOR = 4.0


@pytest.fixture(scope='module')
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, 'ref_fit_terms.npz')))


def oracle(name, g, dtype):
    """(loss, gradient, bound on |loss32 - reference32|, ambiguous-element mask shaped like the gradient)."""
    p = lambda k: g['%s_%s' % (name, k)]      # noqa: E731
    if name == 'edge':
        a = (p('out'), p('gt'), p('valid').reshape(1, -1), p('face'))
        amb = np.broadcast_to(fo.edge_ambiguous(*a[:2], a[3])[..., None], p('out').shape)
        return fo.edge_forward(*a, dtype=dtype), fo.edge_backward(*a, p('g'), dtype=dtype), fo.edge_bound(*a), amb
    if name == 'sym':
        taps, w, _, _ = fo.flip_plan(int(p('vertex_num')), p('face_vertex_idx'), p('closest_faces'), p('bc'))
        amb = np.broadcast_to(fo.sym_ambiguous(p('p'), taps, w)[..., None], p('p').shape)
        return (fo.sym_forward(p('p'), taps, w, dtype), fo.sym_backward(p('p'), taps, w, p('g'), dtype),
                fo.sym_bound(p('p'), taps, w), amb)
    if name == 'pose':
        B = p('out').shape[0]
        amb = np.broadcast_to(fo.pose_ambiguous(p('out'), p('gt')).reshape(B, -1, 1), (B, p('out').shape[1] // 3, 3))
        return (fo.pose_forward(p('out'), p('gt'), dtype).reshape(B, -1, 3, 3),
                fo.pose_backward(p('out'), p('gt'), p('g'), dtype).reshape(B, -1), fo.POSE_K * fo.U, amb.reshape(B, -1))
    a = (p('out'), p('target'), p('weight'))
    return (fo.v2v_forward(*a, dtype=dtype), fo.v2v_backward(*a, p('g'), dtype=dtype), fo.v2v_bound(*a),
            fo.v2v_ambiguous(*a[:2]))


BIT_EQUAL_MAPS = ('sym',)      # the terms whose map coincides with the reference's float32 run bit for bit


def meets_the_bar(e, e_ref):
    """The project's standing bar: at most 4x the reference's own float32 error against its float64 run."""
    return e_ref > 0 and e <= FACTOR * e_ref


@pytest.mark.parametrize('name', ['edge', 'sym', 'pose', 'v2v'])
def test_the_oracle_meets_the_references_own_run(golden, name):
    ref32, ref64 = golden[name + '_loss32'], golden[name + '_loss64']
    gref32, gref64 = golden[name + '_grad32'], golden[name + '_grad64']
    loss, grad, bound, amb = oracle(name, golden, np.float32)
    loss64, grad64, _, _ = oracle(name, golden, np.float64)
    assert loss.dtype == grad.dtype == np.float32 and loss.shape == ref32.shape and grad.shape == gref32.shape
    # the float64 oracle is the float64 reference (the semantics agree; orders do not matter at this precision)
    assert np.abs(loss64 - ref64).max() <= 1e-12 * max(1.0, np.abs(ref64).max())
    # float32 against float32: the derived bound
    diff = np.abs(loss.astype(np.float64) - ref32.astype(np.float64))
    print('%s: map bit-equal to the reference float32 run: %s; worst |diff| / bound %.3f' % (
        name, np.array_equal(loss, ref32), float((diff / np.maximum(bound, 1e-300)).max()) if diff.max() else 0.0))
    assert (diff <= bound).all(), 'worst excess %g' % float((diff - bound).max())
    if name in BIT_EQUAL_MAPS:
        assert np.array_equal(loss.view(np.int32), ref32.view(np.int32)), name + ': the map is the reference float32 run bit for bit'
    # against float64: the standing bar
    e, e_ref = np.abs(loss - ref64).max(), np.abs(ref32 - ref64).max()
    print('%s: map error / reference error %.2f (%.3e / %.3e)' % (name, e / max(e_ref, 1e-300), e, e_ref))
    assert meets_the_bar(e, e_ref), (e, e_ref)
    # gradients: the share of ambiguous elements, then the same bar on the rest
    share = amb.mean()
    assert share <= 0.01, 'share of elements with an ambiguous sign decision %.4f' % share
    keep = ~amb
    assert np.abs(grad64 - gref64)[keep].max() <= 1e-9 * np.abs(gref64).max()
    ge, ge_ref = np.abs(grad - gref64)[keep].max(), np.abs(gref32 - gref64)[keep].max()
    print('%s: gradient error / reference error %.2f (%.3e / %.3e), ambiguous share %.4f' % (
        name, ge / max(ge_ref, 1e-300), ge, ge_ref, share))
    assert np.isfinite(grad).all() and meets_the_bar(ge, ge_ref), (ge, ge_ref)


def test_exact_ties_give_zero(golden):
    g = golden
    face = g['edge_face']
    a, b = face[0, 0], face[0, 1]
    assert np.array_equal(g['edge_out'][:, [a, b]], g['edge_gt'][:, [a, b]])
    loss = fo.edge_forward(g['edge_out'], g['edge_gt'], g['edge_valid'].reshape(1, -1), face)
    assert (loss[:, 0, 0] == 0).all() and (g['edge_loss32'][:, 0, 0] == 0).all()
    # the tied edge sends nothing: the gradient is the same with its cotangent changed
    g2 = g['edge_g'].copy()
    g2[:, 0] = 1e6
    args = (g['edge_out'], g['edge_gt'], g['edge_valid'].reshape(1, -1), face)
    assert np.array_equal(fo.edge_backward(*args, g['edge_g']), fo.edge_backward(*args, g2))
    taps, w, _, _ = fo.flip_plan(int(g['sym_vertex_num']), g['sym_face_vertex_idx'], g['sym_closest_faces'], g['sym_bc'])
    assert (taps[0] == -1).all() and not g['sym_p'][:, 0].any()
    assert (fo.sym_forward(g['sym_p'], taps, w)[:, 0] == 0).all()
    g2 = g['sym_g'].copy()
    g2[:, 0] = 1e6
    assert np.array_equal(fo.sym_backward(g['sym_p'], taps, w, g['sym_g']), fo.sym_backward(g['sym_p'], taps, w, g2))
    assert np.array_equal(g['pose_out'].reshape(-1, 3)[3], g['pose_gt'].reshape(-1, 3)[3])
    assert not fo.pose_backward(g['pose_out'], g['pose_gt'], g['pose_g'])[3].any()


def test_a_zero_length_edge_contributes_nothing_where_the_reference_gives_nan():
    import torch
    c = fo.edge_case(3, 1, 6, 0, face=[[0, 1, 2], [3, 3, 4], [2, 4, 5]])
    c['out'][:, 5] = c['out'][:, 2]                              # a coincident pair: edge (2, 5) of face 2 has length 0
    grad = fo.edge_backward(c['out'], c['gt'], np.ones((1, 6), np.float32), c['face'], c['g'])
    assert np.isfinite(grad).all()
    x = torch.from_numpy(c['out']).requires_grad_(True)
    f = torch.from_numpy(c['face'])
    d = torch.sqrt(torch.sum((x[:, f[:, 0]] - x[:, f[:, 1]]) ** 2, 2))        # the reference's line for the (v0, v1) edges
    (gx,) = torch.autograd.grad(d.sum(), x)
    assert torch.isnan(gx[0, 3]).all(), 'the reference: NaN at the repeated vertex'
    # without the degenerate edges the gradient is unchanged: they contributed exactly 0
    g = c['g'].copy().reshape(1, 3, 3)
    g[0, 0, 1] = 0                                              # edge (3, 3)
    g[0, 1, 2] = 0                                              # edge (2, 5)
    assert np.array_equal(grad, fo.edge_backward(c['out'], c['gt'], np.ones((1, 6), np.float32), c['face'], g.reshape(1, 9, 1)))


def test_the_oracles_transpose_and_rank_order():
    off, ent = fo.transpose(np.array([[1, 1, 2], [0, -1, 2], [2, -1, 1]]), 3)
    assert off.tolist() == [0, 1, 4, 7] and ent.tolist() == [3, 0, 1, 8, 2, 5, 6]
    # float32 addition is not associative: the rank order is each target's own slot order
    big = np.float32(2.0 ** 24)
    acc = fo.add_by_rank(np.zeros((1, 2), np.float32), np.array([0, 0, 0, 1]), np.array([[big, 1, -big, 5]], np.float32))
    assert acc.tolist() == [[0.0, 5.0]]
    acc = fo.add_by_rank(np.zeros((1, 2), np.float32), np.array([0, 0, 0, 1]), np.array([[big, -big, 1, 5]], np.float32))
    assert acc.tolist() == [[1.0, 5.0]]


def test_the_means_of_the_centred_term_stay_within_the_depth_bound():
    for V in (1, 255, 257, 5023):
        c = fo.v2v_case(V, 3, V)
        m32 = fo.v2v_means(c['out'], c['target']).astype(np.float64)
        m64 = np.concatenate([c['out'].astype(np.float64).mean(1), c['target'].astype(np.float64).mean(1)], 1)
        mag = np.concatenate([np.abs(c['out']).astype(np.float64).mean(1), np.abs(c['target']).astype(np.float64).mean(1)], 1)
        assert (np.abs(m32 - m64) <= (fo.v2v_depth(V) + 2) * fo.U * mag).all()
