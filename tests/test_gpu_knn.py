"""The HIP knn_points (exavatar_release_amd.knn) against the numpy oracle tests/knn_oracle.py, run on the GPU.

``idx`` and ``dists`` must equal the oracle BIT FOR BIT, with culling on and off: the semantics (lexicographic (d, j),
d rounded operation by operation in fp32) leave no freedom.  Gradients are compared with the PyTorch stand-in's
autograd (allclose: a different summation order) and must repeat bit for bit from call to call."""
import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import p3d_standins as p3d
from exavatar_release_amd import scenes
from tests import knn_oracle as ko

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def _run(p1, p2, K, cull, **kw):
    exa.config.knn_cull = cull
    return exa.knn_points(p1.to(DEV), p2.to(DEV), K=K, **kw)


def _oracle(p1, p2, K):
    a, b = p1.cpu().numpy(), p2.cpu().numpy()
    if K == 1 and a.shape[1] * b.shape[1] > 1e7:
        return ko.knn_nearest(a, b)
    if a.shape[1] * b.shape[1] > 1e7:
        return ko.knn_small_k(a, b, K)
    return ko.knn(a, b, K)


def _check(p1, p2, K, oracle=None):
    """Both search modes equal the oracle bit for bit; returns the culled result."""
    d_ref, i_ref = oracle if oracle is not None else _oracle(p1, p2, K)
    out = None
    for cull in (True, False):
        r = _run(p1, p2, K, cull)
        i, d = r.idx.cpu().numpy(), r.dists.detach().cpu().numpy()
        assert i.dtype == np.int64
        assert i.shape == i_ref.shape and d.shape == d_ref.shape
        bad = np.nonzero((i != i_ref).any(-1))
        assert bad[0].size == 0, 'cull=%s: %d queries differ in idx, first %s' % (cull, bad[0].size, [x[:3] for x in bad])
        assert np.array_equal(d.view(np.uint32), d_ref.view(np.uint32)), 'cull=%s: dists differ' % cull
        if cull:
            out = r
    return out


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize('K', [1, 2, 3, 4, 5, 8, 16, 32])
def test_random_normal_every_k(K):
    # N = 3, P2 not a multiple of 64
    _check(_randn(3, 1000, 3, seed=K), _randn(3, 777, 3, seed=100 + K), K)


def test_reference_shape_k1_avatar_surface():
    """module.py:543: 167 000 offset Gaussian centres against 10 475 template vertices of the same surface."""
    refs = scenes.dist_b_avatar(10475, seed=1)['mean_3d']
    q = scenes.dist_b_avatar(167000, seed=2)['mean_3d'] + 0.005 * _randn(167000, 3, seed=3)
    _check(q[None], refs[None], 1)


def test_reference_shape_k4_self_query():
    """module.py:86: a K = 4 self-query on a scattered point cloud.  Neighbour 0 is the point itself at distance 0; the
    culled search equals the brute force everywhere and the oracle on a sample of queries (the full oracle is 4e10
    pairs of numpy)."""
    P = 200000
    g = torch.Generator().manual_seed(5)
    xyz = torch.cat([torch.randn(P // 2, 3, generator=g) * 2, torch.rand(P - P // 2, 3, generator=g) * 8 - 4])
    xyz = xyz[torch.randperm(P, generator=g)].contiguous()
    on = _run(xyz[None], xyz[None], 4, True)
    off = _run(xyz[None], xyz[None], 4, False)
    assert torch.equal(on.idx, off.idx)
    assert torch.equal(on.dists.view(torch.int32), off.dists.view(torch.int32))
    idx, d = on.idx.cpu(), on.dists.cpu()
    assert torch.equal(idx[0, :, 0], torch.arange(P)), 'a point is its own nearest neighbour (no exact duplicates here)'
    assert bool((d[0, :, 0] == 0).all())
    sample = torch.randperm(P, generator=g)[:2048]
    d_ref, i_ref = ko.knn_small_k(xyz[sample][None].numpy(), xyz[None].numpy(), 4)
    assert np.array_equal(idx[0, sample].numpy(), i_ref[0])
    assert np.array_equal(d[0, sample].numpy().view(np.uint32), d_ref[0].view(np.uint32))


def test_empty_and_small_shapes_match_the_stand_in():
    for N, P1, P2, K in ((2, 50, 3, 5), (2, 0, 40, 4), (2, 30, 0, 4), (0, 30, 40, 4), (1, 1, 1, 1), (1, 7, 64, 32)):
        a, b = _randn(N, P1, 3, seed=1), _randn(N, P2, 3, seed=2)
        ref = p3d.knn_points(a, b, K=K, return_nn=True)
        for cull in (True, False):
            out = _run(a, b, K, cull, return_nn=True)
            assert out.dists.shape == ref.dists.shape and out.idx.shape == ref.idx.shape
            assert out.knn.shape == ref.knn.shape
            assert out.idx.dtype == torch.int64
            if out.idx.numel():
                assert torch.equal(out.idx.cpu(), ref.idx)
        if N * P1 * min(K, P2):
            _check(a, b, K)


def test_duplicates_and_lattices_tie_to_the_lower_index():
    g = torch.stack(torch.meshgrid(*[torch.arange(-4.0, 5.0)] * 3, indexing='ij'), -1).reshape(-1, 3)   # 729 points
    perm = torch.randperm(g.shape[0], generator=torch.Generator().manual_seed(0))
    lattice = torch.cat([g[perm], g[perm[:200]], g[perm[:100]]])       # exact duplicates at higher indices
    q = torch.cat([g, g + 0.5, g[:300] * 0.5])                         # lattice points and equidistant centres
    for K in (1, 4, 8, 27):
        _check(q[None], lattice[None], K)


def test_dense_cluster_with_far_outliers():
    cl = _randn(4000, 3, seed=7) * 1e-3
    far = _randn(40, 3, seed=8) * 1e4
    pts = torch.cat([cl, far])[torch.randperm(4040, generator=torch.Generator().manual_seed(9))]
    q = torch.cat([_randn(500, 3, seed=10) * 1e-3, _randn(20, 3, seed=11) * 1e4])
    for K in (1, 4, 16):
        _check(q[None], pts[None], K)


def test_offset_far_from_the_origin():
    _check(_randn(2, 3000, 3, seed=12) + 1000.0, _randn(2, 2500, 3, seed=13) + 1000.0, 4)


def test_tiny_separations():
    base = _randn(1, 500, 3, seed=14)
    p2 = torch.cat([base, base + 1e-6, base - 1e-6 * torch.tensor([1.0, -1.0, 0.5])], 1)
    q = base + 5e-7
    for K in (1, 3, 6):
        _check(q, p2, K)


def test_permuting_queries_permutes_the_outputs_and_relabelling_refs_relabels_idx():
    a, b = _randn(1, 3000, 3, seed=15), _randn(1, 2000, 3, seed=16)
    g = torch.Generator().manual_seed(17)
    pa, pb = torch.randperm(3000, generator=g), torch.randperm(2000, generator=g)
    base = _run(a, b, 8, True)
    qp = _run(a[:, pa], b, 8, True)
    assert torch.equal(qp.idx, base.idx[:, pa.to(DEV)])
    assert torch.equal(qp.dists, base.dists[:, pa.to(DEV)])
    rp = _run(a, b[:, pb], 8, True)                  # ref r of the relabelled set is old ref pb[r]
    assert torch.equal(pb.to(DEV)[rp.idx], base.idx)
    assert torch.equal(rp.dists, base.dists)


def _grads(a, b, K, weights, cull=True, standin=False):
    exa.config.knn_cull = cull
    a = a.clone().requires_grad_(True)
    b = b.clone().requires_grad_(True)
    out = (p3d.knn_points if standin else exa.knn_points)(a, b, K=K, return_nn=True)
    loss = out.dists.sum() + (out.knn * weights).sum()
    loss.backward()
    return out, a.grad, b.grad


def test_gradients_match_the_stand_in_and_repeat_bit_for_bit():
    a, b = _randn(2, 2000, 3, seed=18).to(DEV), _randn(2, 300, 3, seed=19).to(DEV)   # many queries per ref
    for K in (1, 4):
        w = _randn(2, 2000, K, 3, seed=20 + K).to(DEV)
        out, ga, gb = _grads(a, b, K, w)
        ref, ra, rb = _grads(a, b, K, w, standin=True)
        assert torch.equal(out.idx, ref.idx)
        assert torch.allclose(ga, ra, rtol=1e-5, atol=1e-5)
        assert torch.allclose(gb, rb, rtol=1e-4, atol=1e-4)
        out2, ga2, gb2 = _grads(a, b, K, w)
        assert torch.equal(ga.view(torch.int32), ga2.view(torch.int32))
        assert torch.equal(gb.view(torch.int32), gb2.view(torch.int32))
        assert torch.equal(out.dists.view(torch.int32), out2.dists.view(torch.int32))
        # each output on its own
        for which in ('dists', 'knn'):
            a1, b1 = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
            a2, b2 = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
            o1 = exa.knn_points(a1, b1, K=K, return_nn=True)
            o2 = p3d.knn_points(a2, b2, K=K, return_nn=True)
            (o1.dists.sum() if which == 'dists' else (o1.knn * w).sum()).backward()
            (o2.dists.sum() if which == 'dists' else (o2.knn * w).sum()).backward()
            assert torch.allclose(b1.grad, b2.grad, rtol=1e-4, atol=1e-4), which
            if which == 'dists':
                assert torch.allclose(a1.grad, a2.grad, rtol=1e-5, atol=1e-5)
            else:
                assert a1.grad is None or not bool(a1.grad.any())


def test_repeat_calls_and_poisoned_workspace_give_the_same_bits():
    a, b = _randn(2, 5000, 3, seed=21), _randn(2, 3000, 3, seed=22)
    r1 = _run(a, b, 5, True)
    r2 = _run(a, b, 5, True)
    exa.config.poison = True
    r3 = _run(a, b, 5, True)
    for r in (r2, r3):
        assert torch.equal(r.idx, r1.idx)
        assert torch.equal(r.dists.view(torch.int32), r1.dists.view(torch.int32))


def test_reference_expressions_run_as_written():
    from exavatar_release_amd import knn_points
    # module.py:86-87: scene Gaussian scales from the three nearest other points
    xyz = (_randn(20000, 3, seed=23) * 3).to(DEV)
    points = knn_points(xyz[None, :, :], xyz[None, :, :], K=4, return_nn=True)
    dist = torch.sum((xyz[:, None, :] - points.knn[0, :, 1:, :]) ** 2, 2).mean(1)
    ref = p3d.knn_points(xyz[None, :, :], xyz[None, :, :], K=4, return_nn=True)
    dref = torch.sum((xyz[:, None, :] - ref.knn[0, :, 1:, :]) ** 2, 2).mean(1)
    assert dist.shape == (20000,) and torch.allclose(dist, dref, rtol=1e-6, atol=0)
    # module.py:543: nearest template vertex of every Gaussian centre
    mesh = scenes.dist_b_avatar(10475, seed=4)['mean_3d'].to(DEV)
    mean_3d = mesh.repeat(4, 1)[:40000] + 0.003 * _randn(40000, 3, seed=24).to(DEV)
    nn_vertex_idxs = knn_points(mean_3d[None, :, :], mesh[None, :, :], K=1, return_nn=True).idx[0, :, 0]
    assert nn_vertex_idxs.shape == (40000,) and nn_vertex_idxs.dtype == torch.int64
    d_ref, i_ref = ko.knn_nearest(mean_3d[None].cpu().numpy(), mesh[None].cpu().numpy())
    assert np.array_equal(nn_vertex_idxs.cpu().numpy(), i_ref[0, :, 0])


def test_graph_capture_replays_with_new_points():
    a, b = _randn(1, 20000, 3, seed=25).to(DEV), _randn(1, 6000, 3, seed=26).to(DEV)
    a2, b2 = _randn(1, 20000, 3, seed=27).to(DEV), _randn(1, 6000, 3, seed=28).to(DEV)
    sa, sb = a.clone(), b.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        exa.knn_points(sa, sb, K=4, return_nn=True)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = exa.knn_points(sa, sb, K=4, return_nn=True)
    sa.copy_(a2)
    sb.copy_(b2)
    graph.replay()
    torch.cuda.synchronize()
    ref = exa.knn_points(a2, b2, K=4, return_nn=True)
    assert torch.equal(out.idx, ref.idx)
    assert torch.equal(out.dists.view(torch.int32), ref.dists.view(torch.int32))
    assert torch.equal(out.knn, ref.knn)
