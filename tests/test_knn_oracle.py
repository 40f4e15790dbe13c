"""CPU checks of tests/knn_oracle.py, the numpy statement of knn_points' semantics the HIP search is held to bit for bit:
known answers, exact ties, and agreement with the PyTorch stand-in on tie-free data."""
import numpy as np
import torch

from exavatar_release_amd import p3d_standins as p3d
from tests import knn_oracle as ko


def test_known_answer():
    p2 = np.array([[[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3]]], dtype=np.float32)
    p1 = np.array([[[0.9, 0, 0], [0, 0, 2.9]]], dtype=np.float32)
    d, i = ko.knn(p1, p2, 3)
    assert i.tolist() == [[[1, 0, 2], [3, 0, 1]]]
    dx = np.float32(0.9) - np.float32(1.0)
    assert d[0, 0, 0] == dx * dx
    assert d[0, 1, 1] == np.float32(2.9) * np.float32(2.9)


def test_distance_is_spelled_out_in_fp32():
    # (dx*dx + dy*dy) + dz*dz in float32, not a float64 sum rounded once
    a = np.array([[0.1, 0.2, 0.3]], dtype=np.float32)
    b = np.array([[0.7, -0.4, 1.9]], dtype=np.float32)
    d = ko.sq_dists(a, b)[0, 0]
    dx, dy, dz = a[0] - b[0]
    assert d == np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(dz * dz)


def test_k_is_clamped_to_p2():
    d, i = ko.knn(np.zeros((2, 5, 3)), np.ones((2, 3, 3)), 8)
    assert d.shape == (2, 5, 3) and i.shape == (2, 5, 3)
    assert i[0, 0].tolist() == [0, 1, 2]


def test_duplicated_points_tie_to_the_lower_index():
    p2 = np.array([[[1, 1, 1], [0, 0, 0], [1, 1, 1], [0, 0, 0], [1, 1, 1]]], dtype=np.float32)
    d, i = ko.knn(np.zeros((1, 1, 3), np.float32), p2, 5)
    assert i[0, 0].tolist() == [1, 3, 0, 2, 4]
    assert d[0, 0].tolist() == [0, 0, 3, 3, 3]


def test_equidistant_lattice_points_tie_to_the_lower_index():
    g = np.stack(np.meshgrid(*[np.arange(-2, 3, dtype=np.float32)] * 3, indexing='ij'), -1).reshape(1, -1, 3)
    rng = np.random.default_rng(0)
    p2 = g[:, rng.permutation(g.shape[1])]
    d, i = ko.knn(np.zeros((1, 1, 3), np.float32), p2, 7)
    # the centre, then its six face neighbours at distance 1 in ascending index order
    assert d[0, 0].tolist() == [0] + [1] * 6
    face = sorted(np.nonzero((p2[0] ** 2).sum(1) == 1)[0].tolist())
    assert i[0, 0, 1:].tolist() == face
    assert np.array_equal(ko.knn_small_k(np.zeros((1, 1, 3), np.float32), p2, 7)[1], i)


def test_agrees_with_the_stand_in_on_tie_free_data():
    g = torch.Generator().manual_seed(3)
    a = torch.randn(2, 300, 3, generator=g)
    b = torch.randn(2, 500, 3, generator=g)
    for K in (1, 4, 9):
        ref = p3d.knn_points(a, b, K=K)
        d, i = ko.knn(a.numpy(), b.numpy(), K)
        assert np.array_equal(i, ref.idx.numpy())
        assert np.allclose(d, ref.dists.numpy(), rtol=1e-5, atol=1e-6)


def test_fast_variants_agree_with_the_full_sort():
    rng = np.random.default_rng(1)
    a = rng.standard_normal((2, 200, 3)).astype(np.float32)
    b = np.round(rng.standard_normal((2, 150, 3)) * 4).astype(np.float32) / 4     # many exact ties
    b[:, 100:] = b[:, :50]
    d1, i1 = ko.knn(a, b, 1)
    d2, i2 = ko.knn_nearest(a, b)
    assert np.array_equal(i1, i2) and np.array_equal(d1, d2)
    for K in (3, 8):
        d1, i1 = ko.knn(a, b, K)
        d2, i2 = ko.knn_small_k(a, b, K)
        assert np.array_equal(i1, i2) and np.array_equal(d1, d2)
