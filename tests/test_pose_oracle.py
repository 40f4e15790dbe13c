"""CPU tests of tests/pose_oracle.py, the numpy restatement that pins the pose-parameter kernels: in float64 its forward
and its hand-written backward equal the reference's expression -- ``matrix_to_axis_angle(rotation_6d_to_matrix(p))`` by
the stand-ins -- and that expression's autograd to 1e-12 relative, on 4096 random rotations pushed 0.05 off the manifold
and on the special rows; they equal the fixture recorded from the reference's own class within the same bound; the
float32 and the float64 run take the same discrete decisions on every row the GPU tests compare across precisions."""
import os

import numpy as np
import pytest

from tests import pose_oracle as po

REL = 1e-12
R = 4096


@pytest.fixture(scope='module')
def rows():
    d6, g = po.random_rows(R, seed=3)
    return d6, g


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'ref_pose.npz'))


def _close(a, b, what):
    scale = np.abs(b).max()
    assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all(), what
    assert np.abs(a - b).max() <= REL * max(scale, 1e-300), '%s: %.3e relative' % (what, np.abs(a - b).max() / scale)


def test_float64_equals_the_standin_expression_and_its_autograd_on_random_rows(rows):
    d6, g = rows
    want, gwant = po.standin(d6, g, np.float64)
    aa, _ = po.forward(d6, np.float64)
    _close(aa, want, 'axis-angle')
    _close(po.backward(d6, g, np.float64), gwant, 'gradient')


def test_float64_equals_the_standin_on_every_special_row():
    """Row by row: the degenerate rows' gradients are 1 / eps larger than the others', and each is held to its own
    scale."""
    d6 = po.special_rows()
    rng = np.random.default_rng(5)
    for g in (np.ones((len(d6), 3)), rng.standard_normal((len(d6), 3))):
        want, gwant = po.standin(d6, g, np.float64)
        aa, _ = po.forward(d6, np.float64)
        got = po.backward(d6, g, np.float64)
        for r in range(len(d6)):
            _close(aa[r], want[r], 'axis-angle of special row %d' % r)
            _close(got[r], gwant[r], 'gradient of special row %d' % r)


def test_the_identity_row_gets_the_stated_finite_gradient():
    for dtype in (np.float32, np.float64):
        got = po.backward(np.array([[1, 0, 0, 0, 1, 0]]), np.ones((1, 3)), dtype)
        assert np.array_equal(got, np.array([[0, -1, 1, 0, 0, -1]], dtype=dtype))
        assert np.array_equal(po.standin(np.array([[1, 0, 0, 0, 1, 0]]), np.ones((1, 3)), dtype)[1], got)


def test_special_rows_land_on_both_sides_of_each_branch():
    d6 = po.special_rows()
    i, neg, small = po.decisions(d6, np.float32)
    assert set(i.tolist()) == {0, 1, 2, 3}                       # every candidate
    assert small.any() and not small.all()
    aa, q = po.forward(d6)
    angle = np.linalg.norm(aa.astype(np.float64), axis=1)
    assert ((angle > 0) & (angle < 1e-6)).sum() >= 3 and ((angle > 1e-6) & (angle < 1e-5)).sum() >= 2
    assert (np.abs(angle - np.pi) < 1e-6).sum() >= 6             # the half turns
    assert (q[:, 0] >= 0).all()
    for a, b in zip(po.decisions(d6, np.float32), po.decisions(d6, np.float64)):
        assert np.array_equal(a, b)


def test_float32_and_float64_take_the_same_decisions_on_the_random_rows(rows):
    d6, _ = rows
    for a, b in zip(po.decisions(d6, np.float32), po.decisions(d6, np.float64)):
        assert np.array_equal(a, b)
    i, neg, small = po.decisions(d6)
    assert len(set(i.tolist())) == 4 and not small.any()


def test_float32_is_float64_rounded_within_first_order(rows):
    """The expression is well conditioned on these rows: the float32 run stays within a few 1e-7 of the float64 run."""
    d6, g = rows
    aa32, q32 = po.forward(d6)
    aa64, q64 = po.forward(d6, np.float64)
    assert aa32.dtype == np.float32 and q32.dtype == np.float32
    assert np.abs(q32 - q64).max() <= 16 * po.U and np.abs(aa32 - aa64).max() <= 64 * po.U * np.pi
    g32, g64 = po.backward(d6, g), po.backward(d6, g, np.float64)
    assert g32.dtype == np.float32 and np.abs(g32 - g64).max() <= 64 * po.U * np.abs(g64).max()


def test_equals_the_fixture(golden):
    for f in golden['frames']:
        for n in ('root_pose', 'body_pose', 'jaw_pose', 'leye_pose', 'reye_pose', 'lhand_pose', 'rhand_pose'):
            d6 = golden['init/smplx_params.%d.%s' % (f, n)]
            _close(d6.reshape(-1, 6), po.rotation_6d(golden['raw/%d/%s' % (f, n)]), 'init %d %s' % (f, n))
            aa, _ = po.forward(d6, np.float64)
            want = golden['out/%d/%s' % (f, n)]
            if np.abs(want).max() == 0:
                assert not aa.any()
            else:
                _close(aa.reshape(want.shape), want, 'out %d %s' % (f, n))
            got = po.backward(d6, golden['G/%d/%s' % (f, n)], np.float64)
            _close(got.reshape(d6.shape), golden['grad/%d/%s' % (f, n)], 'grad %d %s' % (f, n))


def test_the_fixture_covers_what_it_says(golden):
    assert list(golden['frames']) == [3, 17]
    assert not golden['raw/3/leye_pose'].any() and not golden['raw/3/reye_pose'].any()
    angle = np.linalg.norm(golden['raw/17/body_pose'], axis=1)
    assert abs(angle[5] - np.pi) < 1e-3 and 0 < angle[9] < 1e-6
    rows = [golden['raw/3/' + n].size // 3 for n in ('root_pose', 'body_pose', 'jaw_pose', 'leye_pose', 'reye_pose',
                                                      'lhand_pose', 'rhand_pose')]
    assert tuple(rows) == po.SEGMENT_ROWS and sum(rows) == 55


def test_split_and_segment_rows():
    a = np.arange(55 * 3).reshape(55, 3)
    parts = po.split(a, po.SEGMENT_ROWS)
    assert [len(p) for p in parts] == list(po.SEGMENT_ROWS) and np.array_equal(np.concatenate(parts), a)
