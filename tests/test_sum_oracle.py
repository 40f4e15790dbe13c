"""tests/sum_oracle.py against the orders written out by hand (CPU only): the oracles of four stages add through it."""
import numpy as np
import pytest

from tests import sum_oracle as so

F32 = np.float32


def _bits(a):
    return np.asarray(a, dtype=F32).view(np.uint32)


def _random(seed, *shape):
    rs = np.random.RandomState(seed)
    # a wide spread of magnitudes and both signs, so that a changed association changes the rounding
    return (rs.standard_normal(shape) * np.exp(3.0 * rs.standard_normal(shape))).astype(F32)


def test_tree_lane0_equals_butterfly_lane0():
    x = _random(0, 37, 64)
    both = so.butterfly(x)
    assert both.dtype == F32 and both.shape == x.shape
    np.testing.assert_array_equal(_bits(so.tree(x)), _bits(both[:, 0]))
    # every lane of the butterfly holds the wave's sum
    np.testing.assert_array_equal(_bits(both), _bits(np.repeat(both[:, :1], 64, axis=1)))
    # and the order is not that of a plain running sum
    running = np.zeros(37, F32)
    for i in range(64):
        running = running + x[:, i]
    assert (_bits(running) != _bits(both[:, 0])).any()


def _wave_by_hand(v):
    """The wave's sum in lane 0, the six steps written out on Python lists of float32."""
    v = [F32(a) for a in v]
    assert len(v) == 64
    for d in (32, 16, 8, 4, 2, 1):
        v = [F32(v[i] + v[i ^ d]) for i in range(64)]
    return v[0]


def test_wg_sum_is_the_four_wave_formula():
    x = _random(1, 256)
    w = [_wave_by_hand(x[64 * k:64 * k + 64]) for k in range(4)]
    expected = F32(F32(F32(w[0] + w[1]) + w[2]) + w[3])
    got = so.wg_sum(x)
    assert got.dtype == F32 and got.shape == ()
    assert _bits(got) == _bits(expected)
    assert _bits(so.waves(np.array(w, F32))) == _bits(expected)
    # batched over leading axes
    np.testing.assert_array_equal(_bits(so.wg_sum(np.stack([x, x[::-1]]))), _bits([got, so.wg_sum(x[::-1].copy())]))
    # the pairing matters: (w0 + w1) + (w2 + w3) differs somewhere on such data
    many = _random(2, 200, 256)
    ws = so.butterfly(many.reshape(200, 4, 64))[..., 0]
    paired = (ws[:, 0] + ws[:, 1]) + (ws[:, 2] + ws[:, 3])
    assert (_bits(paired) != _bits(so.wg_sum(many))).any()


@pytest.mark.parametrize('n', [257, 513])
def test_strided_sum_is_the_loop(n):
    x = _random(3, n)
    expected = []
    for t in range(256):
        s = F32(0.0)
        j = t
        while j < n:
            s = F32(s + x[j])
            j += 256
        expected.append(s)
    got = so.strided_sum(x)
    assert got.dtype == F32 and got.shape == (256,)
    np.testing.assert_array_equal(_bits(got), _bits(expected))


def test_strided_sum_keeps_the_sign_of_an_untouched_thread():
    # a thread past the end adds nothing: it stays +0.0, it does not become -0.0 + 0.0 or pick up padding
    x = np.full(3, -0.0, F32)
    got = so.strided_sum(x)
    assert (_bits(got[3:]) == 0).all() and (_bits(got[:3]) == 0).all()      # +0.0 + -0.0 = +0.0
    assert so.strided_sum(np.zeros(0, F32)).shape == (256,)
