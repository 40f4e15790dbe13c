"""CPU tests of the LPIPS oracle (tests/lpips_oracle.py) itself: the properties the definition implies, the tap shapes, the
zero-norm rule, and that the cases of the GPU test keep the float32 oracle inside its own bar."""
import numpy as np
import pytest
import torch

from tests import lpips_case as lc
from tests import lpips_oracle as lo


def _run(out, tgt, bbox=None, dtype=torch.float64):
    convs, lins = lo.as_tensors(*lc.weights(), dtype)
    return lo.lpips(torch.from_numpy(out).to(dtype), torch.from_numpy(tgt).to(dtype), convs, lins, bbox)


def test_identical_images_give_exactly_zero():
    out = lc.image(3, 2, 20, 24)
    for dtype in (torch.float64, torch.float32):
        value, maps = _run(out, out.copy(), dtype=dtype)
        assert tuple(value.shape) == (2, 1, 1, 1) and (value == 0).all() and all((m == 0).all() for m in maps)


def test_pixels_outside_the_bbox_change_nothing():
    B, H, W = 2, 48, 72
    out, tgt = lc.image_pair(9, B, H, W)
    bbox = np.array([lc.BBOX] * B)
    a, maps_a = _run(out, tgt, bbox)
    rng = np.random.RandomState(5)
    out2, tgt2 = rng.uniform(0, 1, out.shape).astype(np.float32), rng.uniform(0, 1, tgt.shape).astype(np.float32)
    out2[:, :, 7:48, 0:60], tgt2[:, :, 7:48, 0:60] = out[:, :, 7:48, 0:60], tgt[:, :, 7:48, 0:60]
    b, maps_b = _run(out2, tgt2, bbox)
    assert torch.equal(a, b) and all(torch.equal(m, n) for m, n in zip(maps_a, maps_b))
    assert tuple(maps_a[0].shape) == (2, 1, 41, 60)
    c, _ = _run(out, tgt, None)
    assert not torch.equal(a, c)


@pytest.mark.parametrize('h,w', [(16, 16), (17, 23)])
def test_the_tap_shapes(h, w):
    convs, _ = lo.as_tensors(*lc.weights(), torch.float32)
    taps = lo.trunk(lo.input_map(torch.from_numpy(lc.image(1, 1, h, w))), convs)
    assert [tuple(t.shape) for t in taps] == [(1, c, h >> b, w >> b) for b, c in enumerate((64, 128, 256, 512, 512))]
    assert all((t >= 0).all() for t in taps)


def test_the_norm_has_a_zero_derivative_at_zero():
    f = torch.rand(1, 8, 2, 2, dtype=torch.float64)
    f[0, :, 0, 0] = 0
    f.requires_grad_(True)
    t = torch.rand(1, 8, 2, 2, dtype=torch.float64)
    value, _ = lo.head([f], [t], [torch.ones(8, dtype=torch.float64)])
    value.sum().backward()
    assert torch.isfinite(f.grad).all()
    want = 2 * (0 - lo.normalize(t)[0, :, 0, 0]) / 4 / 1e-10      # only the direct term u / (0 + eps) is left
    assert torch.allclose(f.grad[0, :, 0, 0], want, rtol=1e-12)


@pytest.mark.parametrize('name', list(lc.CASES))
def test_the_cases_keep_the_float32_oracle_inside_its_own_bar(name):
    B, H, W, bbox, seed = lc.CASES[name]
    out, tgt = lc.image_pair(seed, B, H, W)
    bbox = None if bbox is None else np.array([bbox] * B)
    convs, lins = lc.weights()
    r64 = lo.run(out, tgt, convs, lins, bbox, torch.float64)
    r32 = lo.run(out, tgt, convs, lins, bbox, torch.float32)
    assert lo.relu_decisions_agree(r32, r64)
    assert lo.decision_margin(r64) >= lo.MIN_MARGIN
    lo.check_float32_scalar(r32, r64)
    assert all((m > 0).all() for m in r64['maps'])      # no all-zero tap pixel: the biases are positive
    assert all(np.sqrt((a ** 2).sum(1)).min() > 0 for a in (r64['acts'][l] for l in (1, 3, 6, 9, 12)))
