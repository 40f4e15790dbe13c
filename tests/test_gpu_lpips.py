"""GPU tests of the HIP LPIPS module against the CPU oracle (tests/lpips_oracle.py) in float64, with the oracle's own
float32 run as the yardstick: the HIP run is another float32 evaluation, so each of its errors against float64 -- relative
L2 and norm-scaled max of the five per-pixel maps d_l and of dL/d img_out -- may be at most 4 x the float32 oracle's,
floored at 2^-24; the scalar lies within ``lpips_oracle.scalar_scale(.., k=4)``.  Nothing is skipped in
the gradient: the cases (tests/lpips_case.CASES) were chosen so that the float64 run is ``decision_margin >= MIN_MARGIN``
float32-oracle errors away from every ReLU and pool decision, which is asserted here.

The convolution kernel's tile is TILE x TILE = 16 x 16 pixels (CONV_TILE of csrc/lpips.hip); the 'tiles' case is
2 TILE + 5 = 37 pixels both ways: three tiles with a ragged last one.
"""
import functools

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from tests import lpips_case as lc
from tests import lpips_oracle as lo

pytestmark = pytest.mark.gpu

TILE = 16
FLOOR = 2.0 ** -24
assert lc.CASES['tiles'][1:3] == (2 * TILE + 5, 2 * TILE + 5)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(img_out, img_target, bbox, float64 run, float32 run) of a case, computed once and shared."""
    B, H, W, bbox, seed = lc.CASES[name]
    out, tgt = lc.image_pair(seed, B, H, W)
    bbox = None if bbox is None else np.array([bbox] * B)
    convs, lins = lc.weights()
    r64 = lo.run(out, tgt, convs, lins, bbox, torch.float64)
    r32 = lo.run(out, tgt, convs, lins, bbox, torch.float32)
    return out, tgt, bbox, r64, r32


@pytest.fixture(scope='module')
def module():
    return exa.LPIPS.from_arrays(*lc.weights()).cuda()


def hip_run(module, out, tgt, bbox, maps=True, **kw):
    """value [B], maps, dL/d img_out for L = sum_b value_b, as torch tensors on the host."""
    x = torch.from_numpy(out).cuda().requires_grad_(True)
    bb = None if bbox is None else torch.from_numpy(bbox)
    if 'target' in kw:
        value, d = module(x, None, bbox=bb, target=kw['target'], return_maps=True)
    else:
        value, d = module(x, torch.from_numpy(tgt).cuda(), bbox=bb, return_maps=True)
    assert tuple(value.shape) == (out.shape[0], 1, 1, 1)
    value.sum().backward()
    return value.detach().cpu().reshape(-1), [m.cpu() for m in d], x.grad.cpu()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('name', list(lc.CASES))
def test_maps_scalar_and_gradient_against_float64(module, name):
    out, tgt, bbox, r64, r32 = oracle(name)
    assert lo.decision_margin(r64) >= lo.MIN_MARGIN and lo.relu_decisions_agree(r32, r64)
    lo.check_float32_scalar(r32, r64)
    value, maps, grad = hip_run(module, out, tgt, bbox)
    assert [tuple(m.shape) for m in maps] == [m.shape for m in r64['maps']]
    pairs = [('d%d' % t, maps[t].double().numpy(), r32['maps'][t], r64['maps'][t]) for t in range(5)]
    pairs.append(('grad', grad.double().numpy(), r32['grad'], r64['grad']))
    bad = []
    for what, hip, f32, f64 in pairs:
        for metric in (lo.rel_l2, lo.rel_max):
            mine, ref = metric(hip, f64), max(metric(f32, f64), FLOOR)
            print('%s %s %s: HIP %.3g, float32 oracle %.3g, ratio %.2f' % (name, what, metric.__name__, mine, ref, mine / ref))
            if not mine <= 4 * ref:
                bad.append((what, metric.__name__, mine, ref))
    for b in range(len(value)):
        errs = [m32[b] - m64[b] for m32, m64 in zip(r32['maps'], r64['maps'])]
        scale = lo.scalar_scale(errs, r64['value'][b], r64['maps'][0][b].size, 4)
        diff = abs(float(value[b]) - r64['value'][b])
        print('%s value[%d]: HIP %.9g, float64 %.9g, |diff| %.3g, bound %.3g' % (name, b, value[b], r64['value'][b], diff, scale))
        if not diff <= scale:
            bad.append(('value', b, diff, scale))
    assert not bad, bad


def test_the_gradient_outside_the_crop_is_exactly_zero_with_poisoned_workspaces(module):
    out, tgt, bbox, _, _ = oracle('bbox')
    exa.config.poison = True
    value, maps, grad = hip_run(module, out, tgt, bbox)
    x0, y0, w, h = 0, 7, 60, 41      # the reference's clamp of (-5, 7, 60, 50): xmax = min(0 + 60, 72)
    inside = torch.zeros(grad.shape, dtype=torch.bool)
    inside[:, :, y0:y0 + h, x0:x0 + w] = True
    assert torch.isfinite(value).all() and all(torch.isfinite(m).all() for m in maps)
    assert torch.equal(grad[~inside].view(torch.int32), torch.zeros_like(grad[~inside]).view(torch.int32))      # +0.0, not -0.0
    assert torch.isfinite(grad).all() and (grad[inside] != 0).float().mean() > 0.99


def test_pixels_outside_the_bbox_change_nothing(module):
    out, tgt, bbox, _, _ = oracle('bbox')
    a = hip_run(module, out, tgt, bbox)
    rng = np.random.RandomState(5)
    out2, tgt2 = rng.uniform(0, 1, out.shape).astype(np.float32), rng.uniform(0, 1, tgt.shape).astype(np.float32)
    out2[:, :, 7:48, 0:60], tgt2[:, :, 7:48, 0:60] = out[:, :, 7:48, 0:60], tgt[:, :, 7:48, 0:60]
    b = hip_run(module, out2, tgt2, bbox)
    assert same_bits(a[0], b[0]) and same_bits(a[2], b[2]) and all(same_bits(m, n) for m, n in zip(a[1], b[1]))


def test_identical_images_give_exactly_zero(module):
    out, _, bbox, _, _ = oracle('odd')
    value, maps, grad = hip_run(module, out, out.copy(), bbox)
    assert (value == 0).all() and all((m == 0).all() for m in maps) and (grad == 0).all()


def test_all_zero_taps_give_zero_distance_and_a_finite_zero_gradient():
    module = exa.LPIPS.from_arrays(*lc.zero_weights()).cuda()
    out, tgt, bbox, _, _ = oracle('odd')
    value, maps, grad = hip_run(module, out, tgt, bbox)
    assert (value == 0).all() and all((m == 0).all() for m in maps)
    assert torch.isfinite(grad).all() and (grad == 0).all()


def test_two_calls_give_the_same_bits(module):
    out, tgt, bbox, _, _ = oracle('tiles')
    a, b = hip_run(module, out, tgt, bbox), hip_run(module, out, tgt, bbox)
    assert same_bits(a[0], b[0]) and same_bits(a[2], b[2]) and all(same_bits(m, n) for m, n in zip(a[1], b[1]))


def test_the_shared_target_and_the_batch_give_the_same_bits(module):
    out, tgt, bbox, _, _ = oracle('bbox')
    a = hip_run(module, out, tgt, bbox)
    feats = module.target_features(torch.from_numpy(tgt).cuda(), torch.from_numpy(bbox))
    assert [tuple(f.shape) for f in feats] == [(2, 41 >> t, 60 >> t, c) for t, c in enumerate((64, 128, 256, 512, 512))]
    b = hip_run(module, out, None, bbox, target=feats)
    assert same_bits(a[0], b[0]) and same_bits(a[2], b[2]) and all(same_bits(m, n) for m, n in zip(a[1], b[1]))
    for i in range(2):      # B = 2 is two B = 1 calls
        c = hip_run(module, out[i:i + 1], tgt[i:i + 1], bbox[:1])
        assert same_bits(a[0][i:i + 1], c[0]) and same_bits(a[2][i:i + 1], c[2])
        assert all(same_bits(m[i:i + 1], n) for m, n in zip(a[1], c[1]))


@pytest.mark.parametrize('C,h,w', [(64, 3, 5), (512, 3, 5), (64, 33, 17), (512, 33, 17)])
def test_the_head_alone_against_float64(C, h, w):
    """Random non-negative features, B = 2; pixel (0, 0) of image 0 is all-zero in both inputs (torch's NaN: here 0), pixel
    (1, 2) of image 1 in feats_out only (its gradient is u / 1e-10, compared by itself: it would drown every other)."""
    rng = np.random.RandomState(C + h)
    fo = rng.uniform(0, 1, (2, C, h, w)).astype(np.float32) * (rng.uniform(0, 1, (2, C, h, w)) > 0.3)
    ft = rng.uniform(0, 1, (2, C, h, w)).astype(np.float32) * (rng.uniform(0, 1, (2, C, h, w)) > 0.3)
    fo, ft = fo.astype(np.float32), ft.astype(np.float32)
    fo[0, :, 0, 0], ft[0, :, 0, 0], fo[1, :, 1, 2] = 0, 0, 0
    lin = rng.uniform(0, 1, C).astype(np.float32)
    runs = {}
    for dtype in (torch.float64, torch.float32):
        x = torch.from_numpy(fo).to(dtype).requires_grad_(True)
        value, maps = lo.head([x], [torch.from_numpy(ft).to(dtype)], [torch.from_numpy(lin).to(dtype)])
        value.sum().backward()
        runs[dtype] = (value.detach().double().numpy().reshape(-1), maps[0].detach().double().numpy(), x.grad.double().numpy())
    x = torch.from_numpy(fo).cuda().requires_grad_(True)
    value = exa.lpips_distance([x], [torch.from_numpy(ft).cuda()], [torch.from_numpy(lin).cuda()])
    assert tuple(value.shape) == (2, 1, 1, 1)
    value.sum().backward()
    grad = x.grad.cpu().double().numpy()
    v64, m64, g64 = runs[torch.float64]
    v32, m32, g32 = runs[torch.float32]
    assert np.isfinite(grad).all() and (grad[0, :, 0, 0] == 0).all() and (g64[0, :, 0, 0] == 0).all()
    rest = np.ones(grad.shape, bool)
    rest[1, :, 1, 2] = False
    for what, sel in (('the rest', rest), ('the zero pixel', ~rest)):
        for metric in (lo.rel_l2, lo.rel_max):
            mine, ref = metric(grad[sel], g64[sel]), max(metric(g32[sel], g64[sel]), FLOOR)
            print('head C=%d %dx%d grad %s %s: HIP %.3g, float32 oracle %.3g, ratio %.2f' % (C, h, w, what, metric.__name__,
                                                                                            mine, ref, mine / ref))
            assert mine <= 4 * ref
    for b in range(2):
        scale = lo.scalar_scale([m32[b] - m64[b]], v64[b], h * w, 4)
        assert abs(float(value[b]) - v64[b]) <= scale, (b, float(value[b]), v64[b], scale)


def test_a_captured_forward_and_backward_replays_the_eager_bits(module):
    out, tgt, bbox, _, _ = oracle('odd')
    eager = hip_run(module, out, tgt, bbox, maps=False)
    x = torch.from_numpy(out).cuda().requires_grad_(True)
    t = torch.from_numpy(tgt).cuda()

    def step():
        value = module(x, t)
        (g,) = torch.autograd.grad(value.sum(), x)
        return value, g

    from exavatar_release_amd._device import warm_up
    warm_up(x.device, step)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        value, g = step()
    value.detach().zero_()
    g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(value.cpu().reshape(-1), eager[0]) and same_bits(g.cpu(), eager[2])
