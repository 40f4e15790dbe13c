"""The image-loss kernels of csrc/ssim.hip against the float64 oracle (tests/loss_oracle64.py), every output within its
per-element bound: the SSIM drop-in (ssim_fwd_kernel / ssim_bwd_kernel), PhotometricLoss (photo_stats_kernel /
photo_grad_kernel) and RGBLoss (l1_kernel), on uniform, photo-like, bright near-flat and near-white content, at the
shapes where the kernels' tiling goes wrong.  The oracle runs in float64 on the device."""
import pytest
import torch

import exavatar_release_amd as exa
from tests import loss_oracle64 as o64
from tests.helpers import LOSS_CONTENT, loss_content, record_stats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs a ROCm device'
    return torch.device('cuda:0')


WORST = {}


def _within(got, ref, tol, name, key=None):
    """every element of got within tol of the float64 ref; records the worst err / tol under key"""
    err = (got.double() - ref).abs()
    bad = err > tol
    ratio = float(torch.where(err > 0, err / tol, torch.zeros_like(err)).max())
    if key is not None:
        WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert not bool(bad.any()), '%s: %d of %d elements outside the bound, worst err/tol %.3g' % (
        name, int(bad.sum()), bad.numel(), ratio)


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    if WORST:
        record_stats('loss_kernels_worst_err_over_tol', {'%s / %s' % k: round(v, 4) for k, v in sorted(WORST.items())})


def _bc(n):
    return {1: (1, 1), 3: (1, 3), 12: (4, 3), 24: (8, 3)}[n]


# ---------------------------------------------------------------------------------------------------------------------
# SSIM drop-in

def _ssim_case(dev, x, y, kind, tag, bbox=None, mask=None, seed=0):
    xg, yg = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    mg = None if mask is None else mask.to(dev)
    m = exa.SSIM()(xg, yg, bbox=bbox, mask=mg)
    G = torch.randn(m.shape, generator=torch.Generator().manual_seed(seed + 7)).to(dev)
    (m * G).sum().backward()
    r = o64.ssim(x.to(dev), y.to(dev), bbox=bbox, mask=mg, G=G)
    assert m.shape == r['map'].shape
    _within(m.detach(), r['map'], r['tol_map'], '%s %s map' % (tag, kind), ('ssim map', kind))
    _within(xg.grad, r['dx'], r['tol_dx'], '%s %s dL/dx' % (tag, kind), ('ssim dx', kind))
    _within(yg.grad, r['dy'], r['tol_dy'], '%s %s dL/dy' % (tag, kind), ('ssim dy', kind))


SSIM_SIZES = [(1, 1), (1, 37), (37, 1), (7, 5), (16, 16), (17, 33), (61, 130)]


@pytest.mark.parametrize('n', [1, 3, 12, 24])
@pytest.mark.parametrize('hw', SSIM_SIZES, ids=['%dx%d' % s for s in SSIM_SIZES])
def test_ssim_matches_float64(dev, hw, n):
    B, C = _bc(n)
    for kind in LOSS_CONTENT:
        x, y = loss_content(kind, (B, C) + hw, seed=n)
        _ssim_case(dev, x, y, kind, 'N=%d %dx%d' % ((n,) + hw), seed=n)


def test_ssim_matches_float64_at_1024(dev):
    for kind in LOSS_CONTENT:
        x, y = loss_content(kind, (1, 3, 1024, 1024), seed=11)
        _ssim_case(dev, x, y, kind, '1024x1024')


@pytest.mark.parametrize('bbox', [None, [[5, 3, 40, 29]], [[-6.7, 12.2, 33.9, 1e4]], [[50, -3, 9, 7]]])
@pytest.mark.parametrize('with_mask', [False, True])
def test_ssim_mask_and_bbox_match_float64(dev, bbox, with_mask):
    B, C, H, W = 2, 3, 45, 58
    gen = torch.Generator().manual_seed(12)
    mask = None
    if with_mask:
        mask = torch.rand((B, 1, H, W), generator=gen)
        mask[:, :, 10:25, 20:40] = 1.0
        mask[:, :, 30:, :15] = 0.0
    for kind in LOSS_CONTENT:
        x, y = loss_content(kind, (B, C, H, W), seed=13)
        _ssim_case(dev, x, y, kind, 'bbox=%s mask=%s' % (bbox, with_mask), bbox=bbox, mask=mask)


# ---------------------------------------------------------------------------------------------------------------------
# PhotometricLoss

def _photo_case(dev, x, y, kind, tag, bbox=None, l1_weight=None, ssim_mask=None, g_loss=0.37):
    B, C, H, W = x.shape
    xg = x.to(dev).requires_grad_(True)
    lw = None if l1_weight is None else l1_weight.to(dev)
    sm = None if ssim_mask is None else ssim_mask.to(dev)
    loss, l1_mean, ssim_mean = exa.PhotometricLoss()(xg, y.to(dev), bbox=bbox, l1_weight=lw, ssim_mask=sm,
                                                     return_terms=True)
    (loss * g_loss).backward()
    x0, y0, cw, ch = o64.crop_window(bbox, H, W)
    nblk = B * C * ((cw + 31) // 32) * ((ch + 31) // 32)
    r = o64.photometric(x.to(dev), y.to(dev), bbox=bbox, l1_weight=lw, ssim_mask=sm, g_loss=g_loss, n_blocks=nblk)
    for name, got in (('loss', loss), ('l1_mean', l1_mean), ('ssim_mean', ssim_mean)):
        _within(got.detach(), r[name], r['tol_' + name], '%s %s %s' % (tag, kind, name), ('photo ' + name, kind))
    _within(xg.grad, r['dx'], r['tol_dx'], '%s %s dL/dx' % (tag, kind), ('photo dx', kind))
    outside = torch.ones((H, W), dtype=torch.bool, device=dev)
    outside[y0:y0 + ch, x0:x0 + cw] = False
    assert bool((xg.grad[:, :, outside] == 0).all()), '%s: dL/dx is not 0 outside the crop' % tag


# (offset, size) pairs: offsets and sizes at residues {0, 1, 10, 11, 21, 31} mod 32, two or more tiles each way
CROPS = [((0, 1), (64, 65)), ((1, 10), (74, 75)), ((10, 11), (97, 85)), ((11, 21), (107, 96)), ((21, 31), (95, 127)),
         ((31, 0), (65, 64))]


@pytest.mark.parametrize('crop', CROPS, ids=['x%d_y%d_w%d_h%d' % (c[0][0], c[0][1], c[1][0], c[1][1]) for c in CROPS])
def test_photometric_crops_at_every_tile_residue(dev, crop):
    (cx, cy), (cw, ch) = crop
    for kind in LOSS_CONTENT:
        x, y = loss_content(kind, (2, 3, 170, 150), seed=cx)
        _photo_case(dev, x, y, kind, 'crop %s' % (crop,), bbox=[[cx, cy, cw, ch]])


NARROW = [[[7, 9, 1, 40]], [[7, 9, 5, 40]], [[7, 9, 10, 40]], [[7, 9, 45, 1]], [[7, 9, 45, 5]], [[7, 9, 45, 10]],
          [[3, 4, 1, 1]], [[20, 30, 5, 10]]]


@pytest.mark.parametrize('bbox', NARROW, ids=['w%d_h%d' % (b[0][2], b[0][3]) for b in NARROW])
def test_photometric_crops_narrower_than_the_window(dev, bbox):
    for kind in LOSS_CONTENT:
        x, y = loss_content(kind, (2, 3, 60, 70), seed=3)
        _photo_case(dev, x, y, kind, 'bbox %s' % bbox, bbox=bbox)


BORDER = [[[0, 0, 50, 40]], [[33, 0, 100, 40]], [[0, 21, 50, 100]], [[33, 21, 100, 100]], [[0, 0, 83, 61]],
          [[-7.6, -3.2, 80.9, 500.0]], [[20.9, 30.99, 1e4, 1e4]], [[-100.5, 10.5, 140.2, 30.7]]]


@pytest.mark.parametrize('bbox', BORDER, ids=['b%d' % i for i in range(len(BORDER))])
def test_photometric_crops_touching_borders_and_float_bboxes(dev, bbox):
    """crops against every border of an 83x61 image, and float bboxes with negative or overflowing values, which the
    reference truncates with int() before clamping (loss.py:20-24)"""
    for kind in ('photo', 'bright'):
        x, y = loss_content(kind, (1, 3, 61, 83), seed=4)
        _photo_case(dev, x, y, kind, 'bbox %s' % bbox, bbox=bbox)


@pytest.mark.parametrize('B', [1, 2, 4])
@pytest.mark.parametrize('C', [1, 3, 4])
def test_photometric_batch_and_channels(dev, B, C):
    gen = torch.Generator().manual_seed(B * 10 + C)
    lw = torch.rand((B, 1, 70, 90), generator=gen)
    sm = (torch.rand((B, 1, 70, 90), generator=gen) > 0.3).float()
    for kind in ('uniform', 'photo', 'white'):
        x, y = loss_content(kind, (B, C, 70, 90), seed=B + C)
        _photo_case(dev, x, y, kind, 'B=%d C=%d' % (B, C), bbox=[[5, 6, 70, 60]], l1_weight=lw, ssim_mask=sm)


@pytest.mark.parametrize('lw_shape,sm_shape,bbox', [
    ('b', None, None), ('1', None, None), (None, 'b', None), (None, '1', None),
    ('b', 'b', [[9, 4, 66, 40]]), ('1', '1', [[9, 4, 66, 40]]), ('b', '1', [[-3, 12, 50, 70]])])
def test_photometric_l1_weight_and_ssim_mask(dev, lw_shape, sm_shape, bbox):
    """per image ([B,1,H,W]) and broadcast ([1,1,H,W]) weights: the kernels index them by image, plane n / C"""
    B, C, H, W = 3, 3, 56, 77
    gen = torch.Generator().manual_seed(14)
    shapes = {'b': (B, 1, H, W), '1': (1, 1, H, W), None: None}
    lw = None if shapes[lw_shape] is None else torch.rand(shapes[lw_shape], generator=gen)
    sm = None
    if shapes[sm_shape] is not None:
        sm = torch.rand(shapes[sm_shape], generator=gen)
        sm[..., :20, :30] = 1.0
        sm[..., 40:, 50:] = 0.0
    for kind in LOSS_CONTENT:
        x, y = loss_content(kind, (B, C, H, W), seed=15)
        _photo_case(dev, x, y, kind, 'lw=%s sm=%s bbox=%s' % (lw_shape, sm_shape, bbox), bbox=bbox, l1_weight=lw,
                    ssim_mask=sm)


def test_photometric_at_production_sizes(dev):
    """the bench's 1024x1024 whole image, and a 1080x1920 frame with a person-sized bbox"""
    for kind in LOSS_CONTENT:
        x, y = loss_content(kind, (1, 3, 1024, 1024), seed=16)
        _photo_case(dev, x, y, kind, '1024x1024')
    for kind in ('photo', 'bright'):
        x, y = loss_content(kind, (1, 3, 1080, 1920), seed=17)
        _photo_case(dev, x, y, kind, '1080x1920', bbox=[[731.4, 96.8, 458.3, 951.0]])


# ---------------------------------------------------------------------------------------------------------------------
# RGBLoss

@pytest.mark.parametrize('bbox', [None, [[3, 5, 40, 31]], [[-2.5, 20.7, 1e3, 9.0]]])
@pytest.mark.parametrize('compose', [False, True])
def test_rgb_loss_matches_float64(dev, bbox, compose):
    B, C, H, W = 2, 3, 47, 64
    gen = torch.Generator().manual_seed(18)
    x, y = loss_content('photo', (B, C, H, W), seed=19)
    mask = bg = None
    if compose:
        mask = torch.rand((B, 1, H, W), generator=gen)
        mask[:, :, :, 30:40] = 1.0
        mask[:, :, :, 40:50] = 0.0
        bg = torch.rand((B, C), generator=gen)
        x[:, :, :, 35:40] = y[:, :, :, 35:40]                                   # m = 1: t == y exactly
        x[:, :, :, 45:50] = bg[:, :, None, None].expand(B, C, H, 5)             # m = 0: t == bg exactly
    xg, yg = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    md, bd = (mask.to(dev), bg.to(dev)) if compose else (None, None)
    m = exa.RGBLoss()(xg, yg, bbox=bbox, mask=md, bg=bd)
    G = torch.randn(m.shape, generator=gen).to(dev)
    (m * G).sum().backward()
    r = o64.l1(x.to(dev), y.to(dev), bbox=bbox, mask=md, bg=bd, G=G)
    _within(m.detach(), r['map'], r['tol_map'], 'RGBLoss map', ('l1 map', 'photo'))
    x0, y0, cw, ch = r['crop']
    d = torch.zeros_like(r['dx'], dtype=torch.bool)
    d[:, :, y0:y0 + ch, x0:x0 + cw] = True
    exact_tie = d.clone()
    exact_tie[:, :, y0:y0 + ch, x0:x0 + cw] = r['map'] == 0
    assert int(exact_tie.sum()) > 0 or not compose
    sure = ~r['tie']
    assert bool((xg.grad.double()[sure] == r['dx'][sure]).all()), 'RGBLoss backward: wrong sign away from ties'
    assert bool((xg.grad[exact_tie] == 0).all()), 'RGBLoss backward: not 0 where x == t'
    near = r['tie'] & ~exact_tie
    Gf = torch.zeros_like(xg.grad)
    Gf[:, :, y0:y0 + ch, x0:x0 + cw] = G
    got = xg.grad[near]
    assert bool(((got == 0) | (got == Gf[near]) | (got == -Gf[near])).all())
    assert int(near.sum()) <= max(8, near.numel() // 10000), int(near.sum())      # a handful of pixels within a few ulp
    record_stats('rgb_loss_near_ties', {'bbox': str(bbox), 'compose': compose, 'near_ties': int(near.sum()),
                                        'exact_ties': int(exact_tie.sum())})
    dy_ref = -r['dx'] * (mask.to(dev).double() if compose else 1.0)
    ok = ~r['tie'] & ~exact_tie
    assert bool(((yg.grad.double() - dy_ref).abs()[ok] <= o64.U * dy_ref.abs()[ok]).all())


# ---------------------------------------------------------------------------------------------------------------------
# determinism

def test_loss_kernels_are_deterministic(dev):
    """no atomics: two calls give bit-identical outputs"""
    x, y = loss_content('photo', (2, 3, 200, 333), seed=20)
    x, y = x.to(dev), y.to(dev)
    lw = torch.rand((2, 1, 200, 333), generator=torch.Generator().manual_seed(21)).to(dev)

    def run():
        xs = x.clone().requires_grad_(True)
        ys = y.clone().requires_grad_(True)
        m = exa.SSIM()(xs, ys, bbox=[[7, 3, 300, 190]])
        (m * m).sum().backward()
        xp = x.clone().requires_grad_(True)
        terms = exa.PhotometricLoss()(xp, y, bbox=[[11, 5, 290, 180]], l1_weight=lw, ssim_mask=lw, return_terms=True)
        terms[0].backward()
        xl = x.clone().requires_grad_(True)
        l1 = exa.RGBLoss()(xl, y, mask=lw, bg=torch.full((2, 3), 0.5, device=dev))
        l1.sum().backward()
        return [m.detach(), xs.grad, ys.grad, *[t.detach() for t in terms], xp.grad, l1.detach(), xl.grad]
    a, b = run(), run()
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), i
