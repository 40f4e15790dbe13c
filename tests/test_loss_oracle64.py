"""CPU checks of the float64 image-loss oracle (tests/loss_oracle64.py): it equals oracle/loss_oracle.py evaluated in
float64 with autograd, its analytic gradients agree with finite differences, its error bound holds for two fp32
formulations of the reference formula with a third of K to spare, and the bound is tight enough that perturbed fp32
formulations break it."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import loss_oracle as lo
from tests import loss_oracle64 as o64
from tests.helpers import LOSS_CONTENT, loss_content


def _window64(window_size, feat_dim, dtype=torch.float32):
    """loss_oracle.ssim_window with the outer product taken in float64 (the separable window the oracle uses)"""
    g = torch.tensor(o64.window_1d(), dtype=torch.float64)[:, None]
    return (g @ g.T)[None, None].repeat(feat_dim, 1, 1, 1).to(dtype)


def _rand(shape, seed, lo_=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return lo_ + (hi - lo_) * torch.rand(shape, generator=g, dtype=torch.float64)


def _close(got, ref, tol=1e-12):
    return float((got - ref).abs().max()) <= tol * max(1.0, float(ref.abs().max()))


# ---------------------------------------------------------------------------------------------------------------------
# fp32 formulations of the reference formula (and perturbed ones)

def _window32(sigma=1.5):
    gauss = torch.tensor([math.exp(-(x - 5) ** 2 / float(2 * sigma ** 2)) for x in range(11)], dtype=torch.float32)
    return gauss / gauss.sum()


def _sep32(a, g, pad):
    """horizontal then vertical 11-tap pass in float32, in the kernels' order"""
    H, W = a.shape[-2:]
    p = F.pad(a, (5, 5, 0, 0), mode=pad)
    h = torch.zeros_like(a)
    for k in range(11):
        h = h + g[k] * p[..., :, k:k + W]
    p = F.pad(h, (0, 0, 5, 5), mode=pad)
    v = torch.zeros_like(a)
    for k in range(11):
        v = v + g[k] * p[..., k:k + H, :]
    return v


def separable_fp32(x, y, G, c2=0.03 ** 2, sigma=1.5, pad='constant', e11_factor=2.0):
    """The SSIM map and dL/dx of ssim.hip's formulas, evaluated in float32 with separable passes"""
    g = _window32(sigma)

    def f(t):
        return _sep32(t, g, pad)
    x, y, G = x.float(), y.float(), G.float()
    c1, c2 = torch.tensor(0.01, dtype=torch.float32) ** 2, torch.tensor(c2, dtype=torch.float32)
    mu1, mu2, e11, e22, e12 = f(x), f(y), f(x * x), f(y * y), f(x * y)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    A, B = 2 * mu12 + c1, 2 * (e12 - mu12) + c2
    C, D = mu1_sq + mu2_sq + c1, (e11 - mu1_sq) + (e22 - mu2_sq) + c2
    inv = 1 / (C * D)
    m = A * B * inv
    d1 = 2 * (mu2 * (B - A) * C * D - mu1 * A * B * (D - C)) * inv * inv
    d11, d12 = -A * B * inv / D, 2 * A * inv
    return m, f(G * d1) + e11_factor * x * f(G * d11) + y * f(G * d12)


def reference_fp32(x, y, G, **kw):
    """oracle.loss_oracle.ssim_map (the reference's conv2d formula) in float32, and its autograd dL/dx, dL/dy"""
    xi, yi = x.float().clone().requires_grad_(True), y.float().clone().requires_grad_(True)
    m = lo.ssim_map(xi, yi, **kw)
    (m * G.float()).sum().backward()
    return m.detach(), xi.grad, yi.grad


def _worst(got, ref, tol):
    """max err / tol (0 where both are 0)"""
    err = (got.double() - ref).abs()
    return float(torch.where(err > 0, err / tol, torch.zeros_like(err)).max())


# ---------------------------------------------------------------------------------------------------------------------
# the oracle against oracle/loss_oracle.py in float64

@pytest.mark.parametrize('shape,kw', [
    ((1, 1, 1, 1), {}),
    ((1, 3, 7, 5), {}),
    ((2, 3, 13, 17), {'mask': True}),
    ((2, 1, 19, 23), {'bbox': [[3.7, -2.0, 12.9, 30.0]]}),
    ((1, 2, 21, 18), {'mask': True, 'bbox': [[-4, 5, 15, 9]]}),
])
def test_ssim_matches_loss_oracle_in_float64(monkeypatch, shape, kw):
    monkeypatch.setattr(lo, 'ssim_window', _window64)
    x, y = _rand(shape, 1), _rand(shape, 2)
    mask = _rand((shape[0], 1) + shape[2:], 3) if kw.get('mask') else None
    bbox = kw.get('bbox')
    xi, yi = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    m = lo.ssim_map(xi, yi, bbox=bbox, mask=mask)
    G = _rand(m.shape, 4, -1.0, 1.0)
    (m * G).sum().backward()
    r = o64.ssim(x, y, bbox=bbox, mask=mask, G=G)
    assert r['map'].shape == m.shape
    assert _close(r['map'], m.detach())
    assert _close(r['dx'], xi.grad)
    assert _close(r['dy'], yi.grad)


@pytest.mark.parametrize('shape,kw', [
    ((1, 3, 9, 11), {}),
    ((2, 3, 16, 14), {'bbox': [[2.5, 3.9, 9.0, 40.0]], 'l1_weight': 'b'}),
    ((2, 1, 15, 12), {'l1_weight': 'b', 'ssim_mask': 'b'}),
    ((3, 3, 12, 13), {'l1_weight': '1', 'ssim_mask': '1', 'bbox': [[-3, 1, 10, 8]]}),
])
def test_photometric_matches_loss_oracle_in_float64(monkeypatch, shape, kw):
    monkeypatch.setattr(lo, 'ssim_window', _window64)
    x, y = _rand(shape, 5), _rand(shape, 6)
    wshape = {'b': (shape[0], 1) + shape[2:], '1': (1, 1) + shape[2:]}
    lw = _rand(wshape[kw['l1_weight']], 7) if 'l1_weight' in kw else None
    sm = _rand(wshape[kw['ssim_mask']], 8) if 'ssim_mask' in kw else None
    bbox = kw.get('bbox')
    xi = x.clone().requires_grad_(True)
    L = lo.photometric_loss(xi, y, bbox=bbox, l1_weight=None if lw is None else lw.expand(shape[0], 1, *shape[2:]),
                            ssim_mask=sm)
    L.backward()
    r = o64.photometric(x, y, bbox=bbox, l1_weight=lw, ssim_mask=sm)
    assert abs(float(r['loss'] - L.detach())) <= 1e-12
    assert _close(r['dx'], xi.grad)
    x0, y0, cw, ch = o64.crop_window(bbox, shape[2], shape[3])
    xc, yc = x[..., y0:y0 + ch, x0:x0 + cw], y[..., y0:y0 + ch, x0:x0 + cw]
    m = 1.0 if sm is None else sm[..., y0:y0 + ch, x0:x0 + cw]
    assert abs(float(r['ssim_mean'] - lo.ssim_map(xc * m, yc * m).mean())) <= 1e-12
    w = 1.0 if lw is None else lw[..., y0:y0 + ch, x0:x0 + cw]
    assert abs(float(r['l1_mean'] - ((xc - yc).abs() * w).mean())) <= 1e-12


@pytest.mark.parametrize('kw', [{}, {'bbox': [[2, 3, 9, 7]]}, {'mask': True, 'bg': True}, {'mask': True, 'bg': True, 'bbox': [[-1, 2, 8, 30]]}])
def test_l1_matches_loss_oracle_in_float64(kw):
    shape = (2, 3, 10, 12)
    x, y = _rand(shape, 9), _rand(shape, 10)
    mask = _rand((2, 1, 10, 12), 11) if kw.get('mask') else None
    bg = _rand((2, 3), 12) if kw.get('bg') else None
    xi = x.clone().requires_grad_(True)
    m = lo.rgb_loss(xi, y, bbox=kw.get('bbox'), mask=mask, bg=bg)
    G = _rand(m.shape, 13, -1.0, 1.0)
    (m * G).sum().backward()
    r = o64.l1(x, y, bbox=kw.get('bbox'), mask=mask, bg=bg, G=G)
    assert _close(r['map'], m.detach())
    assert _close(r['dx'], xi.grad)


# ---------------------------------------------------------------------------------------------------------------------
# analytic gradients against finite differences

def test_ssim_gradients_match_finite_differences():
    shape = (1, 2, 6, 7)
    x, y = _rand(shape, 14), _rand(shape, 15)
    mask, bbox = _rand((1, 1, 6, 7), 16), [[1, 0, 5, 6]]
    G = _rand((1, 2, 6, 5), 17, -1.0, 1.0)
    r = o64.ssim(x, y, bbox=bbox, mask=mask, G=G)

    def f(a, b):
        return float((o64.ssim(a, b, bbox=bbox, mask=mask)['map'] * G).sum())
    h = 1e-6
    for name, grad in (('x', r['dx']), ('y', r['dy'])):
        fd = torch.zeros_like(x)
        for i in range(x.numel()):
            e = torch.zeros(x.numel(), dtype=torch.float64)
            e[i] = h
            e = e.view(shape)
            fd.view(-1)[i] = (f(x + e, y) - f(x - e, y)) / (2 * h) if name == 'x' else (f(x, y + e) - f(x, y - e)) / (2 * h)
        assert float((fd - grad).abs().max()) <= 1e-7 * float(grad.abs().max()) + 1e-9, name


def test_photometric_gradient_matches_finite_differences():
    shape = (2, 2, 7, 6)
    x = _rand(shape, 18)
    y = x + torch.where(_rand(shape, 19) < 0.5, -1.0, 1.0) * _rand(shape, 20, 0.01, 0.1)     # |x - y| >= 0.01: no kink
    lw, sm, bbox = _rand((2, 1, 7, 6), 21), _rand((1, 1, 7, 6), 22), [[0, 1, 6, 5]]
    r = o64.photometric(x, y, bbox=bbox, l1_weight=lw, ssim_mask=sm)
    fd, h = torch.zeros_like(x), 1e-6
    for i in range(x.numel()):
        e = torch.zeros(x.numel(), dtype=torch.float64)
        e[i] = h
        e = e.view(shape)
        fd.view(-1)[i] = (float(o64.photometric(x + e, y, bbox=bbox, l1_weight=lw, ssim_mask=sm)['loss'])
                          - float(o64.photometric(x - e, y, bbox=bbox, l1_weight=lw, ssim_mask=sm)['loss'])) / (2 * h)
    assert float((fd - r['dx']).abs().max()) <= 1e-7 * float(r['dx'].abs().max())
    assert bool((r['dx'][..., 0:1, :] == 0).all()) and bool((r['dx'][..., 6:, :] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# the bound: it holds for fp32 formulations of the reference formula, with margin, and only for them

BOUND_SHAPES = [(1, 1, 1, 1), (1, 1, 1, 37), (1, 1, 37, 1), (1, 3, 7, 5), (2, 3, 40, 48)]


@pytest.mark.parametrize('kind', LOSS_CONTENT)
@pytest.mark.parametrize('shape', BOUND_SHAPES)
def test_bound_holds_for_both_fp32_formulations(kind, shape):
    x, y = loss_content(kind, shape, seed=3)
    G = torch.randn(shape, generator=torch.Generator().manual_seed(4))
    r = o64.ssim(x, y, G=G)
    m_ref, dx_ref, dy_ref = reference_fp32(x, y, G)
    m_sep, dx_sep = separable_fp32(x, y, G)
    _, dy_sep = separable_fp32(y, x, G)
    worst = {'ref map': _worst(m_ref, r['map'], r['tol_map']), 'ref dx': _worst(dx_ref, r['dx'], r['tol_dx']),
             'ref dy': _worst(dy_ref, r['dy'], r['tol_dy']), 'sep map': _worst(m_sep, r['map'], r['tol_map']),
             'sep dx': _worst(dx_sep, r['dx'], r['tol_dx']), 'sep dy': _worst(dy_sep, r['dy'], r['tol_dy'])}
    assert max(worst.values()) <= 1.0 / 3.0, worst


@pytest.mark.parametrize('kind', LOSS_CONTENT)
def test_bound_holds_for_the_fp32_photometric_loss(kind):
    shape = (2, 3, 45, 38)
    x, y = loss_content(kind, shape, seed=5)
    lw = torch.rand((2, 1, 45, 38), generator=torch.Generator().manual_seed(6))
    sm = (torch.rand((1, 1, 45, 38), generator=torch.Generator().manual_seed(7)) > 0.2).float()
    bbox = [[3, 4, 33, 40]]
    xi = x.clone().requires_grad_(True)
    L = lo.photometric_loss(xi, y, bbox=bbox, l1_weight=lw, ssim_mask=sm)
    L.backward()
    r = o64.photometric(x, y, bbox=bbox, l1_weight=lw, ssim_mask=sm)
    assert abs(float(L.detach()) - float(r['loss'])) <= float(r['tol_loss']) / 3
    assert _worst(xi.grad, r['dx'], r['tol_dx']) <= 1.0 / 3.0


@pytest.mark.parametrize('compose', [False, True])
def test_bound_holds_for_the_fp32_l1_map(compose):
    shape = (2, 3, 30, 31)
    x, y = loss_content('photo', shape, seed=8)
    gen = torch.Generator().manual_seed(9)
    mask = torch.rand((2, 1, 30, 31), generator=gen) if compose else None
    bg = torch.rand((2, 3), generator=gen) if compose else None
    r = o64.l1(x, y, bbox=[[2, 1, 25, 28]], mask=mask, bg=bg)
    m = lo.rgb_loss(x, y, bbox=[[2, 1, 25, 28]], mask=mask, bg=bg)
    assert bool(((m.double() - r['map']).abs() <= r['tol_map']).all())


def test_bound_is_not_vacuous_on_uniform_content():
    x, y = loss_content('uniform', (2, 3, 64, 64), seed=10)
    r = o64.ssim(x, y, G=torch.ones(2, 3, 64, 64))
    assert float(r['tol_map'].median()) <= 2.5e-5          # measured 2.0e-5
    assert float(r['tol_map'].max()) <= 6e-5               # measured 4.7e-5
    assert float((r['tol_dx'] / r['dx'].abs().max()).max()) <= 4e-4     # measured 2.7e-4 of the largest gradient


@pytest.mark.parametrize('perturbation,kinds', [
    ({'c2': 0.03}, ('uniform', 'photo')),           # on bright flat content C2 dominates both B and D either way
    ({'sigma': 1.6}, ('uniform', 'photo')),
    ({'pad': 'replicate'}, LOSS_CONTENT),
    ({'e11_factor': 1.0}, LOSS_CONTENT),
])
def test_perturbed_fp32_formulations_break_the_bound(perturbation, kinds):
    """A wrong constant, window, padding or a dropped factor 2 must show against the bound (at least 4x over it; the
    C2 and sigma perturbations are invisible on bright near-flat content, where the reference formula itself is only
    good to ~1e-3)."""
    for kind in kinds:
        x, y = loss_content(kind, (1, 3, 40, 48), seed=3)
        G = torch.randn(x.shape, generator=torch.Generator().manual_seed(4))
        r = o64.ssim(x, y, G=G)
        m, dx = separable_fp32(x, y, G, **perturbation)
        worst = max(_worst(m, r['map'], r['tol_map']), _worst(dx, r['dx'], r['tol_dx']))
        assert worst > 4.0, (kind, worst)
