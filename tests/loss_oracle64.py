"""Float64 oracle for the image-loss kernels of ``csrc/ssim.hip``, with a per-pixel error bound next to every output.

THIS IS TEST INFRASTRUCTURE.  It restates ``oracle/loss_oracle.py`` (itself pinned to the reference's ``RGBLoss`` /
``SSIM`` classes by ``tests/golden/ref_ssim.npz``) in float64: the SSIM map, its three partial-derivative maps,
``dL/dx`` and ``dL/dy`` of the map; the fused photometric loss (value, both means, ``dL/dx``); the L1 map and its
backward.  Filtering is two separable 11-tap passes built from slices and adds with zero padding at the crop border
(no float64 ``conv2d``), so the module computes the same on the CPU and on a ROCm device.  The window is the
reference's: the 1-D Gaussian (sigma 1.5) normalised in float32, its outer product taken in float64.

Error bound
-----------
An fp32 evaluation of the reference formula makes a relative error of a few ``u = 2**-24`` in every filtered
statistic (mu1, mu2, E11, E22, E12: sums of 11 or 121 weighted terms), relative to the filtered ABSOLUTE values
``|mu|_w = w * |x|`` and ``|E12|_w = w * |x y|``.  To first order the derived quantities then carry absolute errors,
in units of u (a product of two means carries three roundings),

    A = 2 mu1 mu2 + C1                 eA ~ |A|
    B = 2 (E12 - mu1 mu2) + C2         eB = 2 (|E12|_w + 3 |mu1|_w |mu2|_w)
    C = mu1^2 + mu2^2 + C1             eC ~ C
    D = (E11 - mu1^2) + (E22 - mu2^2) + C2       eD = E11 + 3 |mu1|_w^2 + E22 + 3 |mu2|_w^2

B and D are the cancelling differences (sigma^2 = E[x^2] - mu^2 on bright flat content); A and C are sums of
non-negative terms on image content and stay relatively exact.  So for ``ssim = A B / (C D)``

    e_ssim = |A| eB / (C |D|) + |ssim| (eD / |D| + 1)

which is ``|ssim| kappa`` with ``kappa = eD/D + eB/|B| + 1`` written without dividing by B (B = 0 is legal).  The
derivative maps the backward filters again carry the same conditioning, each through its own formula:

    d12 = 2 A / (C D)                  e12 = |d12| (eD/|D| + 1)
    d11 = -A B / (C D^2)               e11 = |A| eB / (C D^2) + |d11| (2 eD/|D| + 1)          (1/D^2: twice kappa_D)
    d1  = 2 [P - Q] / (C D)^2,  P = mu2 (B - A) C D,  Q = mu1 A B (D - C)
                                       e1  = 2 (eP + eQ) / (C D)^2 + 2 |d1| (eD/|D| + 1)

with eP, eQ the first-order bounds of the two products (every factor's error times the other factors, plus one
rounding of each product; B - A and D - C get eB + |A| + |B - A| and eD + C + |D - C|).  The second 11x11 pass is
linear, so its error is the filter of the absolute errors, plus the rounding of the pass and of the final
combination, bounded by the same filter applied to the absolute terms:

    e_dx = w*(|g| e1) + 2|x| w*(|g| e11) + |y| w*(|g| e12)  +  w*|g d1| + 2|x| w*|g d11| + |y| w*|g d12|

The bound is ``K u e``.  K absorbs the small integer constants of each step (how many roundings per sum, FMA or
not); it was calibrated once on the CPU against two fp32 formulations of the reference formula -- its own ``conv2d``
and a separable horizontal-then-vertical emulation of the kernels' order -- over uniform, photo-like, bright near-flat
and near-white content, 40x48 to 256x256: the largest ``err / (u e)`` was 6.0 for the conv2d formulation (SSIM
map, uniform content) and 2.2 for the separable one; gradients stay under 0.7.  K = 24 leaves both under K/3, which
tests/test_loss_oracle64.py asserts.
A kernel outside ``K u e`` is less accurate than the reference formula itself.

Means are bounded by the mean of the per-pixel bounds plus the rounding of summing the per-pixel values, ``u L
mean(|v|)`` with L the depth of the summation tree (``sum_depth``).  The L1 map has no conditioning: its bound is the
fp32 rounding of ``|x - t|`` and, with a composed target ``t = y m + (1 - m) bg``, of forming t (``l1``).
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24               # fp32 unit roundoff
K = 24.0                     # calibrated once on the CPU (docstring); fixed, never tuned per test
C1 = 0.01 ** 2               # the reference's constants (loss.py:69-70), as Python floats
C2 = 0.03 ** 2
R = 5                        # window radius (window_size 11)


def window_1d():
    """The reference's 1-D window (loss.py:35-43): exp() in double, rounded to float32, normalised by its float32 sum;
    returned as Python floats (exactly those float32 values)."""
    gauss = torch.tensor([math.exp(-(x - R) ** 2 / float(2 * 1.5 ** 2)) for x in range(2 * R + 1)], dtype=torch.float32)
    return (gauss / gauss.sum()).double().tolist()


def filt(a, g=None):
    """Separable 11x11 Gaussian filter of the last two dims, zero padding (= conv2d padding 5): horizontal pass, then
    vertical.  The window is symmetric, so this is also its own adjoint."""
    g = window_1d() if g is None else g
    H, W = a.shape[-2:]
    p = F.pad(a, (R, R, 0, 0))
    h = g[0] * p[..., :, 0:W]
    for k in range(1, 2 * R + 1):
        h = h + g[k] * p[..., :, k:k + W]
    p = F.pad(h, (0, 0, R, R))
    v = g[0] * p[..., 0:H, :]
    for k in range(1, 2 * R + 1):
        v = v + g[k] * p[..., k:k + H, :]
    return v


def crop_window(bbox, H, W):
    """(x0, y0, w, h) of the reference's bbox clamp (loss.py:19-24 / 51-56): ``int()`` of each value, top-left clamped
    at 0, bottom-right at the image size (from the CLAMPED top-left); the whole image when ``bbox`` is None."""
    if bbox is None:
        return 0, 0, W, H
    xmin, ymin, width, height = [int(v) for v in bbox[0]]
    x0, y0 = max(xmin, 0), max(ymin, 0)
    x1, y1 = min(x0 + width, W), min(y0 + height, H)
    return x0, y0, max(x1 - x0, 0), max(y1 - y0, 0)


def _stats(a, b):
    """The SSIM map of (a, b), its derivative maps with respect to a, and their error maps (units of u)."""
    g = window_1d()
    mu1, mu2 = filt(a, g), filt(b, g)
    e11, e22, e12 = filt(a * a, g), filt(b * b, g), filt(a * b, g)
    am1, am2, a12 = filt(a.abs(), g), filt(b.abs(), g), filt((a * b).abs(), g)
    mu12 = mu1 * mu2
    A = 2 * mu12 + C1
    B = 2 * (e12 - mu12) + C2
    Cc = mu1 * mu1 + mu2 * mu2 + C1
    D = (e11 - mu1 * mu1) + (e22 - mu2 * mu2) + C2
    CD = Cc * D
    ssim = A * B / CD
    eB = 2 * (a12 + 3 * am1 * am2)
    eD = e11 + 3 * am1 * am1 + e22 + 3 * am2 * am2
    aA, aD, rD = A.abs(), D.abs(), eD / D.abs()
    e_ssim = aA * eB / (Cc * aD) + ssim.abs() * (rD + 1)
    P = mu2 * (B - A) * Cc * D
    Q = mu1 * A * B * (D - Cc)
    d1 = 2 * (P - Q) / (CD * CD)
    d11 = -A * B / (CD * D)
    d12 = 2 * A / CD
    eBA = eB + aA + (B - A).abs()
    eDC = eD + Cc + (D - Cc).abs()
    eP = (am2 * (B - A).abs() * Cc * aD + mu2.abs() * eBA * Cc * aD + (mu2 * (B - A)).abs() * Cc * (aD + eD) + P.abs())
    eQ = (am1 * (A * B * (D - Cc)).abs() + mu1.abs() * (aA * B.abs() + aA * eB) * (D - Cc).abs()
          + (mu1 * A * B).abs() * eDC + Q.abs())
    e1 = 2 * (eP + eQ) / (CD * CD) + 2 * d1.abs() * (rD + 1)
    e11m = aA * eB / (Cc * aD * aD) + d11.abs() * (2 * rD + 1)
    e12m = d12.abs() * (rD + 1)
    return dict(map=ssim, e_map=e_ssim, d1=d1, d11=d11, d12=d12, e1=e1, e11=e11m, e12=e12m)


def _grad(a, b, s, G):
    """dL/da = w*(G d1) + 2 a w*(G d11) + b w*(G d12) and its error map (units of u)."""
    g = window_1d()
    c0, c1, c2 = filt(G * s['d1'], g), filt(G * s['d11'], g), filt(G * s['d12'], g)
    aG = G.abs()
    e = (filt(aG * s['e1'], g) + 2 * a.abs() * filt(aG * s['e11'], g) + b.abs() * filt(aG * s['e12'], g)
         + filt((G * s['d1']).abs(), g) + 2 * a.abs() * filt((G * s['d11']).abs(), g)
         + b.abs() * filt((G * s['d12']).abs(), g))
    return c0 + 2 * a * c1 + b * c2, e


def ssim_derivative_maps(a, b):
    """map, d ssim/d mu1, d ssim/d E11, d ssim/d E12 of ssim(a, b) in float64 (the maps the forward kernels store)."""
    s = _stats(a.double(), b.double())
    return s['map'], s['d1'], s['d11'], s['d12']


def ssim(x, y, bbox=None, mask=None, G=None):
    """Float64 ``SSIM()(x, y, bbox, mask)`` (loss.py:45-74) and, for the upstream gradient G (shape of the map, default
    ones), ``dL/dx`` and ``dL/dy`` over the full [B, C, H, W] inputs (0 outside the crop).  Each output comes with its
    bound ``tol_*`` (absolute, per element)."""
    x, y = x.double(), y.double()
    B_, C_, H, W = x.shape
    x0, y0, cw, ch = crop_window(bbox, H, W)
    m = None if mask is None else mask.double().expand(B_, 1, H, W)
    xm, ym = (x, y) if m is None else (x * m, y * m)
    a, b = xm[:, :, y0:y0 + ch, x0:x0 + cw], ym[:, :, y0:y0 + ch, x0:x0 + cw]
    G = torch.ones_like(a) if G is None else G.double().expand(a.shape)
    s = _stats(a, b)
    gx, ex = _grad(a, b, s, G)
    t = _stats(b, a)
    gy, ey = _grad(b, a, t, G)
    out = dict(map=s['map'], tol_map=K * U * torch.maximum(s['e_map'], t['e_map']))
    for name, gr, er in (('dx', gx, ex), ('dy', gy, ey)):
        full, tol = torch.zeros_like(x), torch.zeros_like(x)
        full[:, :, y0:y0 + ch, x0:x0 + cw] = gr
        tol[:, :, y0:y0 + ch, x0:x0 + cw] = K * U * er
        if m is not None:          # d(x m)/dx = m, and one more rounding of the product
            full, tol = full * m, tol * m.abs() + U * (full * m).abs()
        out[name], out['tol_' + name] = full, tol
    return out


def sum_depth(n_blocks):
    """Depth of the fused loss's summation: four sequential terms per thread, a 64-lane butterfly, four waves, then the
    partial sums of ``n_blocks`` workgroups (a tree, allowed two levels per halving) and the division by N."""
    return 4 + 6 + 2 + 2 * max(math.ceil(math.log2(max(n_blocks, 1))), 1) + 2


def photometric(x, y, bbox=None, l1_weight=None, ssim_mask=None, w_l1=0.8, w_ssim=0.2, g_loss=1.0, n_blocks=1):
    """Float64 ``PhotometricLoss``: ``w_l1 mean(l1_weight |x - y|) + w_ssim (1 - mean(ssim(x m, y m)))`` over the bbox
    crop (``oracle.loss_oracle.photometric_loss``), its two means, and ``g_loss * dL/dx`` over the full image (0
    outside the crop), each with its bound.  ``n_blocks`` is the number of partial sums the means are reduced from."""
    x, y = x.double(), y.double()
    B_, C_, H, W = x.shape
    x0, y0, cw, ch = crop_window(bbox, H, W)
    sl = (slice(None), slice(None), slice(y0, y0 + ch), slice(x0, x0 + cw))
    xc, yc = x[sl], y[sl]
    m = torch.ones_like(xc[:, :1]) if ssim_mask is None else ssim_mask.double().expand(B_, 1, H, W)[sl]
    lw = torch.ones_like(xc[:, :1]) if l1_weight is None else l1_weight.double().expand(B_, 1, H, W)[sl]
    a, b = xc * m, yc * m
    s = _stats(a, b)
    gs_in, e_in = _grad(a, b, s, torch.ones_like(a))
    n = xc.numel()
    L = sum_depth(n_blocks)
    l1 = (xc - yc).abs() * lw
    l1_mean, ssim_mean = l1.mean(), s['map'].mean()
    tol_l1 = K * U * l1.mean() + U * L * l1.mean()
    tol_ssim = K * U * s['e_map'].mean() + U * L * s['map'].abs().mean()
    loss = w_l1 * l1_mean + w_ssim * (1 - ssim_mean)
    tol_loss = abs(w_l1) * tol_l1 + abs(w_ssim) * tol_ssim + K * U * (abs(w_l1) * l1_mean + abs(w_ssim) * (1 + ssim_mean.abs()))
    gs = -(w_ssim / n) * m * gs_in
    gl = (w_l1 / n) * torch.sign(xc - yc) * lw
    dx, tol = torch.zeros_like(x), torch.zeros_like(x)
    dx[sl] = g_loss * (gs + gl)
    tol[sl] = abs(g_loss) * K * U * ((abs(w_ssim) / n) * m.abs() * e_in + gs.abs() + gl.abs())
    return dict(loss=loss, tol_loss=tol_loss, l1_mean=l1_mean, tol_l1_mean=tol_l1,
                ssim_mean=ssim_mean, tol_ssim_mean=tol_ssim, dx=dx, tol_dx=tol)


def l1(x, y, bbox=None, mask=None, bg=None, G=None):
    """Float64 ``RGBLoss()(x, y, bbox, mask, bg)`` (loss.py:15-29): the map ``|x - t|`` over the crop with ``t = y m +
    (1 - m) bg`` when both mask and bg are given, its fp32 rounding bound ``tol_map``, ``dx = sign(x - t) G`` over the
    full image, and ``tie``: the crop pixels within the rounding of t of a tie, where an fp32 t (fused or not) may
    land on either side of x."""
    x, y = x.double(), y.double()
    B_, C_, H, W = x.shape
    x0, y0, cw, ch = crop_window(bbox, H, W)
    if mask is not None and bg is not None:
        m = mask.double().expand(B_, 1, H, W)
        bgd = bg.double().expand(B_, C_)[:, :, None, None]
        t = y * m + (1 - m) * bgd
        st = (y * m).abs() + ((1 - m) * bgd).abs()
    else:
        t, st = y, torch.zeros_like(y)
    sl = (slice(None), slice(None), slice(y0, y0 + ch), slice(x0, x0 + cw))
    d = x[sl] - t[sl]
    margin = 4 * U * st[sl]
    G = torch.ones_like(d) if G is None else G.double().expand(d.shape)
    dx = torch.zeros_like(x)
    dx[sl] = torch.sign(d) * G
    tie = torch.zeros_like(x, dtype=torch.bool)
    tie[sl] = (d.abs() <= margin) & (margin > 0)
    return dict(map=d.abs(), tol_map=margin + 2 * U * d.abs(), dx=dx, tie=tie, crop=(x0, y0, cw, ch))
