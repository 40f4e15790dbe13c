"""CPU restatement of ``lpips.LPIPS(net='vgg')`` 0.1.4 (eval mode) behind the reference's bbox crop
(``avatar/common/nets/loss.py:77-95``) with torch ops, in float64 or float32:

1. crop both images to the clamped bbox (``bbox[0]`` for the whole batch);
2. ``x = x * 2 - 1``, then ``(x - shift) / scale`` per channel;
3. VGG-16 ``features``: 3x3 convolutions, stride 1, zero padding 1 (at the border of the crop), bias, ReLU; a 2x2 stride-2
   max-pool (floor) in front of blocks 2-5;
4. the taps relu1_2, relu2_2, relu3_3, relu4_3, relu5_3;
5. per tap ``n(f) = f / (sqrt(sum_c f^2) + 1e-10)``, ``d = sum_c w_c (n(f_out) - n(f_target))_c^2``, ``D`` = the mean of d;
6. the sum of the five ``D``, ``[B, 1, 1, 1]``.

ONE difference from torch, shared with the HIP module: the derivative of ``sqrt(sum_c f^2)`` is 0 where the sum is 0
(torch gives NaN there).  ``norm`` below writes that with a ``where``.

The scalar's bound.  The HIP value of one image is ``sum_l mean(d_l)``.  Its error has two parts.  (a) The error of the
maps: ``|mean(e_l)| <= mean|e_l| <= rms(e_l)`` (Jensen), so a run whose maps carry the error ``e_l`` is off by at most
``sum_l rms(e_l)``; the project's bar grants the HIP maps 4 x the float32 oracle's own error, hence ``4 sum_l rms(e_l)`` with
``e_l`` the float32 oracle's map error against float64.  (b) The sums themselves: an element passes through at most
``d = sum_depth(n)`` float32 additions on its way into the value, plus the division by n and the rounding of the result:
``(d + 2) 2^-24`` of the value, all terms being non-negative (Higham's bound for a sum of depth d, first order).
``scalar_scale(e, value, n, k)`` is ``k sum_l rms(e_l) + (d + 2) 2^-24 |value|``; the HIP scalar is asserted within
``k = 4``, the float32 oracle within ``k = 1`` (``check_float32_scalar``; torch's pairwise sums are not deeper than d).
"""
import numpy as np
import torch
import torch.nn.functional as F

from exavatar_release_amd.lpips import SCALE, SHIFT, TAP_LAYER
from exavatar_release_amd.losses import _crop_window

POOL_BEFORE = (2, 4, 7, 10)
U = 2.0 ** -24


def as_tensors(convs, lins, dtype):
    t = lambda a: torch.from_numpy(np.array(a)).to(dtype)      # noqa: E731
    return [(t(w), t(b)) for w, b in convs], [t(x).reshape(-1) for x in lins]


def crop(img, bbox):
    x0, y0, w, h = _crop_window(bbox, img.shape[2], img.shape[3])
    return img[:, :, y0:y0 + h, x0:x0 + w]


def input_map(x, shift=SHIFT, scale=SCALE):
    shift = torch.tensor(shift, dtype=torch.float64).to(x).view(1, 3, 1, 1)
    scale = torch.tensor(scale, dtype=torch.float64).to(x).view(1, 3, 1, 1)
    return ((x * 2 - 1) - shift) / scale


def trunk(x, convs, keep_all=False, pre=None):
    """The five taps of the mapped input x [B, 3, h, w] (``keep_all``: all thirteen activations; ``pre``: a list that
    receives the thirteen convolution outputs in front of their ReLUs)."""
    acts = []
    for l, (w, b) in enumerate(convs):
        if l in POOL_BEFORE:
            x = F.max_pool2d(x, 2, 2)
        z = F.conv2d(x, w, b, padding=1)
        if pre is not None:
            pre.append(z.detach())
        x = F.relu(z)
        acts.append(x)
    return acts if keep_all else [acts[l] for l in TAP_LAYER]


def norm(f):
    """sqrt(sum_c f^2) [B, 1, h, w] with the derivative 0 where the sum is 0."""
    s = (f * f).sum(1, keepdim=True)
    pos = s > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, s, torch.ones_like(s))), torch.zeros_like(s))


def normalize(f):
    return f / (norm(f) + 1e-10)


def head(feats_out, feats_target, lins):
    """(value [B, 1, 1, 1], the maps d_l [B, 1, h_l, w_l])."""
    maps = [(w.view(1, -1, 1, 1) * (normalize(fo) - normalize(ft)) ** 2).sum(1, keepdim=True)
            for fo, ft, w in zip(feats_out, feats_target, lins)]
    value = maps[0].mean((2, 3), keepdim=True)
    for m in maps[1:]:
        value = value + m.mean((2, 3), keepdim=True)
    return value, maps


def lpips(img_out, img_target, convs, lins, bbox=None, shift=SHIFT, scale=SCALE):
    fo = trunk(input_map(crop(img_out, bbox), shift, scale), convs)
    ft = trunk(input_map(crop(img_target, bbox), shift, scale), convs)
    return head(fo, ft, lins)


def run(case_out, case_target, convs, lins, bbox, dtype):
    """One oracle run in ``dtype`` from float32 numpy inputs: dict with 'value' [B], 'maps' (5 arrays), 'grad'
    (dL/d img_out for L = sum_b value_b), 'acts' and 'pre' (the thirteen activations of img_out and the convolution outputs
    in front of their ReLUs), all float64 numpy."""
    cv, ln = as_tensors(convs, lins, dtype)
    x = torch.as_tensor(case_out).to(dtype).requires_grad_(True)
    t = torch.as_tensor(case_target).to(dtype)
    pre = []
    acts = trunk(input_map(crop(x, bbox)), cv, keep_all=True, pre=pre)
    ft = trunk(input_map(crop(t, bbox)), cv)
    value, maps = head([acts[l] for l in TAP_LAYER], ft, ln)
    value.sum().backward()
    f64 = lambda a: a.detach().double().numpy()      # noqa: E731
    return dict(value=f64(value).reshape(-1), maps=[f64(m) for m in maps], grad=f64(x.grad), acts=[f64(a) for a in acts],
                pre=[f64(z) for z in pre])


def rel_l2(a, ref):
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


def rel_max(a, ref):
    """max |error| sqrt(n) / L2 norm."""
    return float(np.abs(a - ref).max() * np.sqrt(ref.size) / np.linalg.norm(ref))


def sum_depth(n):
    """Float32 additions an element of the largest map (n pixels) passes through into the value: the workgroup sum
    (6 + 3), the reduce's strided sum over ceil(n / 256) partials, its workgroup sum (6 + 3) and the four tap additions."""
    nblk = -(-n // 256)
    return 9 + -(-nblk // 256) + 9 + 4


def scalar_scale(map_err, value, n, k):
    """k sum_l rms(e_l) + (d + 2) 2^-24 |value| for one image (module docstring); map_err: the five error maps of that image."""
    return k * sum(float(np.sqrt(np.mean(e * e))) for e in map_err) + (sum_depth(n) + 2) * U * abs(float(value))


def relu_decisions_agree(r32, r64):
    return all(np.array_equal(a > 0, b > 0) for a, b in zip(r32['acts'], r64['acts']))


def decision_margin(r64):
    """How far the float64 run is from every decision two float32 evaluations need not share, from float64 numbers alone
    (so the same on every machine).  The unit of layer l is ``2^-24 sqrt(K) rms(z)``, K = 9 Cin and z the layer's
    convolution outputs: the size of the rounding error of a K-term float32 sum of such terms.  Measured on the float32
    oracle on the four cases: its LARGEST error over a layer is 0.2 .. 1.6 units (2.7 .. 3.6 in the first layer, whose
    input carries the input map's roundings), its rms error 0.06 .. 0.33 units.  The margin is the smallest, over the
    layers, of min |z| / unit (the ReLU's decision) and, in front of a pool, of the smallest gap between the two largest
    activations of a 2 x 2 window with a positive maximum / unit (the pool's routing).

    The cases of the GPU test are the first seeds with a margin of at least MIN_MARGIN = 1 unit, 3 .. 16 rms errors.  A
    worst-case margin (several times the largest error) cannot be had at the size of the 'bbox' case: 1.3 million
    convolution outputs with a density of ~0.4 / rms at 0 put 3 of them within one unit of 0 in a typical draw."""
    from exavatar_release_amd.lpips import CHANNELS
    margin = np.inf
    for l, z in enumerate(r64['pre']):
        unit = U * np.sqrt(9 * CHANNELS[l][0]) * np.sqrt(np.mean(z * z))
        margin = min(margin, np.abs(z).min() / unit)
        if l + 1 in POOL_BEFORE:
            a = r64['acts'][l]
            B, C, h, w = a.shape
            win = a[:, :, :h // 2 * 2, :w // 2 * 2].reshape(B, C, h // 2, 2, w // 2, 2).transpose(0, 1, 2, 4, 3, 5)
            win = np.sort(win.reshape(B, C, h // 2, w // 2, 4), axis=-1)
            gap = (win[..., 3] - win[..., 2])[win[..., 3] > 0]
            margin = min(margin, gap.min() / unit)
    return float(margin)


MIN_MARGIN = 1.0


def check_float32_scalar(r32, r64):
    """The float32 oracle's value lies within 1 scale of the float64 one, per image."""
    for b in range(len(r64['value'])):
        errs = [m32[b] - m64[b] for m32, m64 in zip(r32['maps'], r64['maps'])]
        n = r64['maps'][0][b].size
        scale = scalar_scale(errs, r64['value'][b], n, 1)
        assert abs(r32['value'][b] - r64['value'][b]) <= scale, (b, r32['value'][b], r64['value'][b], scale)
