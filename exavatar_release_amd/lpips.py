"""HIP LPIPS (VGG-16) perceptual loss: the reference's ``LPIPS`` class (``avatar/common/nets/loss.py:77-95``, called at
``avatar/main/model.py:199,206``) without the ``lpips`` and ``torchvision`` packages.

* ``LPIPS`` -- ``lpips.LPIPS(net='vgg')`` 0.1.4 in eval mode behind the reference's bbox crop.  The module holds the thirteen
  convolutions, the five linear heads and the scaling layer as float32 buffers (``LPIPS.from_state_dict`` /
  ``LPIPS.from_arrays``) and runs ``csrc/lpips.hip`` both ways: crop + input map, the trunk as implicit GEMMs on the
  f32-input MFMA, the head with fixed two-level sums.  ``forward(img_out, img_target, bbox=None)`` -> ``[B, 1, 1, 1]``.
  ``target_features(img_target, bbox)`` returns the five normalised target taps, which ``forward(img_out, None, bbox,
  target=feats)`` takes instead of the image: the two calls of a training iteration share target and bbox, so the target
  trunk runs once.  ``forward`` with ``img_target`` is exactly ``target_features`` followed by ``forward(target=)``.
* ``lpips_distance(feats_out, feats_target, lins)`` -- the head alone behind any trunk: lists of raw ``[B, C, h, w]``
  features (C a multiple of 4, at most 8 taps) and of ``[C]`` weights -> ``[B, 1, 1, 1]``, differentiable in ``feats_out``.

Gradients reach ``img_out`` (``feats_out``) only: the weights are frozen as ``lpips`` freezes them and ``img_target`` is
data (a target that requires grad is refused).  The backward writes ``dL/d img_out`` for the whole image in one pass, exact
zeros outside the crop included.  ONE deliberate difference from torch: at a tap pixel whose channels are all 0 torch's
``sqrt`` backward gives NaN; here the derivative of the norm is defined as 0 there (the package's "finite gradient at zero
rows" convention), so the gradient stays finite.  Every sum has a fixed order (``include/exa_raster.h``): the same bits on
every call, and a batch of B images gives the bits of B single calls.  fp32 throughout.

Internal arrays (the taps ``target_features`` returns among them) are channel-innermost, ``[B, rows, columns, C]``.  The
re-laid weights the kernels read (and the transposed, rotated ones of the backward) are non-persistent buffers, rebuilt when
the weights change.  ROCm device tensors only, no CPU path; the CPU restatement is ``tests/lpips_oracle.py``.  A crop below
16 x 16 is refused (the fifth tap would be empty; torch raises there too).
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._device import _ptr, _ptrs, _workspace, config, check_no_grad, check_tensor, grad_in, launch, need_rocm
from .losses import _c_crop, _crop_window

CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
            (512, 512), (512, 512), (512, 512))                    # (Cin, Cout) of the thirteen convolutions
FEATURE_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)   # their places in torchvision's vgg16().features
SLICE = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)                    # and the lpips slice each sits in
TAP_LAYER = (1, 3, 6, 9, 12)
TAP_CHANNELS = (64, 128, 256, 512, 512)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
MIN_CROP = 16
MAX_TAPS = 8
_CHANNEL_OF_SLOT = (0, 2, 4, 6, 1, 3, 5, 7)      # include/exa_raster.h: slot p of an 8-group holds channel 2 (p & 3) + (p >> 2)


def grad_weights(w):
    """``[Cout, Cin, 3, 3]`` -> the ``[Cin, Cout, 3, 3]`` weights whose convolution (padding 1) with dL/d(output) is
    dL/d(input): transposed and rotated by 180 degrees."""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def pack_weights(w):
    """``[Cout, Cin, 3, 3]`` (Cout % 64 == 0, Cin % 16 == 0) -> the image the convolution kernel stages
    (include/exa_raster.h): ``[Cout / 64][Cin / 16][tap][2][64][8]``."""
    co, ci = w.shape[:2]
    v = w.reshape(co // 64, 64, ci // 16, 2, 8, 9)[:, :, :, :, list(_CHANNEL_OF_SLOT), :]
    return v.permute(0, 2, 5, 3, 1, 4).contiguous()


def pack_first(w):
    """``[64, 3, 3, 3]`` -> ``[tap][ci][co]``."""
    return w.permute(2, 3, 1, 0).reshape(9, 3, 64).contiguous()


def state_dict_keys(dialect='lpips'):
    """The (weight, bias) key pairs of the thirteen convolutions in a state dict of ``lpips.LPIPS(net='vgg')``
    (``dialect='lpips'``) or of torchvision's ``vgg16()`` (``'torchvision'``)."""
    if dialect == 'lpips':
        stems = ['net.slice%d.%d' % (s, i) for s, i in zip(SLICE, FEATURE_INDEX)]
    elif dialect == 'torchvision':
        stems = ['features.%d' % i for i in FEATURE_INDEX]
    else:
        raise ValueError("LPIPS: dialect must be 'lpips' or 'torchvision' (it is %r)" % (dialect,))
    return [(s + '.weight', s + '.bias') for s in stems]


def _entry(sd, key, shape):
    if key not in sd:
        raise KeyError('LPIPS.from_state_dict: %s is missing' % key)
    x = sd[key]
    if not isinstance(x, torch.Tensor):
        raise TypeError('LPIPS.from_state_dict: %s must be a tensor' % key)
    if x.dtype != torch.float32:
        raise ValueError('LPIPS.from_state_dict: %s must be float32 (it is %s)' % (key, x.dtype))
    if tuple(x.shape) != tuple(shape):
        raise ValueError('LPIPS.from_state_dict: %s must be %s (it has %s)' % (key, list(shape), list(x.shape)))
    return x.detach()


def _crop_of(what, bbox, H, W):
    crop = _crop_window(bbox, H, W)
    if crop[2] < MIN_CROP or crop[3] < MIN_CROP:
        raise ValueError('%s: the crop is %d x %d (h x w); LPIPS needs at least %d x %d, the fifth tap would be empty' % (
            what, crop[3], crop[2], MIN_CROP, MIN_CROP))
    return crop


def _check_image(what, name, x):
    check_tensor(what, name, x)
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError('%s: %s must be [B, 3, H, W] (it has %s)' % (what, name, tuple(x.shape)))


def _floats(n, device):
    return _workspace(4 * int(n), device).view(torch.float32)


def _head_forward(taps, nts, lins, B, want_maps):
    """Per tap the head's forward, then the one reduce: (out [B, 1, 1, 1], the d maps or Nones)."""
    lib, dev = _lib.load(), taps[0].device
    partials, maps, npix = [], [], []
    for f, nt, lin in zip(taps, nts, lins):
        n, C = f.shape[1] * f.shape[2], f.shape[3]
        p = _floats(B * int(lib.exa_lpips_head_blocks(n)), dev)
        m = _floats(B * n, dev).view(B, 1, f.shape[1], f.shape[2]) if want_maps else None
        launch(_lib.RASTER, 'exa_lpips_head_forward', dev, B, n, C, _ptr(f), _ptr(nt), _ptr(lin), _ptr(m), _ptr(p))
        partials.append(p)
        maps.append(m)
        npix.append(n)
    out = torch.empty((B, 1, 1, 1), dtype=torch.float32, device=dev)      # (no view: callers may add to it in place)
    if config.poison:
        out.fill_(float('nan'))
    launch(_lib.RASTER, 'exa_lpips_head_reduce', dev, B, len(taps), _ptrs(partials), (ctypes.c_int64 * len(npix))(*npix),
           _ptr(out))
    return out, maps


def _head_backward(taps, nts, lins, B, g):
    grads = []
    for f, nt, lin in zip(taps, nts, lins):
        d = _floats(f.numel(), f.device).view(f.shape)
        launch(_lib.RASTER, 'exa_lpips_head_backward', f.device, B, f.shape[1] * f.shape[2], f.shape[3], _ptr(f), _ptr(nt),
               _ptr(lin), _ptr(g), _ptr(d))
        grads.append(d)
    return grads


class _Lpips(torch.autograd.Function):
    """img_out [B, 3, H, W] (float32, contiguous, ROCm), the module's kernel-side state, crop, want_maps, the five
    normalised target taps -> ([B, 1, 1, 1], d maps or Nones)."""

    @staticmethod
    def forward(ctx, img_out, state, crop, want_maps, *nts):
        B, _, H, W = img_out.shape
        ws, taps = state.trunk(img_out, crop)
        out, maps = _head_forward(taps, nts, state.lins, B, want_maps)
        ctx.state, ctx.crop, ctx.ws, ctx.taps, ctx.nts, ctx.shape = state, crop, ws, taps, nts, (B, H, W)
        ctx.mark_non_differentiable(*[m for m in maps if m is not None])
        return (out,) + tuple(maps)

    @staticmethod
    def backward(ctx, g, *_maps):
        B, H, W = ctx.shape
        st, dev = ctx.state, ctx.ws.device
        g = grad_in(g).expand(B, 1, 1, 1).contiguous()
        head_grads = _head_backward(ctx.taps, ctx.nts, st.lins, B, g)
        d_img = _floats(B * 3 * H * W, dev).view(B, 3, H, W)
        launch(_lib.RASTER, 'exa_lpips_trunk_backward', dev, B, H, W, _c_crop(ctx.crop), st.shift_scale, _ptrs(st.packed_t),
               _ptrs(head_grads), _ptr(ctx.ws), ctx.ws.numel(), _ptr(d_img))
        return (d_img,) + (None,) * (3 + len(ctx.nts))


class _KernelState:
    """What the kernels read, as of one state of the module's buffers."""

    def __init__(self, mod):
        self.packed = [getattr(mod, '_packed%d' % l) for l in range(13)]
        self.packed_t = [getattr(mod, '_packed_t%d' % l) for l in range(13)]
        self.biases = [getattr(mod, 'conv%d_bias' % l) for l in range(13)]
        self.lins = [getattr(mod, 'lin%d' % t) for t in range(5)]
        self.shift_scale = (ctypes.c_float * 6)(*(mod.shift.tolist() + mod.scale.tolist()))

    def trunk(self, img, crop):
        """The trunk's forward over the crop of ``img``: (workspace, the five taps as views of it)."""
        B, _, H, W = img.shape
        dev = img.device
        ws = _workspace(_lib.lpips_workspace_size(B, crop[3], crop[2]), dev)
        launch(_lib.RASTER, 'exa_lpips_trunk_forward', dev, B, H, W, _c_crop(crop), _ptr(img), self.shift_scale,
               _ptrs(self.packed), _ptrs(self.biases), _ptr(ws), ws.numel())
        lib, taps = _lib.load(), []
        for t in range(5):
            off, shape = ctypes.c_uint64(), (ctypes.c_int32 * 3)()
            _lib.RASTER.check(lib.exa_lpips_tap_layout(B, crop[3], crop[2], t, ctypes.byref(off), shape))
            n = B * shape[0] * shape[1] * shape[2]
            taps.append(ws[off.value:off.value + 4 * n].view(torch.float32).view(B, shape[0], shape[1], shape[2]))
        return ws, taps


class LPIPS(nn.Module):
    """``forward(img_out, img_target, bbox=None, target=None)`` -> ``[B, 1, 1, 1]`` (module docstring)."""

    def __init__(self, convs, lins, shift=SHIFT, scale=SCALE):
        super(LPIPS, self).__init__()
        what = 'LPIPS.from_arrays'
        if len(convs) != 13 or len(lins) != 5:
            raise ValueError('%s: 13 (weight, bias) pairs and 5 lin weights are needed (there are %d and %d)' % (
                what, len(convs), len(lins)))
        f32 = lambda x: x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x))      # noqa: E731
        for l, ((ci, co), (w, b)) in enumerate(zip(CHANNELS, convs)):
            w, b = f32(w), f32(b)
            for name, x, shape in (('convs[%d] weight' % l, w, (co, ci, 3, 3)), ('convs[%d] bias' % l, b, (co,))):
                if x.dtype != torch.float32:
                    raise ValueError('%s: %s must be float32 (it is %s)' % (what, name, x.dtype))
                if tuple(x.shape) != shape:
                    raise ValueError('%s: %s must be %s (it has %s)' % (what, name, list(shape), list(x.shape)))
            self.register_buffer('conv%d_weight' % l, w.detach().clone().contiguous())
            self.register_buffer('conv%d_bias' % l, b.detach().clone().contiguous())
        for t, (C, x) in enumerate(zip(TAP_CHANNELS, lins)):
            x = f32(x)
            if x.dtype != torch.float32:
                raise ValueError('%s: lins[%d] must be float32 (it is %s)' % (what, t, x.dtype))
            if x.numel() != C:
                raise ValueError('%s: lins[%d] must have %d elements (it has %s)' % (what, t, C, list(x.shape)))
            self.register_buffer('lin%d' % t, x.detach().reshape(C).clone())
        self.register_buffer('shift', torch.as_tensor(shift, dtype=torch.float32).reshape(3).clone())
        self.register_buffer('scale', torch.as_tensor(scale, dtype=torch.float32).reshape(3).clone())
        for l in range(13):
            self.register_buffer('_packed%d' % l, None, persistent=False)
            self.register_buffer('_packed_t%d' % l, None, persistent=False)
        self._state, self._state_key = None, None

    @classmethod
    def from_arrays(cls, convs, lins, shift=SHIFT, scale=SCALE):
        """``convs``: 13 (weight [Cout, Cin, 3, 3], bias [Cout]) pairs; ``lins``: 5 weights of 64, 128, 256, 512, 512
        elements; float32 tensors or numpy arrays."""
        return cls(convs, lins, shift, scale)

    @classmethod
    def from_state_dict(cls, sd):
        """From the state dict of ``lpips.LPIPS(net='vgg')`` (``net.slice*.N.*``, ``lin{t}.model.1.weight`` or
        ``lins.{t}.model.1.weight``, optional ``scaling_layer.shift`` / ``.scale``) or of torchvision's ``vgg16()``
        (``features.N.*``) plus the five lin weights."""
        dialect = 'torchvision' if any(k.startswith('features.') for k in sd) else 'lpips'
        convs = [(_entry(sd, kw, (co, ci, 3, 3)), _entry(sd, kb, (co,)))
                 for (ci, co), (kw, kb) in zip(CHANNELS, state_dict_keys(dialect))]
        lins = []
        for t, C in enumerate(TAP_CHANNELS):
            key = 'lin%d.model.1.weight' % t
            if key not in sd and 'lins.%d.model.1.weight' % t in sd:
                key = 'lins.%d.model.1.weight' % t
            lins.append(_entry(sd, key, (1, C, 1, 1)))
        shift = _entry(sd, 'scaling_layer.shift', (1, 3, 1, 1)) if 'scaling_layer.shift' in sd else SHIFT
        scale = _entry(sd, 'scaling_layer.scale', (1, 3, 1, 1)) if 'scaling_layer.scale' in sd else SCALE
        return cls(convs, lins, shift, scale)

    def _weights(self):
        return [getattr(self, 'conv%d_weight' % l) for l in range(13)]

    def _kernel_state(self):
        """The re-laid weights, rebuilt when a weight was replaced, moved or written in place."""
        named = self._weights() + [getattr(self, 'conv%d_bias' % l) for l in range(13)] + \
            [getattr(self, 'lin%d' % t) for t in range(5)] + [self.shift, self.scale]
        key = tuple((x.data_ptr(), x._version, x.device, x.dtype) for x in named)
        if key != self._state_key:
            for x in named:
                if x.dtype != torch.float32:
                    raise ValueError('LPIPS: the weights must be float32 (one is %s)' % x.dtype)
            for l, w in enumerate(self._weights()):
                setattr(self, '_packed%d' % l, pack_first(w) if l == 0 else pack_weights(w))
                setattr(self, '_packed_t%d' % l, pack_first(w) if l == 0 else pack_weights(grad_weights(w)))
            self._state, self._state_key = _KernelState(self), key
        return self._state

    def _check(self, what, name, img, bbox):
        _check_image(what, name, img)
        return _crop_of(what, bbox, img.shape[2], img.shape[3])

    def target_features(self, img_target, bbox=None):
        """The five normalised taps of ``img_target`` over the clamped ``bbox``: ``[B, h >> t, w >> t, C_t]`` each."""
        what = 'LPIPS.target_features'
        crop = self._check(what, 'img_target', img_target, bbox)
        check_no_grad(what, 'img_target', img_target)
        need_rocm(img_target.device, 'LPIPS')
        check_tensor(what, 'img_target', img_target, f32=False, on=(self.shift, 'the weights'))
        return self._target_features(img_target, crop)

    def _target_features(self, img_target, crop):
        _, taps = self._kernel_state().trunk(img_target.detach().contiguous(), crop)
        feats = []
        for f in taps:
            nt = _floats(f.numel(), f.device).view(f.shape)
            launch(_lib.RASTER, 'exa_lpips_normalize', f.device, f.numel() // f.shape[3], f.shape[3], _ptr(f), _ptr(nt))
            feats.append(nt)
        return feats

    def forward(self, img_out, img_target, bbox=None, target=None, return_maps=False):
        """``target``: what ``target_features(img_target, bbox)`` returned, instead of ``img_target`` (then None).
        ``return_maps=True`` also returns the five per-pixel maps ``d_l`` ``[B, 1, h_l, w_l]`` (no gradient)."""
        what = 'LPIPS'
        crop = self._check(what, 'img_out', img_out, bbox)
        B = img_out.shape[0]
        if target is None:
            _check_image(what, 'img_target', img_target)
            if img_target.shape != img_out.shape:
                raise ValueError('%s: img_target must have the shape of img_out, %s (it has %s)' % (
                    what, tuple(img_out.shape), tuple(img_target.shape)))
            check_no_grad(what, 'img_target', img_target)
        else:
            if img_target is not None:
                raise ValueError('%s: pass img_target or target, not both' % what)
            target = list(target)
            if len(target) != 5:
                raise ValueError('%s: target must be the five taps of target_features (it has %d)' % (what, len(target)))
            for t, f in enumerate(target):
                check_tensor(what, 'target[%d]' % t, f)
                want = (B, crop[3] >> t, crop[2] >> t, TAP_CHANNELS[t])
                if tuple(f.shape) != want:
                    raise ValueError('%s: target[%d] must be %s, the tap of this crop (it has %s)' % (
                        what, t, list(want), list(f.shape)))
                check_no_grad(what, 'target[%d]' % t, f)
        need_rocm(img_out.device, what)
        for name, x in ([('img_target', img_target)] if target is None else
                        [('target[%d]' % t, f) for t, f in enumerate(target)]) + [('the weights', self.shift)]:
            check_tensor(what, name, x, f32=False, on=(img_out, 'img_out'))
        if target is None:
            target = self._target_features(img_target, crop)
        res = _Lpips.apply(img_out.contiguous(), self._kernel_state(), crop, bool(return_maps),
                           *[f.detach().contiguous() for f in target])
        return (res[0], list(res[1:])) if return_maps else res[0]


class _Distance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lins, feats_target, *feats_out):
        B = feats_out[0].shape[0]
        taps = [f.detach().permute(0, 2, 3, 1).contiguous() for f in feats_out]
        nts = []
        for f in feats_target:
            f = f.detach().permute(0, 2, 3, 1).contiguous()
            nt = _floats(f.numel(), f.device).view(f.shape)
            launch(_lib.RASTER, 'exa_lpips_normalize', f.device, f.numel() // f.shape[3], f.shape[3], _ptr(f), _ptr(nt))
            nts.append(nt)
        out, _ = _head_forward(taps, nts, lins, B, False)
        ctx.lins, ctx.taps, ctx.nts, ctx.B = lins, taps, nts, B
        return out

    @staticmethod
    def backward(ctx, g):
        g = grad_in(g).expand(ctx.B, 1, 1, 1).contiguous()
        grads = _head_backward(ctx.taps, ctx.nts, ctx.lins, ctx.B, g)
        return (None, None) + tuple(d.permute(0, 3, 1, 2) for d in grads)


def lpips_distance(feats_out, feats_target, lins):
    """The LPIPS head alone (module docstring): raw features ``[B, C, h, w]`` per tap, ``lins`` the ``[C]`` (or
    ``[1, C, 1, 1]``) weights -> ``[B, 1, 1, 1]``; gradients reach ``feats_out`` only."""
    what = 'lpips_distance'
    feats_out, feats_target, lins = list(feats_out), list(feats_target), list(lins)
    n = len(feats_out)
    if not 1 <= n <= MAX_TAPS or len(feats_target) != n or len(lins) != n:
        raise ValueError('%s: 1 .. %d taps with one target and one weight each are needed (there are %d, %d, %d)' % (
            what, MAX_TAPS, n, len(feats_target), len(lins)))
    for t in range(n):
        for name, x in (('feats_out[%d]' % t, feats_out[t]), ('feats_target[%d]' % t, feats_target[t]), ('lins[%d]' % t, lins[t])):
            check_tensor(what, name, x)
    B = feats_out[0].shape[0] if feats_out[0].dim() == 4 else -1
    for t in range(n):
        f = feats_out[t]
        if f.dim() != 4 or f.shape[0] != B or f.shape[1] % 4 != 0 or f.shape[1] == 0 or f.shape[2] * f.shape[3] == 0:
            raise ValueError('%s: feats_out[%d] must be [B, C, h, w] with C a multiple of 4 and pixels (it has %s)' % (
                what, t, tuple(f.shape)))
        if feats_target[t].shape != f.shape:
            raise ValueError('%s: feats_target[%d] must have the shape of feats_out[%d], %s (it has %s)' % (
                what, t, t, tuple(f.shape), tuple(feats_target[t].shape)))
        if lins[t].numel() != f.shape[1]:
            raise ValueError('%s: lins[%d] must have %d elements (it has %s)' % (what, t, f.shape[1], tuple(lins[t].shape)))
        check_no_grad(what, 'feats_target[%d]' % t, feats_target[t])
        check_no_grad(what, 'lins[%d]' % t, lins[t], 'a frozen weight')
    need_rocm(feats_out[0].device, what)
    for t in range(n):
        for name, x in (('feats_out[%d]' % t, feats_out[t]), ('feats_target[%d]' % t, feats_target[t]), ('lins[%d]' % t, lins[t])):
            check_tensor(what, name, x, f32=False, on=(feats_out[0], 'feats_out[0]'))
    return _Distance.apply([x.detach().reshape(-1).contiguous() for x in lins], feats_target, *feats_out)
