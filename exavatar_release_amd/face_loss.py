"""HIP face composite and face-composited L1 term: the last torch piece of the image side of the training loss block, and
the two overlays of the test branch.

* ``FaceRGBLoss`` -- reference ``avatar/main/model.py:200-201, 207-208``::

      is_face = ((face_renders[:,:3] != -1) * (face_renders[:,3:] == 1)).float()
      rgb_loss(scene_human_renders['img'] * (1 - is_face) + face_renders[:,:3] * is_face, data['img'], bbox=data['bbox'])

  as ONE launch each way (``reduce=None``: the L1 map, a drop-in for the two lines) or, with ``reduce='mean'``, the map's
  ``.mean()`` from two launches forward (per-workgroup partial sums, then one workgroup that adds them) and one backward.
  The forward reads the bbox crop only; the backward walks the whole image, so that it writes the zeros outside the crop
  and in the coverage channel itself: nothing is cleared beforehand and no crop-sized intermediate exists.
* ``face_composite(img, face_render, soft=False)`` -- the same selection on the full image, differentiable in ``img`` and
  the colour channels of ``face_render``; ``soft=True`` is the overlay of ``model.py:268-271``, forward only.
* ``foreground_composite(fg_img, fg_mask, bg_img, thr=0.9)`` -- ``model.py:273-276``, forward only.

The kernels are ``csrc/face_loss.hip`` behind ``include/exa_raster.h`` (``exa_face_l1_*``, ``exa_composite_*``), which
writes out every operation and the order of every sum; ROCm device tensors only, no CPU path.  The CPU restatement that
pins them is ``tests/face_oracle.py``.  The map and every gradient equal the torch expression bit for bit (the composite
with a 0 / 1 weight is a selection); the mean is reproducible bit for bit from call to call, and within
``(d + 2) * 2^-24`` of the exact mean, d the additions an element passes through (``face_oracle.mean_depth``).  The mean's
backward scales by ``g * (1 / n)``, the rounded reciprocal first, as torch's backward of ``.mean()`` does on the device.

The calls allocate their outputs with torch and neither allocate nor synchronise inside the library; the ``bbox`` is read
on the host, as ``RGBLoss`` reads it.  No stream capture of them has been run.
"""
import torch
import torch.nn as nn

from . import _lib
from ._device import _ptr, check_no_grad, check_reduce, check_tensor, grad_in, launch
from .losses import _c_crop, _crop_window


class _FaceL1(torch.autograd.Function):
    """img_out [B, C, H, W], face [B, C + 1, H, W], img_target [B, C, H, W] (float32, contiguous, one ROCm device), crop,
    mean -> the [B, C, h, w] map or its 0-dim mean."""

    @staticmethod
    def forward(ctx, img_out, face, img_target, crop, mean):
        B, C, H, W = img_out.shape
        dev, (cw, ch) = img_out.device, crop[2:]
        ctx.crop, ctx.mean, ctx.n = crop, mean, B * C * cw * ch
        ctx.save_for_backward(img_out, face, img_target)
        if not mean:
            out = torch.empty((B, C, ch, cw), dtype=torch.float32, device=dev)
            if ctx.n:
                launch(_lib.RASTER, 'exa_face_l1_forward', dev, B, C, H, W, _c_crop(crop), _ptr(img_out), _ptr(face),
                       _ptr(img_target), _ptr(out), None)
            return out
        n_partials = int(_lib.load().exa_face_l1_blocks(B, C, cw, ch))
        partials = torch.empty(n_partials, dtype=torch.float32, device=dev)
        out = torch.empty((), dtype=torch.float32, device=dev)
        if n_partials:
            launch(_lib.RASTER, 'exa_face_l1_forward', dev, B, C, H, W, _c_crop(crop), _ptr(img_out), _ptr(face),
                   _ptr(img_target), None, _ptr(partials))
        launch(_lib.RASTER, 'exa_face_l1_reduce', dev, n_partials, ctx.n, _ptr(partials) if n_partials else None, _ptr(out))
        return out

    @staticmethod
    def backward(ctx, g):
        img_out, face, img_target = ctx.saved_tensors
        B, C, H, W = img_out.shape
        g, mean = grad_in(g), ctx.mean
        if not mean:
            g = g.expand(B, C, ctx.crop[3], ctx.crop[2]).contiguous()
            if ctx.n == 0:      # an empty map has no cotangent to point at: the launch that writes the zeros takes a mean's
                g, mean = torch.zeros((), dtype=torch.float32, device=img_out.device), True
        d_img = torch.empty_like(img_out) if ctx.needs_input_grad[0] else None
        d_face = torch.empty_like(face) if ctx.needs_input_grad[1] else None
        launch(_lib.RASTER, 'exa_face_l1_backward', img_out.device, B, C, H, W, _c_crop(ctx.crop), _ptr(img_out), _ptr(face),
               _ptr(img_target), None if mean else _ptr(g), _ptr(g) if mean else None, ctx.n, _ptr(d_img), _ptr(d_face))
        return d_img, d_face, None, None, None


def _check_images(what, named, face_name, face):
    """``named``: (name, [B, C, H, W] tensor) pairs of one shape; ``face``: the [B, C + 1, H, W] face render (or None).  The
    package's order: tensor, dtype, shape, then the device."""
    everything = list(named) + ([(face_name, face)] if face_name else [])
    for name, x in everything:
        check_tensor(what, name, x)
    name0, x0 = named[0]
    if x0.dim() != 4:
        raise ValueError('%s: %s must be [B, C, H, W] (it has %s)' % (what, name0, tuple(x0.shape)))
    for name, x in named[1:]:
        if x.shape != x0.shape:
            raise ValueError('%s: %s must have the shape of %s, %s (it has %s)' % (
                what, name, name0, tuple(x0.shape), tuple(x.shape)))
    if face_name:
        B, C, H, W = x0.shape
        if face.dim() != 4 or face.shape[1] != C + 1:
            raise ValueError('%s: %s must have one channel more than %s, %d colour channels and the coverage (it has %s)' % (
                what, face_name, name0, C, tuple(face.shape)))
        if tuple(face.shape) != (B, C + 1, H, W):
            raise ValueError('%s: %s must be [%d, %d, %d, %d] (it has %s)' % (what, face_name, B, C + 1, H, W,
                                                                             tuple(face.shape)))
    return everything


def _on_one_device(what, everything):
    anchor = everything[0]
    for name, x in everything:
        check_tensor(what, name, x, f32=False, rocm=True, on=(anchor[1], anchor[0]))


def _forward_only(what, everything):
    if torch.is_grad_enabled() and any(x.requires_grad for _, x in everything):
        raise NotImplementedError('%s is forward only (the reference composes its outputs under torch.no_grad()); detach '
                                  'the inputs or call it under torch.no_grad()' % what)


class FaceRGBLoss(nn.Module):
    """``forward(img_out, face_render, img_target, bbox=None, reduce=None)``: the L1 map ``[B, C, h, w]`` of the
    face-composited render against the target over the clamped ``bbox`` (module docstring), or with ``reduce='mean'`` its
    mean as a 0-dim tensor.  Gradients reach ``img_out`` and the colour channels of ``face_render`` (the coverage
    channel's is exactly zero); ``img_target`` is data and gets none.  An empty crop gives the empty map, or a NaN mean
    as ``torch.mean`` of the empty map does, and zero gradients."""

    def __init__(self):
        super(FaceRGBLoss, self).__init__()

    def forward(self, img_out, face_render, img_target, bbox=None, reduce=None):
        what = 'FaceRGBLoss'
        check_reduce(what, reduce)
        everything = _check_images(what, [('img_out', img_out), ('img_target', img_target)], 'face_render', face_render)
        check_no_grad(what, 'img_target', img_target)
        _on_one_device(what, everything)
        crop = _crop_window(bbox, img_out.shape[2], img_out.shape[3])
        if crop[2] == 0 or crop[3] == 0:      # a bbox outside the image: its corner may lie anywhere, the C ABI wants it inside
            crop = (0, 0, crop[2], crop[3])
        return _FaceL1.apply(img_out.contiguous(), face_render.contiguous(), img_target.contiguous(), crop,
                             reduce == 'mean')


class _HardComposite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, face):
        B, C, H, W = img.shape
        out = torch.empty_like(img)
        launch(_lib.RASTER, 'exa_composite_forward', img.device, _lib.COMPOSITE_FACE_HARD, B, C, H, W, None, _ptr(face),
               _ptr(img), _ptr(out), 0.0)
        ctx.save_for_backward(face)
        ctx.shape = (B, C, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        (face,) = ctx.saved_tensors
        B, C, H, W = ctx.shape
        g = grad_in(g).expand(B, C, H, W).contiguous()
        d_img = torch.empty_like(g) if ctx.needs_input_grad[0] else None
        d_face = torch.empty_like(face) if ctx.needs_input_grad[1] else None
        launch(_lib.RASTER, 'exa_composite_backward', face.device, B, C, H, W, None, _ptr(face), _ptr(g), _ptr(d_img),
               _ptr(d_face))
        return d_img, d_face


def face_composite(img, face_render, soft=False):
    """``img`` [B, C, H, W] with the face render [B, C + 1, H, W] laid over it.  ``soft=False``: per channel the face
    colour where it is not -1 and the coverage is 1 (model.py:200), differentiable in ``img`` and the colour channels of
    ``face_render``.  ``soft=True``: ``img * (1 - w) + face * w`` with ``w = (face != -1) * coverage`` (model.py:268-271),
    forward only: raises NotImplementedError for an input that requires grad under grad mode."""
    what = 'face_composite'
    everything = _check_images(what, [('img', img)], 'face_render', face_render)
    if soft:
        _forward_only(what, everything)
    _on_one_device(what, everything)
    if not soft:
        return _HardComposite.apply(img.contiguous(), face_render.contiguous())
    B, C, H, W = img.shape
    img, face, out = img.detach().contiguous(), face_render.detach().contiguous(), torch.empty_like(img)
    if out.numel():
        launch(_lib.RASTER, 'exa_composite_forward', img.device, _lib.COMPOSITE_FACE_SOFT, B, C, H, W, None, _ptr(face),
               _ptr(img), _ptr(out), 0.0)
    return out


def foreground_composite(fg_img, fg_mask, bg_img, thr=0.9):
    """``fg_img`` where ``fg_mask > thr``, ``bg_img`` elsewhere (model.py:273-276): images [B, C, H, W], mask [B, 1, H, W].
    Forward only: raises NotImplementedError for an input that requires grad under grad mode."""
    what = 'foreground_composite'
    check_tensor(what, 'fg_mask', fg_mask)
    everything = _check_images(what, [('fg_img', fg_img), ('bg_img', bg_img)], None, None) + [('fg_mask', fg_mask)]
    B, C, H, W = fg_img.shape
    if tuple(fg_mask.shape) != (B, 1, H, W):
        raise ValueError('%s: fg_mask must be [%d, 1, %d, %d] (it has %s)' % (what, B, H, W, tuple(fg_mask.shape)))
    _forward_only(what, everything)
    _on_one_device(what, everything)
    a, m, b = (x.detach().contiguous() for x in (fg_img, fg_mask, bg_img))
    out = torch.empty_like(a)
    if out.numel():
        launch(_lib.RASTER, 'exa_composite_forward', a.device, _lib.COMPOSITE_FOREGROUND, B, C, H, W, _ptr(a), _ptr(m),
               _ptr(b), _ptr(out), float(thr))
    return out
