"""CPU tests of the face composite's host side: the entry points are exported and bound, every invalid argument fails with
its negative status and its message before any GPU work, and the Python surface refuses what it does not support.  The
ABI itself (include/exa_raster.h against its binding) is checked by tests/test_abi.py."""
import ctypes
import sys

import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import _lib, build
from tests import face_oracle as fo

BAD = ctypes.c_void_p(0x1000)      # never dereferenced: every call below fails validation first
INVALID, NULLPTR = -1, -2
ENTRY_POINTS = (('exa_face_l1_blocks', 4), ('exa_face_l1_forward', 11), ('exa_face_l1_reduce', 5),
                ('exa_face_l1_backward', 14), ('exa_composite_forward', 11), ('exa_composite_backward', 10))


def crop(*v):
    return (ctypes.c_int32 * 4)(*v)


def test_the_entry_points_are_exported_and_bound():
    lib = _lib.load()
    for name, n_args in ENTRY_POINTS:
        assert name in _lib.RASTER.signatures
        assert len(getattr(lib, name).argtypes) == n_args
    assert lib.exa_face_l1_blocks.restype is ctypes.c_int64
    assert lib.exa_raster_version() == 139
    assert build.SOURCES['face_loss.hip'] == ['-ffp-contract=off']
    module = sys.modules['exavatar_release_amd.face_loss']
    for name in ('FaceRGBLoss', 'face_composite', 'foreground_composite'):
        assert name in exa.__all__ and getattr(exa, name) is getattr(module, name)
    assert (_lib.COMPOSITE_FACE_HARD, _lib.COMPOSITE_FACE_SOFT, _lib.COMPOSITE_FOREGROUND) == (0, 1, 2)


def test_the_number_of_partials_is_the_headers():
    lib = _lib.load()
    for B, C, w, h in ((2, 3, 60, 41), (1, 3, 500, 800), (1, 3, 1, 5), (3, 1, 4, 1), (1, 3, 0, 5), (1, 3, 5, 0), (0, 3, 5, 5),
                       (1, 0, 5, 5), (-1, 3, 5, 5)):
        assert lib.exa_face_l1_blocks(B, C, w, h) == fo.blocks(B, C, w, h), (B, C, w, h)


def _fwd(lib, B=1, C=3, H=8, W=8, window=(1, 1, 4, 4), **null):
    names = ('img_out', 'face', 'img_target', 'l1_map', 'partials')
    return lib.exa_face_l1_forward(B, C, H, W, crop(*window) if window else None,
                                   *[None if null.get(n) else BAD for n in names], None)


def _bwd(lib, B=1, C=3, H=8, W=8, window=(1, 1, 4, 4), n=48, **null):
    names = ('img_out', 'face', 'img_target', 'dL_dmap', 'dL_dmean')
    ins = [None if null.get(k) else BAD for k in names]
    outs = [None if null.get(k) else BAD for k in ('dL_dimg', 'dL_dface')]
    return lib.exa_face_l1_backward(B, C, H, W, crop(*window) if window else None, *ins, n, *outs, None)


@pytest.mark.parametrize('call', [_fwd, _bwd], ids=['forward', 'backward'])
def test_bad_sizes_and_windows_are_rejected_on_the_host(call):
    lib = _lib.load()
    err = lib.exa_raster_last_error
    for size in ('B', 'C', 'H', 'W'):
        assert call(lib, **{size: -1}) == INVALID and err() == b'exa_raster: negative size', size
    assert call(lib, window=None) == NULLPTR and b'crop is NULL' in err()
    for window in ((-1, 1, 4, 4), (1, -1, 4, 4), (1, 1, -4, 4), (1, 1, 4, -4), (5, 1, 4, 4), (1, 5, 4, 4)):
        assert call(lib, window=window) == INVALID and b'crop window outside the image' in err(), window
    for n in ('img_out', 'face', 'img_target'):
        assert call(lib, dL_dmean=True, **{n: True}) == NULLPTR and b'face_l1: NULL argument' in err(), n
    assert call(lib, H=1 << 20, W=1 << 20, window=(0, 0, 4, 4)) == INVALID and b'more than 2^31 - 1 runs' in err()


def test_backward_wants_exactly_one_cotangent():
    lib = _lib.load()
    err = lib.exa_raster_last_error
    assert _bwd(lib) == INVALID and b'pass exactly one of dL_dmap / dL_dmean' in err()                  # both
    assert _bwd(lib, dL_dmap=True, dL_dmean=True) == INVALID and b'pass exactly one of dL_dmap / dL_dmean' in err()
    assert _bwd(lib, dL_dmap=True, n=-1) == INVALID and b'negative size' in err()
    with pytest.raises(RuntimeError, match='exa_raster: face_l1 backward: pass exactly one of dL_dmap / dL_dmean'):
        _lib.RASTER.check(_bwd(lib))
    assert _bwd(lib, dL_dmean=True, dL_dimg=True, dL_dface=True, img_out=True, face=True, img_target=True) == 0      # nothing wanted
    assert _bwd(lib, B=0, dL_dmean=True) == 0 and _fwd(lib, B=0) == 0                                    # nothing to do


def test_reduce_and_the_composites_check_their_arguments():
    lib = _lib.load()
    err = lib.exa_raster_last_error
    assert lib.exa_face_l1_reduce(-1, 4, BAD, BAD, None) == INVALID and b'negative size' in err()
    assert lib.exa_face_l1_reduce(1, -4, BAD, BAD, None) == INVALID and b'negative size' in err()
    assert lib.exa_face_l1_reduce(1, 4, None, BAD, None) == NULLPTR and b'face_l1 reduce: NULL argument' in err()
    assert lib.exa_face_l1_reduce(0, 0, None, None, None) == NULLPTR
    assert lib.exa_composite_forward(3, 1, 3, 8, 8, BAD, BAD, BAD, BAD, 0.9, None) == INVALID and b'unknown mode' in err()
    assert lib.exa_composite_forward(0, 1, 3, -8, 8, BAD, BAD, BAD, BAD, 0.9, None) == INVALID and b'negative size' in err()
    assert lib.exa_composite_forward(0, 1, 3, 8, 8, None, None, BAD, BAD, 0.9, None) == NULLPTR
    assert b'composite: NULL argument' in err()
    assert lib.exa_composite_forward(2, 1, 3, 8, 8, None, BAD, BAD, BAD, 0.9, None) == NULLPTR      # the foreground reads a
    assert lib.exa_composite_forward(1, 0, 3, 8, 8, None, None, None, None, 0.9, None) == 0
    assert lib.exa_composite_backward(1, 3, 8, -8, None, BAD, BAD, BAD, BAD, None) == INVALID
    assert lib.exa_composite_backward(1, 3, 8, 8, None, None, BAD, BAD, BAD, None) == NULLPTR
    assert lib.exa_composite_backward(1, 3, 8, 8, None, None, None, None, None, None) == 0          # nothing wanted


def _images(B=2, C=3, H=6, W=8):
    z = torch.zeros
    return dict(img_out=z(B, C, H, W), face_render=z(B, C + 1, H, W), img_target=z(B, C, H, W))


def test_face_rgb_loss_raises_as_specified():
    loss = exa.FaceRGBLoss()
    for reduce in (None, 'mean'):
        with pytest.raises(RuntimeError, match=r'FaceRGBLoss runs on a ROCm device only \(no CPU path\)'):
            loss(**_images(), reduce=reduce)
    for name in ('img_out', 'face_render', 'img_target'):
        a = _images()
        with pytest.raises(TypeError, match='FaceRGBLoss: %s must be a tensor' % name):
            loss(**dict(a, **{name: a[name].numpy()}))
        for other in (torch.float64, torch.float16):
            with pytest.raises(ValueError, match=r'FaceRGBLoss: %s must be float32 \(it is %s\)' % (name, other)):
                loss(**dict(a, **{name: a[name].to(other)}))
    for channels in (3, 5):
        with pytest.raises(ValueError, match='FaceRGBLoss: face_render must have one channel more than img_out'):
            loss(**dict(_images(), face_render=torch.zeros(2, channels, 6, 8)))
    with pytest.raises(ValueError, match=r'FaceRGBLoss: face_render must be \[2, 4, 6, 8\]'):
        loss(**dict(_images(), face_render=torch.zeros(2, 4, 6, 9)))
    with pytest.raises(ValueError, match='FaceRGBLoss: img_target must have the shape of img_out'):
        loss(**dict(_images(), img_target=torch.zeros(2, 3, 6, 9)))
    with pytest.raises(ValueError, match=r'FaceRGBLoss: img_out must be \[B, C, H, W\]'):
        loss(**dict(_images(), img_out=torch.zeros(3, 6, 8)))
    with pytest.raises(ValueError, match='FaceRGBLoss: img_target is data in the reference and gets no gradient; detach it'):
        loss(**dict(_images(), img_target=torch.zeros(2, 3, 6, 8, requires_grad=True)))
    with pytest.raises(ValueError, match="FaceRGBLoss: reduce must be None or 'mean'"):
        loss(**_images(), reduce='sum')


def test_the_composites_raise_as_specified():
    a = _images()
    img, face = a['img_out'], a['face_render']
    mask = torch.zeros(2, 1, 6, 8)
    for soft in (False, True):
        with pytest.raises(RuntimeError, match=r'face_composite runs on a ROCm device only \(no CPU path\)'):
            exa.face_composite(img, face, soft=soft)
    with pytest.raises(RuntimeError, match=r'foreground_composite runs on a ROCm device only \(no CPU path\)'):
        exa.foreground_composite(img, mask, img)
    with pytest.raises(ValueError, match='face_composite: face_render must have one channel more than img'):
        exa.face_composite(img, img)
    with pytest.raises(ValueError, match=r'face_composite: img must be float32 \(it is torch.float64\)'):
        exa.face_composite(img.double(), face)
    with pytest.raises(ValueError, match=r'foreground_composite: fg_mask must be \[2, 1, 6, 8\]'):
        exa.foreground_composite(img, face, img)
    with pytest.raises(ValueError, match='foreground_composite: bg_img must have the shape of fg_img'):
        exa.foreground_composite(img, mask, torch.zeros(2, 3, 6, 9))
    with pytest.raises(ValueError, match=r'foreground_composite: fg_mask must be float32'):
        exa.foreground_composite(img, mask > 0, img)
    grad = lambda t: t.clone().requires_grad_(True)      # noqa: E731
    for args in ((grad(img), face), (img, grad(face))):
        with pytest.raises(NotImplementedError, match='face_composite is forward only'):
            exa.face_composite(*args, soft=True)
    for args in ((grad(img), mask, img), (img, grad(mask), img), (img, mask, grad(img))):
        with pytest.raises(NotImplementedError, match='foreground_composite is forward only'):
            exa.foreground_composite(*args)
    with torch.no_grad():      # without grad mode the refusal is the device's
        with pytest.raises(RuntimeError, match='ROCm device only'):
            exa.face_composite(grad(img), face, soft=True)
