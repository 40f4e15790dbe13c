"""CPU tests of the image-loss terms' host side (exa_ssim_*, exa_photo_loss_*, exa_l1_*): every invalid argument fails with
its negative status and its message before any GPU work, and exa_photo_loss_blocks is the header's formula.  The ABI itself
(include/exa_raster.h against its binding) is checked by tests/test_abi.py."""
import ctypes

import pytest

from exavatar_release_amd import _lib

BAD = ctypes.c_void_p(0x1000)      # never dereferenced: every call below fails validation first or has nothing to do
INVALID, NULLPTR = -1, -2
WINDOW = (1, 1, 4, 4)              # inside the 8 x 8 images below


def crop(*v):
    return (ctypes.c_int32 * 4)(*v)


def _pointers(names, null):
    unknown = set(null) - set(names)
    assert not unknown, unknown
    return [None if null.get(n) else BAD for n in names]


def _ssim_fwd(lib, N=1, H=8, W=8, **null):
    names = ('img1', 'img2', 'ssim_map', 'dm_dmu1', 'dm_dE11', 'dm_dE12')
    return lib.exa_ssim_forward(N, H, W, *_pointers(names, null), None)


def _ssim_bwd(lib, N=1, H=8, W=8, **null):
    names = ('img1', 'img2', 'dL_dmap', 'dm_dmu1', 'dm_dE11', 'dm_dE12', 'dL_dimg1')
    return lib.exa_ssim_backward(N, H, W, *_pointers(names, null), None)


def _photo_fwd(lib, B=1, C=3, H=8, W=8, window=WINDOW, **null):
    names = ('img_out', 'img_target', 'l1_weight', 'ssim_mask', 'maps_ws', 'partials')
    return lib.exa_photo_loss_forward(B, C, H, W, crop(*window) if window else None, *_pointers(names, null), None)


def _photo_grad(lib, B=1, C=3, H=8, W=8, window=WINDOW, **null):
    p = dict(zip(('img_out', 'img_target', 'l1_weight', 'ssim_mask', 'maps_ws', 'dL_dimg'),
                 _pointers(('img_out', 'img_target', 'l1_weight', 'ssim_mask', 'maps_ws', 'dL_dimg'), null)))
    return lib.exa_photo_loss_grad(B, C, H, W, crop(*window) if window else None, p['img_out'], p['img_target'],
                                   p['l1_weight'], p['ssim_mask'], 0.8, 0.2, p['maps_ws'], p['dL_dimg'], None)


def _l1_fwd(lib, B=1, C=3, H=8, W=8, window=WINDOW, **null):
    names = ('img_out', 'img_target', 'mask', 'bg', 'l1_map')
    return lib.exa_l1_forward(B, C, H, W, crop(*window) if window else None, *_pointers(names, null), None)


def _l1_bwd(lib, B=1, C=3, H=8, W=8, window=WINDOW, **null):
    names = ('img_out', 'img_target', 'mask', 'bg', 'dL_dmap', 'dL_dimg')
    return lib.exa_l1_backward(B, C, H, W, crop(*window) if window else None, *_pointers(names, null), None)


# call, its required pointers, the message of a missing one
SSIM = ((_ssim_fwd, ('img1', 'img2', 'ssim_map'), b'exa_raster: img / map is NULL'),
        (_ssim_bwd, ('img1', 'img2', 'dL_dmap', 'dm_dmu1', 'dm_dE11', 'dm_dE12', 'dL_dimg1'),
         b'exa_raster: ssim backward: NULL argument'))
CROPPED = ((_photo_fwd, ('img_out', 'img_target', 'maps_ws', 'partials'), b'exa_raster: photo loss: NULL argument'),
           (_photo_grad, ('img_out', 'img_target', 'maps_ws', 'dL_dimg'), b'exa_raster: photo loss: NULL argument'),
           (_l1_fwd, ('img_out', 'img_target', 'l1_map'), b'exa_raster: l1: NULL argument'),
           (_l1_bwd, ('img_out', 'img_target', 'dL_dmap', 'dL_dimg'), b'exa_raster: l1: NULL argument'))
IDS = {_ssim_fwd: 'ssim_forward', _ssim_bwd: 'ssim_backward', _photo_fwd: 'photo_loss_forward',
       _photo_grad: 'photo_loss_grad', _l1_fwd: 'l1_forward', _l1_bwd: 'l1_backward'}


def _ids(cases):
    return [IDS[c[0]] for c in cases]


@pytest.mark.parametrize('call,required,message', SSIM, ids=_ids(SSIM))
def test_ssim_rejects_bad_sizes_and_missing_pointers(call, required, message):
    lib = _lib.load()
    err = lib.exa_raster_last_error
    for size in ('N', 'H', 'W'):
        assert call(lib, **{size: -1}) == INVALID and err() == b'exa_raster: negative size', size
    for name in required:
        assert call(lib, **{name: True}) == NULLPTR and err() == message, name
    for size in ('N', 'H', 'W'):      # nothing to do: no pointer is looked at
        assert call(lib, **{size: 0}, **{n: True for n in required}) == 0, size


def test_ssim_forward_wants_all_three_derivative_maps_or_none():
    lib = _lib.load()
    err = lib.exa_raster_last_error
    maps = ('dm_dmu1', 'dm_dE11', 'dm_dE12')
    for missing in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)):
        null = {maps[i]: True for i in missing}
        assert _ssim_fwd(lib, **null) == INVALID, missing
        assert err() == b'exa_raster: pass all three derivative maps or none', missing
        assert _ssim_fwd(lib, N=0, **null) == INVALID, missing      # a rule of the call, whatever its size
    with pytest.raises(RuntimeError, match='exa_raster: pass all three derivative maps or none'):
        _lib.RASTER.check(_ssim_fwd(lib, dm_dE11=True))
    assert _ssim_fwd(lib, N=0) == 0 and _ssim_fwd(lib, N=0, **{m: True for m in maps}) == 0
    # a missing image is reported before the derivative maps are looked at
    assert _ssim_fwd(lib, img1=True, dm_dmu1=True) == NULLPTR and b'img / map is NULL' in err()


@pytest.mark.parametrize('call,required,message', CROPPED, ids=_ids(CROPPED))
def test_the_cropped_terms_reject_bad_sizes_windows_and_missing_pointers(call, required, message):
    lib = _lib.load()
    err = lib.exa_raster_last_error
    for size in ('B', 'C', 'H', 'W'):
        assert call(lib, **{size: -1}) == INVALID and err() == b'exa_raster: negative size', size
    assert call(lib, window=None) == NULLPTR and err() == b'exa_raster: crop is NULL'
    assert call(lib, B=-1, window=None) == INVALID and b'negative size' in err()      # the sizes come first
    # x0 < 0, y0 < 0, w < 0, h < 0, past the right edge, past the bottom edge (by one pixel, and by its origin)
    for window in ((-1, 1, 4, 4), (1, -1, 4, 4), (1, 1, -4, 4), (1, 1, 4, -4), (5, 1, 4, 4), (1, 5, 4, 4), (9, 1, 0, 4),
                   (1, 9, 4, 0)):
        assert call(lib, window=window) == INVALID and err() == b'exa_raster: crop window outside the image', window
    assert call(lib, H=4, W=9, window=(0, 0, 5, 5)) == INVALID and b'crop window outside the image' in err()
    for name in required:
        assert call(lib, **{name: True}) == NULLPTR and err() == message, name
    assert call(lib, window=(9, 1, 0, 4), **{required[0]: True}) == INVALID      # the window comes before the pointers
    nothing = {n: True for n in required}      # nothing to do: no pointer is looked at
    for empty in (dict(B=0), dict(C=0), dict(window=(1, 1, 0, 4)), dict(window=(1, 1, 4, 0)), dict(window=(8, 8, 0, 0))):
        assert call(lib, **empty, **nothing) == 0, empty


def test_the_number_of_photo_loss_partials_is_the_headers():
    lib = _lib.load()
    assert lib.exa_photo_loss_blocks.restype is ctypes.c_int64
    for B, C, w, h in ((1, 3, 32, 32), (1, 3, 33, 32), (2, 3, 60, 41), (1, 3, 500, 800), (3, 1, 1, 1), (1, 3, 0, 5),
                       (1, 3, 5, 0), (0, 3, 5, 5), (1, 0, 5, 5), (-1, 3, 5, 5), (1, -3, 5, 5), (1, 3, -5, 5), (1, 3, 5, -5),
                       (65536, 3, 32768, 32768)):
        want = 0 if min(B, C, w, h) < 0 else B * C * ((w + 31) // 32) * ((h + 31) // 32)
        assert lib.exa_photo_loss_blocks(B, C, w, h) == want, (B, C, w, h)
    assert lib.exa_photo_loss_blocks(65536, 3, 32768, 32768) == 3 << 36      # (the count is a 64-bit one)
