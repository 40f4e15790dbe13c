"""The face composite and the face-composited L1 term on the GPU (``exa.FaceRGBLoss``, ``exa.face_composite``,
``exa.foreground_composite``; csrc/face_loss.hip) against the drop-in expression on the same device -- the two reference
lines (``avatar/main/model.py:200-201``) in torch followed by ``exa.RGBLoss`` -- bit for bit, against the float64 restatement
(tests/face_oracle.py) for the mean, and against the stored float64 run of the reference's loss block.

Cases: the loss-block case (B = 2, 48 x 72, crop (0, 7, 60, 41): whole 16-byte runs, both face renders) and small random
ones: 5 x 7 and 9 x 19 (widths that allow no 16-byte access; an odd x0), 6 x 24 with an odd x0 (a pixel-by-pixel head and
tail around 16-byte runs), with a crop one pixel wide, with an aligned crop (16-byte access to the map too), 7 x 12 without
a bbox, and a bbox wholly outside the image.

Mean-mode figures measured on an MI355X are printed by the tests before they assert (pytest -s)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import _lib
from exavatar_release_amd._device import _stream_ptr
from tests import face_oracle as fo
from tests import loss_case as lc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U24 = 2.0 ** -24
W_RGB = lc.W_RGB
# name -> (seed, B, H, W, bbox (xmin, ymin, width, height) or None)
SMALL = {'5x7': (11, 2, 5, 7, (2, 1, 3, 3)),
         '9x19_odd_x0': (12, 2, 9, 19, (3, 2, 13, 9)),
         'one_pixel_wide': (13, 1, 6, 24, (5, 1, 1, 4)),
         'no_bbox': (14, 2, 7, 12, None),
         '6x24_odd_x0': (15, 2, 6, 24, (3, 1, 14, 4)),
         '6x24_aligned': (16, 1, 6, 24, (4, 0, 16, 5))}
EMPTY = ('empty', (17, 2, 5, 7, (30, 2, 5, 5)))
LOSSBLOCK = ('lossblock', 'lossblock_refined')
CASES = LOSSBLOCK + tuple(SMALL)


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and \
        bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


@functools.lru_cache(maxsize=None)
def arrays(name):
    """(numpy dict with img, face, target, fg_mask; bbox or None; crop)."""
    if name in LOSSBLOCK:
        c, tag = lc.build_case(), name[len('lossblock'):]
        a = {'img': c['scene_human' + tag], 'target': c['img'], 'fg_mask': c['mask'],
             'face': np.concatenate([c['face' + tag], c['face%s_alpha' % tag]], 1)}
        return a, lc.BBOX, lc.CROP
    seed, B, H, W, bbox = dict(SMALL, **dict([EMPTY]))[name]
    crop = fo.crop_window(bbox, H, W)
    return fo.make_case(seed, B, H, W, crop), bbox, crop


def to_dev(a, grad=False):
    return torch.from_numpy(np.array(a)).to(DEV).requires_grad_(grad)


def host_bbox(bbox, B):
    return None if bbox is None else torch.tensor([bbox] * B, dtype=torch.float32)


def dropin_map(img, face, target, bbox):
    """model.py:200-201 in torch, then exa.RGBLoss."""
    is_face = ((face[:, :3] != -1) * (face[:, 3:] == 1)).float()
    return exa.RGBLoss()(img * (1 - is_face) + face[:, :3] * is_face, target, bbox=bbox)


def cotangent(shape):
    return to_dev(np.random.RandomState(5).standard_normal(tuple(shape)).astype(np.float32))


def run_hip(a, bbox, poison=None):
    """FaceRGBLoss both ways: the map with its gradients for the fixed cotangent, the mean with those of ``mean * 0.8``."""
    img, target = np.array(a['img']), np.array(a['target'])
    if poison is not None:
        x0, y0, w, h = poison
        keep = np.zeros(img.shape, bool)
        keep[:, :, y0:y0 + h, x0:x0 + w] = True
        img, target = np.where(keep, img, np.float32('nan')), np.where(keep, target, np.float32('nan'))
    img, face, target = to_dev(img, True), to_dev(a['face'], True), to_dev(target)
    loss, bb = exa.FaceRGBLoss(), host_bbox(bbox, img.shape[0])
    out = loss(img, face, target, bbox=bb)
    gi, gf = torch.autograd.grad(out, (img, face), cotangent(out.shape))
    mean = loss(img, face, target, bbox=bb, reduce='mean')
    mi, mf = torch.autograd.grad(mean * W_RGB, (img, face))
    return {'map': out.detach(), 'd_img': gi, 'd_face': gf, 'mean': mean.detach(), 'mean_d_img': mi, 'mean_d_face': mf}


@functools.lru_cache(maxsize=None)
def results(name):
    """name -> (the module's results, the drop-in expression's), computed once and shared."""
    a, bbox, _ = arrays(name)
    hip = run_hip(a, bbox)
    img, face, target = to_dev(a['img'], True), to_dev(a['face'], True), to_dev(a['target'])
    out = dropin_map(img, face, target, host_bbox(bbox, img.shape[0]))
    gi, gf = torch.autograd.grad(out, (img, face), cotangent(out.shape), retain_graph=True)
    mi, mf = torch.autograd.grad(out.mean() * W_RGB, (img, face))
    ref = {'map': out.detach(), 'd_img': gi, 'd_face': gf, 'mean': out.detach().mean(), 'mean_d_img': mi, 'mean_d_face': mf}
    return hip, ref


def outside(crop, shape):
    x0, y0, w, h = crop
    m = torch.ones(shape, dtype=torch.bool, device=DEV)
    m[:, :, y0:y0 + h, x0:x0 + w] = False
    return m


@pytest.mark.parametrize('name', tuple(SMALL))
def test_the_small_cases_take_every_branch(name):
    a, _, (x0, y0, w, h) = arrays(name)
    face = a['face'][:, :, y0:y0 + h, x0:x0 + w]
    rgb, cov = face[:, :3], face[:, 3]
    assert (((rgb == -1).sum(1) == 1) & (cov == 1)).any(), 'no pixel with a single channel at -1 and coverage 1 in the crop'
    for v in (0.0, 0.5, 1.0):
        assert ((cov == v) & (rgb != -1).any(1)).any(), 'no coloured pixel with coverage %g in the crop' % v
    f = fo.is_face(face)
    assert f.any() and not f.all()


@pytest.mark.parametrize('name', CASES)
def test_map_and_map_mode_gradients_equal_the_drop_in_expression(name):
    (a, _, crop), (hip, ref) = arrays(name), results(name)
    assert tuple(hip['map'].shape) == (a['img'].shape[0], 3, crop[3], crop[2])
    assert torch.equal(hip['map'], ref['map'])
    assert torch.equal(hip['d_img'], ref['d_img']) and torch.equal(hip['d_face'], ref['d_face'])
    assert hip['d_img'].any() and not hip['d_img'][outside(crop, hip['d_img'].shape)].any()
    assert not hip['d_face'][outside(crop, hip['d_face'].shape)].any() and not hip['d_face'][:, 3].any()
    assert hip['d_face'][:, :3].any()


@pytest.mark.parametrize('name', CASES)
def test_only_the_crop_is_read(name):
    (a, bbox, crop), (hip, _) = arrays(name), results(name)
    poisoned = run_hip(a, bbox, poison=crop)
    assert [k for k in hip if not bits_equal(hip[k], poisoned[k])] == []


@pytest.mark.parametrize('name', CASES)
def test_mean_mode_gradients_equal_the_drop_in_expression(name):
    """Bit-equal to ``(dropin_map.mean() * 0.8).backward()`` on the device, where torch's backward of ``.mean()`` leaves
    0.8 * (1 / n) -- not 0.8 / n, which differs in the last bit for the loss-block case, ``no_bbox`` and ``6x24_aligned`` --
    and to the restatement that writes that product out."""
    (a, _, crop), (hip, ref) = arrays(name), results(name)
    assert hip['mean'].dim() == 0 and hip['mean'].dtype == torch.float32
    assert torch.equal(hip['mean_d_img'], ref['mean_d_img']) and torch.equal(hip['mean_d_face'], ref['mean_d_face'])
    d_img, d_face = fo.l1_grads(a['img'], a['face'], a['target'], crop, g_mean=np.float32(W_RGB))
    assert torch.equal(hip['mean_d_img'].cpu(), torch.from_numpy(d_img))
    assert torch.equal(hip['mean_d_face'].cpu(), torch.from_numpy(d_face))
    assert hip['mean_d_img'].any() and not hip['mean_d_img'][outside(crop, hip['mean_d_img'].shape)].any()
    assert not hip['mean_d_face'][outside(crop, hip['mean_d_face'].shape)].any() and not hip['mean_d_face'][:, 3].any()


@pytest.mark.parametrize('name', CASES)
def test_the_mean_is_within_its_rounding_of_float64(name):
    """|mean - mean64| <= (d + 2) 2^-24 mean64: the terms are non-negative, an element passes through at most d additions
    in the order include/exa_raster.h states (``face_oracle.mean_depth`` computes d from the sizes), and 2 covers the
    element's own subtraction and the final division."""
    (a, _, crop), (hip, _) = arrays(name), results(name)
    B = a['img'].shape[0]
    mean64 = fo.l1_mean64(a['img'], a['face'], a['target'], crop)
    d = fo.mean_depth(B, 3, crop[2], crop[3])
    err = abs(float(hip['mean'].double()) - mean64)
    print('%s: mean %.9g, float64 %.12g, error %.3g = %.3f of the bound (d = %d)' % (
        name, float(hip['mean']), mean64, err, err / ((d + 2) * U24 * mean64), d))
    assert mean64 > 0 and err <= (d + 2) * U24 * mean64


@pytest.mark.parametrize('name,term', zip(LOSSBLOCK, ('rgb_face', 'rgb_face_refined')))
def test_the_mean_is_the_reference_blocks_term(golden_dir, name, term):
    g = np.load(os.path.join(golden_dir, 'ref_lossblock_w0.npz'))
    hip, _ = results(name)
    got, scale = W_RGB * float(hip['mean'].double()), lc.term_scale(g, 'fused', term)
    print('%s: %.9g against %.12g, %.3f scales' % (term, got, lc.term_value(g, term), abs(got - lc.term_value(g, term)) / scale))
    assert abs(got - lc.term_value(g, term)) <= lc.FACTOR * scale


@pytest.mark.parametrize('name', CASES)
def test_two_calls_give_the_same_bits(name):
    (a, bbox, _), (hip, _) = arrays(name), results(name)
    again = run_hip(a, bbox)
    assert [k for k in hip if not bits_equal(hip[k], again[k])] == []


def test_the_empty_crop():
    a, bbox, crop = arrays('empty')
    assert crop[2] == 0 and crop[3] == 3
    hip = run_hip(a, bbox)
    assert tuple(hip['map'].shape) == (2, 3, 3, 0)
    assert bool(torch.isnan(hip['mean'])) and bool(torch.isnan(hip['map'].mean()))
    for k in ('d_img', 'd_face', 'mean_d_img', 'mean_d_face'):
        assert hip[k].shape == (2, 3 + k.endswith('face'), 5, 7) and not hip[k].any(), k


@pytest.mark.parametrize('name', CASES)
def test_the_composites(name):
    a, _, _ = arrays(name)
    img, face = to_dev(a['img'], True), to_dev(a['face'], True)
    out = exa.face_composite(img, face)
    g = cotangent(out.shape)
    gi, gf = torch.autograd.grad(out, (img, face), g)
    ri, rf = to_dev(a['img'], True), to_dev(a['face'], True)
    is_face = ((rf[:, :3] != -1) * (rf[:, 3:] == 1)).float()
    ref = ri * (1 - is_face) + rf[:, :3] * is_face
    rgi, rgf = torch.autograd.grad(ref, (ri, rf), g)
    assert torch.equal(out, ref) and torch.equal(gi, rgi) and torch.equal(gf, rgf) and not gf[:, 3].any()
    d_img, d_face = fo.hard_grads(a['face'], g.cpu().numpy())
    assert torch.equal(gi.cpu(), torch.from_numpy(d_img)) and torch.equal(gf.cpu(), torch.from_numpy(d_face))
    with torch.no_grad():
        soft = exa.face_composite(img, face, soft=True)
        fg = exa.foreground_composite(img, to_dev(a['fg_mask']), to_dev(a['target']))
    assert not soft.requires_grad and not fg.requires_grad
    assert bits_equal(soft.cpu(), torch.from_numpy(fo.soft(a['img'], a['face'])))
    want = fo.foreground(a['img'], a['fg_mask'], a['target'])
    assert bits_equal(fg.cpu(), torch.from_numpy(np.ascontiguousarray(want)))
    assert 0 < int((a['fg_mask'] > np.float32(0.9)).sum()) < a['fg_mask'].size
    again = exa.face_composite(img.detach(), face.detach(), soft=True)
    assert bits_equal(soft, again) and bits_equal(out.detach(), exa.face_composite(img, face).detach())


@pytest.mark.parametrize('name', CASES)
def test_the_raw_c_abi_writes_every_byte(name):
    """exa_face_l1_forward / _reduce / _backward on preallocated buffers filled with 0xFF: the module's results."""
    (a, _, crop), (hip, _) = arrays(name), results(name)
    lib = _lib.load()
    img, face, target = to_dev(a['img']), to_dev(a['face']), to_dev(a['target'])
    B, C, H, W = img.shape
    n = B * C * crop[2] * crop[3]
    ff = lambda *shape: torch.full(shape, float('nan'), device=DEV).view(torch.uint8).fill_(255).view(torch.float32)      # noqa: E731
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    ccrop, stream = (ctypes.c_int32 * 4)(*crop), _stream_ptr(torch.device(DEV))
    n_partials = lib.exa_face_l1_blocks(B, C, crop[2], crop[3])
    assert n_partials == fo.blocks(B, C, crop[2], crop[3])
    l1_map, partials, mean = ff(B, C, crop[3], crop[2]), ff(n_partials), ff(1)
    check = _lib.RASTER.check
    check(lib.exa_face_l1_forward(B, C, H, W, ccrop, ptr(img), ptr(face), ptr(target), ptr(l1_map), ptr(partials), stream))
    check(lib.exa_face_l1_reduce(n_partials, n, ptr(partials), ptr(mean), stream))
    assert bits_equal(l1_map, hip['map']) and bits_equal(mean[0], hip['mean'])
    assert not bool(torch.isnan(partials).any())
    g_map, g_mean = cotangent(l1_map.shape), torch.full((1,), W_RGB, dtype=torch.float32, device=DEV)
    for cot, keys in (((ptr(g_map), None), ('d_img', 'd_face')), ((None, ptr(g_mean)), ('mean_d_img', 'mean_d_face'))):
        d_img, d_face = ff(B, C, H, W), ff(B, C + 1, H, W)
        check(lib.exa_face_l1_backward(B, C, H, W, ccrop, ptr(img), ptr(face), ptr(target), cot[0], cot[1], n, ptr(d_img),
                                       ptr(d_face), stream))
        assert bits_equal(d_img, hip[keys[0]]) and bits_equal(d_face, hip[keys[1]])
        only = ff(B, C + 1, H, W)                   # one output alone
        check(lib.exa_face_l1_backward(B, C, H, W, ccrop, ptr(img), ptr(face), ptr(target), cot[0], cot[1], n, None, ptr(only),
                                       stream))
        assert bits_equal(only, d_face)
