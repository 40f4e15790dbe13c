"""CPU tests of tests/face_oracle.py, the numpy restatement that pins the face-composite kernels: on the loss-block case
(``tests/loss_case.build_case``) its float32 arrays equal the reference's expressions (``avatar/main/model.py:200-201,
268-276`` with ``RGBLoss``'s crop, loss.py:19-29), evaluated by torch on the CPU, bit for bit -- the map, its gradients for
a random cotangent and for the mean, the soft and the foreground overlays -- and the case exercises every branch."""
import numpy as np
import pytest
import torch

from tests import face_oracle as fo
from tests import loss_case as lc

TAGS = ('', '_refined')


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


def values_equal(a, b):
    """Equal as numbers: a zero's sign is free (torch forms x * 0 where the restatement selects)."""
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a, b)


@pytest.fixture(scope='module')
def case():
    return lc.build_case()


def arrays(case, tag):
    face = np.concatenate([case['face' + tag], case['face%s_alpha' % tag]], 1)
    return case['scene_human' + tag], face, case['img']


def reference_map(img, face, target):
    """model.py:200-201 with RGBLoss's crop (loss.py:19-29) in torch: (map, the leaves)."""
    img = torch.from_numpy(np.array(img)).requires_grad_(True)
    face = torch.from_numpy(np.array(face)).requires_grad_(True)
    target = torch.from_numpy(np.array(target))
    is_face = ((face[:, :3] != -1) * (face[:, 3:] == 1)).float()
    comp = img * (1 - is_face) + face[:, :3] * is_face
    x0, y0, w, h = lc.CROP
    out = torch.abs(comp[:, :, y0:y0 + h, x0:x0 + w] - target[:, :, y0:y0 + h, x0:x0 + w])
    return out, img, face


@pytest.mark.parametrize('tag', TAGS)
def test_the_map_and_its_gradients_equal_the_reference_expression(case, tag):
    img, face, target = arrays(case, tag)
    assert fo.crop_window(lc.BBOX, lc.H, lc.W) == lc.CROP
    out, ti, tf = reference_map(img, face, target)
    assert bits_equal(fo.l1_map(img, face, target, lc.CROP), out.detach().numpy())
    g = np.random.RandomState(7).standard_normal(tuple(out.shape)).astype(np.float32)
    gi, gf = torch.autograd.grad(out, (ti, tf), torch.from_numpy(g), retain_graph=True)
    d_img, d_face = fo.l1_grads(img, face, target, lc.CROP, g_map=g)
    assert bits_equal(d_img, gi.numpy()) and bits_equal(d_face, gf.numpy())
    assert not d_face[:, 3].any() and d_img.any() and d_face.any()
    gi, gf = torch.autograd.grad(out.mean() * lc.W_RGB, (ti, tf))
    d_img, d_face = fo.l1_grads(img, face, target, lc.CROP, g_mean=np.float32(lc.W_RGB), reciprocal=False)      # torch on the CPU
    assert bits_equal(d_img, gi.numpy()) and bits_equal(d_face, gf.numpy())
    r_img, r_face = fo.l1_grads(img, face, target, lc.CROP, g_mean=np.float32(lc.W_RGB))      # the kernel's: one bit apart here
    assert not values_equal(r_img, d_img) and np.allclose(r_img, d_img, rtol=2.0 ** -22, atol=0)
    assert np.array_equal(r_img != 0, d_img != 0) and np.array_equal(r_face != 0, d_face != 0)
    assert abs(fo.l1_mean64(img, face, target, lc.CROP) - float(out.detach().double().mean())) < 1e-6


@pytest.mark.parametrize('tag', TAGS)
def test_the_overlays_equal_the_reference_expressions(case, tag):
    img, face, _ = arrays(case, tag)
    ti, tf = torch.from_numpy(np.array(img)), torch.from_numpy(np.array(face))
    is_face = (tf[:, :3] != -1).float() * tf[:, 3:]                                    # model.py:268-269
    assert bits_equal(fo.soft(img, face), (ti * (1 - is_face) + tf[:, :3] * is_face).numpy())
    is_face = ((tf[:, :3] != -1) * (tf[:, 3:] == 1)).float()                           # model.py:200-201
    assert values_equal(fo.hard(img, face), (ti * (1 - is_face) + tf[:, :3] * is_face).numpy())
    fg, mask = torch.from_numpy(np.array(case['human' + tag])), torch.from_numpy(np.array(case['mask']))
    is_fg = mask > 0.9                                                                 # model.py:273-274
    assert bits_equal(fo.foreground(case['human' + tag], case['mask'], img), (is_fg * fg + (1 - is_fg.float()) * ti).numpy())
    assert 0 < int(is_fg.sum()) < is_fg.numel()


@pytest.mark.parametrize('tag', TAGS)
def test_the_case_takes_every_branch(case, tag):
    _, face, _ = arrays(case, tag)
    x0, y0, w, h = lc.CROP
    f, cov, rgb = fo.is_face(face), face[:, 3:], face[:, :3]
    inside = np.zeros(f.shape, bool)
    inside[:, :, y0:y0 + h, x0:x0 + w] = True
    assert (f & inside).any(), 'no face pixel with f = 1 inside the crop'
    assert f[:, :, :, 60:].any() and x0 + w == 60, 'no face pixel outside the crop (x >= 60)'
    one = ((rgb == -1).sum(1) == 1) & (cov[:, 0] == 1)
    assert (one & inside[:, 0]).any(), 'no pixel with one channel at -1 and coverage 1 inside the crop'
    assert ((cov == 0.5) & (rgb != -1) & inside).any(), 'no pixel with coverage 0.5 inside the crop'
    assert ((rgb == -1).all(1) & (cov[:, 0] == 0)).any(), 'no background pixel'


def test_the_work_split_follows_the_header():
    assert fo.blocks(2, 3, 60, 41) == (2 * 41 * 16 + 255) // 256 == 6
    assert fo.blocks(1, 3, 1, 5) == 1 and fo.blocks(1, 3, 0, 5) == 0 and fo.blocks(0, 3, 4, 4) == 0
    assert fo.mean_depth(2, 3, 60, 41) == 12 + 9 + 1 + 9
    assert fo.blocks(1, 3, 500, 800) == 394 and fo.mean_depth(1, 3, 500, 800) == 12 + 9 + 2 + 9      # two per thread at most
