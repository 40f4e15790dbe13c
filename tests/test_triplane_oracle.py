"""CPU checks of the triplane oracle (tests/triplane_oracle.py) -- the restatement the HIP lookup is held to bit for bit:
in float64 it is F.grid_sample and the autograd of extract_tri_feature; in float32 it stays within a few ulps of
F.grid_sample; and it gives the known answers at texel centres, the borders and just outside them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import triplane_oracle as to


def _planes(C, H, W, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(3, C, H, W, generator=g, dtype=dtype), torch.randn(3, C, H, W, generator=g, dtype=dtype)


def _coords(N, seed, lo=-1.2, hi=1.2):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(N, 3, generator=g) * (hi - lo) + lo).float()


def _grid_sample_rows(planes, coords):
    """F.grid_sample of every row of ``coords`` on each of the three planes -> [N, 3C] (the reference's layout)."""
    feats = []
    for k, (a, b) in enumerate(to.PLANE_AXES):
        grid = torch.stack((coords[:, a], coords[:, b]), 1).to(planes.dtype)
        feats.append(F.grid_sample(planes[k, None], grid[None, :, None, :], mode='bilinear', padding_mode='zeros',
                                   align_corners=False)[0, :, :, 0])
    return torch.cat(feats).permute(1, 0)


def _extract_tri_feature(body, face, coords, is_face):
    """A restatement of extract_tri_feature on already normalised coordinates: both sets on every row they own, the face
    rows overwritten by an indexed assignment, so autograd routes their gradient to the face set alone."""
    tri = _grid_sample_rows(body, coords)
    if bool(is_face.any()):
        tri = tri.clone()
        tri[is_face] = _grid_sample_rows(face, coords[is_face])
    return tri


@pytest.mark.parametrize('C,H,W,N', [(4, 16, 16, 3000), (3, 5, 3, 500), (1, 1, 1, 200), (33, 2, 7, 300),
                                     (2, 128, 128, 4000)])
def test_float64_oracle_is_grid_sample(C, H, W, N):
    body, face = _planes(C, H, W, seed=C + H)
    coords = _coords(N, seed=N)
    is_face = torch.rand(N, generator=torch.Generator().manual_seed(1)) < 0.3
    ref = _extract_tri_feature(body, face, coords.double(), is_face).numpy()
    out = to.forward(body.numpy(), face.numpy(), coords.numpy(), is_face.numpy(), dtype=np.float64)
    assert np.abs(out - ref).max() <= 1e-12


@pytest.mark.parametrize('seg_len', [None, 32])
def test_float64_oracle_is_autograd_of_extract_tri_feature(seg_len):
    C, H, W, N = 5, 12, 9, 4000
    body, face = _planes(C, H, W, seed=3)
    body.requires_grad_(True)
    face.requires_grad_(True)
    coords = _coords(N, seed=4)
    is_face = torch.rand(N, generator=torch.Generator().manual_seed(5)) < 0.4
    g = torch.randn(N, 3 * C, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    (_extract_tri_feature(body, face, coords.double(), is_face) * g).sum().backward()
    gb, gf = to.backward(g.numpy(), coords.numpy(), is_face.numpy(), C, H, W, seg_len=seg_len, dtype=np.float64)
    scale = float(body.grad.abs().max())
    assert np.abs(gb - body.grad.numpy()).max() <= 1e-12 * scale
    assert np.abs(gf - face.grad.numpy()).max() <= 1e-12 * scale
    # lists longer than a segment exist here, so the two-level order is exercised
    assert to.list_lengths(coords.numpy(), is_face.numpy(), H, W).max() > 64


def test_float32_oracle_is_within_a_few_ulps_of_grid_sample():
    C, H, W, N = 8, 128, 128, 20000
    body, face = _planes(C, H, W, seed=7, dtype=torch.float32)
    coords = _coords(N, seed=8)
    is_face = torch.rand(N, generator=torch.Generator().manual_seed(9)) < 0.2
    ref = _extract_tri_feature(body, face, coords, is_face).numpy()
    out = to.forward(body.numpy(), face.numpy(), coords.numpy(), is_face.numpy())
    assert out.dtype == np.float32
    assert np.abs(out - ref).max() <= 2e-6


def test_float32_backward_stays_close_to_float64():
    C, H, W, N = 4, 6, 6, 5000
    coords = _coords(N, seed=10)
    is_face = torch.rand(N, generator=torch.Generator().manual_seed(11)) < 0.5
    g = torch.randn(N, 3 * C, generator=torch.Generator().manual_seed(12))
    lens = to.list_lengths(coords.numpy(), is_face.numpy(), H, W)
    assert lens.max() > 200
    g32 = to.backward(g.numpy(), coords.numpy(), is_face.numpy(), C, H, W, seg_len=32)
    g64 = to.backward(g.numpy(), coords.numpy(), is_face.numpy(), C, H, W, seg_len=None, dtype=np.float64)
    seq = to.backward(g.numpy(), coords.numpy(), is_face.numpy(), C, H, W, seg_len=None)
    for a, b, c in zip(g32, g64, seq):
        assert a.dtype == np.float32
        assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max()
        assert np.abs(c - b).max() <= 1e-4 * np.abs(b).max()
    # with every list at most one segment long the two orders agree bit for bit
    short = to.backward(g.numpy(), coords.numpy(), is_face.numpy(), C, H, W, seg_len=1 << 20)
    for a, c in zip(short, seq):
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32))


def test_known_answers():
    C, H, W = 2, 4, 5
    body, face = _planes(C, H, W, seed=13, dtype=torch.float32)
    b, f = body.numpy(), face.numpy()
    # texel centres: u = (2x + 1) / W - 1 lands on texel x with weight 1
    x, y, z = 3, 1, 2
    cx, cy, cz = (2 * x + 1) / W - 1, (2 * y + 1) / W - 1, (2 * z + 1) / H - 1
    coords = np.array([[cx, (2 * y + 1) / H - 1, cz]], dtype=np.float32)
    out = to.forward(b, f, coords, np.array([False]))
    assert np.array_equal(out[0, :C], b[0, :, y, x])
    # plane 1 = (gx, gz): column x, row z
    assert np.array_equal(out[0, C:2 * C], b[1, :, z, x])
    # the face selector reads the face set
    assert np.array_equal(to.forward(b, f, coords, np.array([True]))[0, :C], f[0, :, y, x])
    del cy
    # u = -1: ix = -0.5, half of texel 0 and half of the zero padding
    coords = np.array([[-1.0, (2 * 2 + 1) / H - 1, 0.0]], dtype=np.float32)
    out = to.forward(b, f, coords, np.array([False]))
    assert np.array_equal(out[0, :C], b[0, :, 2, 0] * np.float32(0.5))
    # u = +1: half of the last texel
    coords[0, 0] = 1.0
    out = to.forward(b, f, coords, np.array([False]))
    assert np.array_equal(out[0, :C], b[0, :, 2, W - 1] * np.float32(0.5))
    # just outside: u = -1 - 1/W puts ix at -1, all weight on the padding; further out every tap is padding
    for u in (-1 - 1 / W, 1 + 1 / W, -1.3, 2.0):
        coords = np.array([[u, u, u]], dtype=np.float32)
        assert not to.forward(b, f, coords, np.array([False])).any()
    # gradients of those rows are zero everywhere
    gb, gf = to.backward(np.ones((1, 3 * C), np.float32), coords, np.array([False]), C, H, W, seg_len=32)
    assert not gb.any() and not gf.any()
