"""CPU checks of the Phong-shaded render: the float64 oracle tests/shade_oracle.py against answers worked out by hand,
the package's composite against the reference's four lines, and the argument checks of the shaded entry points that
return before any launch (their symbols and struct layout: tests/test_abi.py)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from exavatar_release_amd import _lib, mesh
from tests import mesh_oracle as mo
from tests import shade_oracle as so

H, W = 12, 16
FOCAL, PRINCPT = 10.0, (8.0, 6.0)


def _triangle(flip):
    """A large triangle in the plane z = 2 that covers the whole H x W image; ``flip`` reverses its winding."""
    v = torch.tensor([[[-30.0, -30.0, 2.0], [30.0, -30.0, 2.0], [0.0, 30.0, 2.0]]], dtype=torch.float64)
    f = torch.tensor([[0, 1, 2]] if flip else [[0, 2, 1]])
    return v, f


def _cam():
    return torch.tensor([[FOCAL, FOCAL]], dtype=torch.float64), torch.tensor([PRINCPT], dtype=torch.float64)


def _pixel_points(z=2.0):
    """Camera-space point on the plane z = 2 seen through every pixel centre: [H, W, 3]."""
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    return np.stack(((jj - PRINCPT[0]) * z / FOCAL, (ii - PRINCPT[1]) * z / FOCAL, np.full_like(jj, z)), -1)


def test_triangle_windings_light_one_side_only():
    focal, princpt = _cam()
    # (v1 - v0) x (v2 - v0) of [0, 2, 1] points along -z (at the camera): cos = n^ . l^ = 2 / |l|, l = (0, -1, 0) - p
    v, f = _triangle(False)
    n, _ = so.vertex_normals(v, f)
    assert np.allclose(n[0], [[0, 0, -1]] * 3)
    img, cos, fr = so.render(v, f, focal, princpt, H, W)
    assert bool((fr['face'] == 0).all())
    p = _pixel_points()
    lnorm = np.linalg.norm(np.array([0.0, -1.0, 0.0]) - p, axis=-1)
    want = 0.5 + 0.3 * 2.0 / lnorm
    assert np.abs(img[0].numpy() - want[..., None]).max() < 1e-12
    assert float(cos.min()) > 0
    # the other winding faces away from the light everywhere: ambient only, exactly
    v, f = _triangle(True)
    img, cos, _ = so.render(v, f, focal, princpt, H, W)
    assert float(cos.max()) < 0
    assert bool((img == 0.5).all())


def test_icosphere_normals_are_radial():
    err = []
    for level in (3, 4):
        v, f = mo.icosphere(level)
        n, _ = so.vertex_normals(v * 0.7 + torch.tensor([0.1, -0.2, 3.0], dtype=torch.float64), f)
        radial = (v / v.norm(dim=1, keepdim=True)).numpy()
        assert np.abs(np.linalg.norm(n[0], axis=1) - 1).max() < 1e-12
        assert float((n[0] * radial).sum(1).min()) > 0.9998
        err.append(np.abs(n[0] - radial).max())
    # the departure from radial is the sphere's discretisation: ~1e-2 at level 3, halved by each subdivision
    assert err[0] < 2e-2 and err[1] < 0.6 * err[0]


def test_specular_mirror_gives_light_times_material():
    # light at the camera, a face-on plane: at the pixel on the optical axis l^ = v^ = n^ = (0, 0, -1), so r = v^ and the
    # specular term is Ls Ms whatever the shininess; everywhere else it is smaller
    focal = torch.tensor([[FOCAL, FOCAL]], dtype=torch.float64)
    princpt = torch.tensor([[8.5, 6.5]], dtype=torch.float64)         # the centre of pixel (6, 8)
    v, f = _triangle(False)
    sh = dict(light_location=(0.0, 0.0, 0.0), lights=(0.0, 0.0, (0.2, 0.4, 0.6)), materials=(1.0, 1.0, 0.5),
              shininess=50.0)
    img, cos, _ = so.render(v, f, focal, princpt, H, W, **sh)
    want = np.array([0.1, 0.2, 0.3])
    assert np.abs(img[0, 6, 8].numpy() - want).max() < 1e-12
    assert abs(float(cos[0, 6, 8]) - 1) < 1e-15
    others = img[0].numpy().copy()
    others[6, 8] = 0
    assert (others < want - 1e-6).all()


def test_shininess_zero_with_the_face_turned_away_gives_full_specular():
    focal, princpt = _cam()
    v, f = _triangle(True)                      # cos < 0 everywhere: [cos > 0] = 0, 0 ** 0 = 1
    sh = dict(lights=(0.5, 0.3, (0.2, 0.1, 0.05)), materials=(1.0, 1.0, 1.0), shininess=0.0)
    img, cos, _ = so.render(v, f, focal, princpt, H, W, **sh)
    assert float(cos.max()) < 0
    assert np.abs(img[0].numpy() - np.array([0.7, 0.6, 0.55])).max() < 1e-15
    img8, _, _ = so.render(v, f, focal, princpt, H, W, **dict(sh, shininess=8.0))
    assert bool((img8 == 0.5).all())            # 0 ** 8 = 0: ambient only


def test_degenerate_faces_give_zero_normals_and_ambient_only():
    # vertices 3..5 belong to one collinear face only; the first triangle is also listed with the other winding, so the
    # cross products of its vertices cancel exactly and the visible (lower-index) face shades with n = 0
    v = torch.tensor([[[-30.0, -30.0, 2.0], [30.0, -30.0, 2.0], [0.0, 30.0, 2.0],
                       [0.1, 0.1, 1.0], [0.2, 0.2, 1.0], [0.3, 0.3, 1.0]]], dtype=torch.float64)
    f = torch.tensor([[0, 2, 1], [0, 1, 2], [3, 4, 5]])
    n, raw = so.vertex_normals(v, f)
    assert np.all(raw[0] == 0) and np.all(n[0] == 0)
    focal, princpt = _cam()
    for sh, want in ((so.REFERENCE, 0.5), (dict(materials=(1.0, 1.0, 1.0), shininess=0.0), 0.7),
                     (dict(materials=(1.0, 1.0, 1.0), shininess=3.0), 0.5)):
        img, cos, fr = so.render(v, f, focal, princpt, H, W, **sh)
        assert bool((fr['face'] <= 1).all()) and bool((cos == 0).all())        # either copy: the z tie is rounding
        assert np.abs(img.numpy() - want).max() < 1e-15


def test_background_pixels_get_the_background_colour():
    v = torch.tensor([[[-0.2, -0.2, 2.0], [0.2, -0.2, 2.0], [0.0, 0.2, 2.0]]], dtype=torch.float64)
    f = torch.tensor([[0, 1, 2]])
    focal, princpt = _cam()
    img, _, fr = so.render(v, f, focal, princpt, H, W, background=(0.2, 0.3, 0.4))
    bg = fr['face'] < 0
    assert 0 < int((~bg).sum()) < H * W
    assert bool((img[bg] == torch.tensor([0.2, 0.3, 0.4], dtype=torch.float64)).all())
    assert bool((img[~bg] >= 0.5).all())


@pytest.mark.parametrize('dtype', [np.float32, np.uint8, np.float64])
@pytest.mark.parametrize('blend_ratio', [1.0, 0.6])
def test_composite_is_the_reference_composite(dtype, blend_ratio):
    g = np.random.default_rng(3)
    images = torch.from_numpy(g.uniform(0.5, 0.8, (1, H, W, 3)).astype(np.float32))
    pix_to_face = torch.from_numpy(np.where(g.uniform(size=(1, H, W)) < 0.3, -1, 7))
    zbuf = torch.where(pix_to_face >= 0, torch.tensor(2.5), torch.tensor(-1.0))[..., None]
    bkg = g.uniform(0, 255, (H, W, 3)).astype(dtype)
    bkg = bkg[..., ::-1]                          # the fitting caller's BGR view: negative strides
    want = so.reference_composite(images, zbuf, bkg, blend_ratio)
    is_bkg = (pix_to_face[0] == -1)[..., None].float().numpy()
    got = mesh._composite(images[0].numpy(), is_bkg, bkg, blend_ratio)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    # worked by hand: background pixels are bkg, covered ones (render r) r * a + bkg / 255 * (1 - a), times 255
    bg = pix_to_face[0].numpy() == -1
    assert np.array_equal(got[bg], bkg[bg].astype(got.dtype))
    r = images[0].numpy().astype(np.float64)
    hand = (r * blend_ratio + bkg.astype(np.float64) / 255 * (1 - blend_ratio)) * 255
    assert np.abs(got[~bg] - hand[~bg]).max() < 1e-3


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def _shading(shininess=0.0):
    sh = _lib.ExaMeshShading()
    sh.light_location[:] = [0.0, -1.0, 0.0]
    sh.light_ambient[:] = sh.light_diffuse[:] = sh.light_specular[:] = [0.5, 0.3, 0.2]
    sh.material_ambient[:] = sh.material_diffuse[:] = [1.0, 1.0, 1.0]
    sh.shininess = shininess
    sh.background[:] = [1.0, 1.0, 1.0]
    return sh


FAKE = ctypes.c_void_p(1 << 20)       # never dereferenced: every call below fails its checks before any launch


def _geom(N=1, H=8, W=8):
    return _lib.ExaMeshGeometry(N, 3, 1, H, W, FAKE.value, FAKE.value, FAKE.value, FAKE.value)


def _shaded(g, sh, image=FAKE):
    return _lib.load().exa_mesh_forward_shaded(ctypes.byref(g), ctypes.byref(sh) if sh is not None else None, FAKE, FAKE,
                                               FAKE, FAKE, None, image, None)


def test_shaded_forward_rejects_invalid_arguments_without_a_gpu():
    lib = _lib.load()
    assert _shaded(_geom(N=0), _shading()) == -1
    assert _shaded(_geom(N=-1), _shading()) == -1
    assert _shaded(_geom(), _shading(), image=None) == -2
    assert b'image' in lib.exa_mesh_last_error()
    assert _shaded(_geom(), _shading(-0.5)) == -1
    assert b'shininess' in lib.exa_mesh_last_error()
    assert _shaded(_geom(), _shading(float('nan'))) == -1
    assert _shaded(_geom(), None) == -2
    assert _shaded(_geom(H=8193), _shading()) == -1
    assert b'8192' in lib.exa_mesh_last_error()
    assert lib.exa_mesh_forward_shaded(None, ctypes.byref(_shading()), FAKE, FAKE, FAKE, FAKE, None, FAKE, None) == -2


def test_vertex_normals_rejects_invalid_arguments_without_a_gpu():
    lib = _lib.load()
    # focal / princpt are not used: NULL is fine there
    g = _lib.ExaMeshGeometry(1, 3, 1, 0, 0, FAKE.value, FAKE.value, None, None)
    assert lib.exa_mesh_vertex_normals(ctypes.byref(g), FAKE, FAKE, None, None) == -2
    assert lib.exa_mesh_vertex_normals(ctypes.byref(g), None, FAKE, FAKE, None) == -2
    assert lib.exa_mesh_vertex_normals(ctypes.byref(g), FAKE, None, FAKE, None) == -2
    assert lib.exa_mesh_vertex_normals(None, FAKE, FAKE, FAKE, None) == -2
    for N, V in ((0, 3), (-1, 3), (1, -3)):
        g = _lib.ExaMeshGeometry(N, V, 1, 0, 0, FAKE.value, FAKE.value, None, None)
        assert lib.exa_mesh_vertex_normals(ctypes.byref(g), FAKE, FAKE, FAKE, None) == -1


def test_python_entry_points_refuse_cpu_tensors_and_bad_shading():
    v, f = _triangle(False)
    cam = {'focal': torch.tensor([FOCAL, FOCAL]), 'princpt': torch.tensor(PRINCPT)}
    with pytest.raises(RuntimeError, match='ROCm'):
        mesh.shade_mesh(v.float(), f.numpy(), cam, (H, W))
    with pytest.raises(RuntimeError, match='ROCm'):
        mesh.vertex_normals(v.float(), f.numpy())
    with pytest.raises(ValueError, match='RGB'):
        mesh._shading((0, -1, 0), (0.5, (0.3, 0.3), 0.2), (1, 1, 0), 0.0, (1, 1, 1))
    sh = mesh._shading((0, -1, 0), (0.5, 0.3, (0.2, 0.1, 0.0)), (1, 1, 0), 2.0, (1, 1, 1))
    assert list(sh.light_specular) == pytest.approx([0.2, 0.1, 0.0]) and list(sh.light_ambient) == [0.5] * 3
    assert sh.shininess == 2.0 and list(sh.light_location) == [0.0, -1.0, 0.0]
    assert math.isclose(sh.material_diffuse[1], 1.0)
