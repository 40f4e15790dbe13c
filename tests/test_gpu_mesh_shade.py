"""The HIP Phong-shaded mesh render (exavatar_release_amd.shade_mesh / render_mesh / vertex_normals) against the float64
oracle tests/shade_oracle.py, run on the GPU.

Three views of every scene: the decisions (pix_to_face equals get_face_index_map_xy's bit for bit), the shading at the
kernel's own decisions (the oracle evaluated at the GPU's pix_to_face and barycentrics), and the render end to end
against the oracle's own rasterization with test_gpu_mesh.py's ambiguity masks.  Where the specular term is on with
shininess > 0, a pixel with |cos| < 1e-5 is ambiguous too: [cos > 0] switches the term on or off there."""
import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from tests import mesh_oracle as mo
from tests import shade_oracle as so

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
AMB_MAX_FRACTION = 1e-3
VAL_TOL = 1e-5
COS_EPS = 1e-5


def _cam(sc):
    return {'focal': sc['focal'].to(DEV), 'princpt': sc['princpt'].to(DEV)}


def _terminator(cos, shading):
    spec_on = shading.get('shininess', 0.0) > 0 and np.any(np.asarray(shading.get('materials', (0, 0, 0))[2]) != 0) and \
        np.any(np.asarray(shading.get('lights', so.REFERENCE['lights'])[2]) != 0)
    return (cos.abs() < COS_EPS) if spec_on else torch.zeros_like(cos, dtype=torch.bool)


def _check(sc, H, W, **shading):
    """All three views of one scene; returns (image, pix_to_face, clean mask, oracle image, oracle fragments)."""
    verts = sc['verts'].to(DEV)
    faces = sc['faces']
    N, F = verts.shape[0], faces.shape[0]
    image, p2f = exa.shade_mesh(verts, faces.numpy(), _cam(sc), (H, W), **shading)
    assert image.shape == (N, H, W, 3) and image.dtype == torch.float32 and p2f.shape == (N, H, W)
    # decisions: the raster of the face render, bit for bit
    fr = exa.get_face_index_map_xy(verts, faces.numpy(), _cam(sc), (H, W))
    assert torch.equal(p2f, fr.pix_to_face[..., 0])
    cov = p2f >= 0
    assert int(cov.sum()) > 0
    bg = torch.tensor(shading.get('background', so.REFERENCE['background']), dtype=torch.float32, device=DEV)
    assert bool((image[~cov] == bg).all()), 'background pixels must hold the background colour exactly'
    # shading at the kernel's own decisions
    normals, raw = so.vertex_normals(verts, faces)
    nrm = torch.from_numpy(normals).to(DEV)
    face = torch.where(cov, p2f - torch.arange(N, device=DEV)[:, None, None] * F, p2f)
    want, cos = so.shade(verts, faces.to(DEV), nrm, face, fr.bary_coords[:, :, :, 0], **shading)
    term = _terminator(cos, shading) & cov
    assert int(term.sum()) <= 1e-4 * N * H * W
    d = (image.double() - want).abs().amax(-1)
    assert float(d[cov & ~term].max()) <= VAL_TOL, 'image at the kernel decisions off by %g' % float(d[cov & ~term].max())
    # end to end against the oracle's own rasterization
    ref_img, ref_cos, ref = so.render(verts.double(), faces.to(DEV), sc['focal'].to(DEV), sc['princpt'].to(DEV), H, W,
                                      **shading)
    amb = ref['edge_amb'] | ref['z_amb'] | (_terminator(ref_cos, shading) & (ref['face'] >= 0))
    assert float(amb.double().mean()) <= AMB_MAX_FRACTION, 'ambiguous fraction %g' % float(amb.double().mean())
    bad = (p2f != ref['pix_to_face']) & ~amb
    assert int(bad.sum()) == 0, '%d pixels pick another face away from any ambiguity' % int(bad.sum())
    clean = ~amb & (p2f == ref['pix_to_face'])
    d = (image.double() - ref_img).abs().amax(-1)
    assert float(d[clean].max()) <= VAL_TOL, 'image end to end off by %g' % float(d[clean].max())
    return image, p2f, clean, ref_img, ref


@pytest.mark.parametrize('scene', ['flame', 'smplx'])
def test_vertex_normals_match_the_oracle_and_are_deterministic(scene):
    sc = mo.flame_sized_scene(256, 256) if scene == 'flame' else so.smplx_sized_scene(1080, 1920)
    verts = sc['verts'].to(DEV)
    n1 = exa.vertex_normals(verts, sc['faces'].numpy())
    n2 = exa.vertex_normals(verts, sc['faces'].numpy())
    assert n1.shape == verts.shape and torch.equal(n1, n2)
    want, raw = so.vertex_normals(verts, sc['faces'])
    keep = torch.from_numpy(np.linalg.norm(raw, axis=-1) >= 1e-9).to(DEV)
    assert int((~keep).sum()) <= 0.001 * keep.numel()
    d = (n1.double() - torch.from_numpy(want).to(DEV)).abs().amax(-1)
    assert float(d[keep].max()) <= VAL_TOL, 'normals off by %g (%d excluded)' % (float(d[keep].max()), int((~keep).sum()))
    # a [V, 3] mesh is one mesh
    assert torch.equal(exa.vertex_normals(verts[0], sc['faces'].numpy()), n1)


def test_smplx_sized_1080p_matches_the_oracle():
    sc = so.smplx_sized_scene(1080, 1920)
    image, p2f, clean, _, _ = _check(sc, 1080, 1920)
    assert int((p2f >= 0).sum()) > 0.04 * 1080 * 1920
    # the reference's configuration: grey in [0.5, 0.8]
    cov = p2f >= 0
    assert bool((image[cov] >= 0.5).all()) and bool((image[cov] <= 0.8 + 1e-6).all())
    assert bool((image[..., 0] == image[..., 1]).all() and (image[..., 1] == image[..., 2]).all())
    assert int((image[cov][:, 0] > 0.7).sum()) > 1000 and int((image[cov][:, 0] == 0.5).sum()) > 100


def test_non_square_image_with_an_off_centre_principal_point():
    H, W = 300, 520
    sc = mo.flame_sized_scene(H, W, seed=3)
    sc['princpt'] = sc['princpt'] + torch.tensor([[61.3, -37.7]])
    _check(sc, H, W)


def _mixed_scene():
    """One mesh of three parts: a sphere wound outward, a sphere wound inward (lit from inside: the winding decides),
    and a triangle whose corners straddle z = 0 (culled: background where it would project)."""
    v, f = mo.icosphere(3)
    a = v * 0.5 + torch.tensor([-0.55, 0.0, 3.0], dtype=torch.float64)
    b = v * 0.5 + torch.tensor([0.55, 0.1, 3.2], dtype=torch.float64)
    V0 = v.shape[0]
    cross = torch.tensor([[-0.3, -0.3, -0.5], [0.3, -0.2, 1.0], [0.0, 0.4, 1.0]], dtype=torch.float64)
    verts = torch.cat([a, b, cross])[None]
    faces = torch.cat([f, f[:, [0, 2, 1]] + V0, torch.tensor([[2 * V0, 2 * V0 + 1, 2 * V0 + 2]])])
    H, W = 200, 320
    return {'verts': verts.float(), 'faces': faces, 'focal': torch.tensor([[260.0, 250.0]]),
            'princpt': torch.tensor([[W / 2 + 0.3, H / 2 - 0.4]])}, H, W


def test_both_windings_and_a_face_across_the_camera_plane():
    sc, H, W = _mixed_scene()
    image, p2f, clean, _, _ = _check(sc, H, W)
    F = sc['faces'].shape[0]
    assert not bool((p2f == F - 1).any()), 'the face across z = 0 must be culled'
    assert bool((image[0, H // 2 - 3:H // 2 + 3, W // 2 - 3:W // 2 + 3] == 1).all())      # the gap between the spheres
    # the light (y = -1) sits above the camera: the outward sphere shows mostly lit faces, the inward one mostly faces
    # turned away from the light (ambient only, exactly 0.5)
    Fs = (F - 1) // 2
    left = (p2f[0] >= 0) & (p2f[0] < Fs)
    right = (p2f[0] >= Fs) & (p2f[0] < 2 * Fs)
    assert int(left.sum()) > 1000 and int(right.sum()) > 1000
    assert float((image[0][left][:, 0] == 0.5).double().mean()) < 0.2
    assert float((image[0][right][:, 0] == 0.5).double().mean()) > 0.8


@pytest.mark.parametrize('shininess', [0.0, 8.0])
def test_non_default_lights_and_materials(shininess):
    sc = mo.flame_sized_scene(384, 512, seed=5)
    shading = dict(light_location=(1.5, -2.0, 0.5), lights=((0.2, 0.25, 0.3), 0.6, (0.5, 0.4, 0.3)),
                   materials=(0.9, (1.0, 0.8, 0.6), (0.7, 0.8, 0.9)), shininess=shininess, background=(0.1, 0.2, 0.3))
    image, p2f, _, _, _ = _check(sc, 384, 512, **shading)
    assert not torch.equal(image[..., 0], image[..., 2])


def test_four_meshes_in_one_launch_equal_four_single_calls():
    sc = so.smplx_sized_scene(270, 480, seed=1, N=4)
    verts = sc['verts'].to(DEV)
    shading = dict(materials=(1.0, 1.0, 0.5), shininess=8.0)
    image, p2f = exa.shade_mesh(verts, sc['faces'].numpy(), _cam(sc), (270, 480), **shading)
    F = sc['faces'].shape[0]
    for n in range(4):
        cam = {'focal': sc['focal'][n].to(DEV), 'princpt': sc['princpt'][n].to(DEV)}
        i1, p1 = exa.shade_mesh(verts[n], sc['faces'].numpy(), cam, (270, 480), **shading)
        assert torch.equal(i1[0], image[n])
        assert torch.equal(torch.where(p1[0] >= 0, p1[0] + n * F, p1[0]), p2f[n])
    _check(sc, 270, 480, **shading)


def _reference_render(sc, H, W, bkg, blend_ratio):
    """The oracle through the reference's composite, plus its ambiguity mask [H, W]."""
    ref_img, ref_cos, ref = so.render(sc['verts'].to(DEV).double(), sc['faces'].to(DEV), sc['focal'].to(DEV),
                                      sc['princpt'].to(DEV), H, W)
    # pytorch3d's images and zbuf are float32: so is what the reference composites
    want = so.reference_composite(ref_img.float().cpu(), ref['zbuf'][..., None].float().cpu(), bkg, blend_ratio)
    amb = (ref['edge_amb'] | ref['z_amb'])[0].cpu().numpy()
    return want, amb


def _compare_composites(got, want, amb):
    assert got.shape == want.shape and got.dtype == want.dtype
    assert amb.mean() <= AMB_MAX_FRACTION
    d = np.abs(got.astype(np.float64) - want.astype(np.float64)).max(-1)
    assert d[~amb].max() <= 1e-3, 'composite off by %g' % d[~amb].max()
    du = np.abs(got.astype(np.uint8).astype(np.int32) - want.astype(np.uint8).astype(np.int32)).max(-1)
    assert (du > 0).mean() <= 1e-3 and du[~amb].max() <= 1


def test_render_mesh_avatar_form():
    """animate.py:83: torch mesh [V,3], cam_param tensors with extra R / t keys, a float32 background of 255s."""
    H, W = 540, 960
    sc = so.smplx_sized_scene(H, W, seed=2)
    cam = {'focal': sc['focal'][0].to(DEV), 'princpt': sc['princpt'][0].to(DEV), 'R': torch.eye(3, device=DEV),
           't': torch.zeros(3, device=DEV)}
    bkg = np.ones((H, W, 3), dtype=np.float32) * 255
    got = exa.render_mesh(sc['verts'][0].to(DEV), sc['faces'].numpy(), cam, bkg)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    want, amb = _reference_render(sc, H, W, bkg, 1.0)
    _compare_composites(got, want, amb)
    assert (got.astype(np.uint8) == 255).all(-1).mean() > 0.5 and (got.astype(np.uint8) == 127).any()


@pytest.mark.parametrize('blend_ratio', [1.0, 0.6])
def test_render_mesh_fitting_form(blend_ratio):
    """fit.py:162: numpy mesh and cam_param, and a [..., ::-1] view of a float32 image as bkg."""
    H, W = 400, 300
    sc = so.smplx_sized_scene(H, W, seed=3)
    img = np.random.default_rng(0).uniform(0, 255, (H, W, 3)).astype(np.float32)
    bkg = img[:, :, ::-1]
    cam = {'focal': sc['focal'][0].numpy(), 'princpt': sc['princpt'][0].numpy()}
    got = exa.render_mesh(sc['verts'][0].numpy(), sc['faces'].numpy(), cam, bkg, blend_ratio)
    want, amb = _reference_render(sc, H, W, bkg, blend_ratio)
    _compare_composites(got, want, amb)


def test_grad_mode_is_refused():
    sc = so.smplx_sized_scene(64, 64)
    v = sc['verts'].to(DEV).requires_grad_(True)
    with pytest.raises(NotImplementedError):
        exa.shade_mesh(v, sc['faces'].numpy(), _cam(sc), (64, 64))
    with pytest.raises(NotImplementedError):
        exa.vertex_normals(v, sc['faces'].numpy())
    with torch.no_grad():
        image, _ = exa.shade_mesh(v, sc['faces'].numpy(), _cam(sc), (64, 64))
    assert not image.requires_grad
    # render_mesh renders under no_grad, as the reference does
    exa.render_mesh(v[0], sc['faces'].numpy(), {k: x[0] for k, x in _cam(sc).items()}, np.zeros((64, 64, 3), np.float32))
