"""The HIP face render (exavatar_release_amd.mesh) against the float64 oracle tests/mesh_oracle.py, run on the GPU.

Pixels whose centre lies within 1e-5 (barycentric units) of a covering face's edge, or where two covering faces' z
agree within 1e-6 (relative), are ambiguous IN THE ORACLE: fp32 may legitimately pick the other face there.  They are
counted (at most 0.1 % of the pixels), excluded from the value checks, and their upstream gradient is zeroed so that
both sides differentiate the same pixel set."""

import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import mesh
from tests import mesh_oracle as mo

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
AMB_MAX_FRACTION = 1e-3
VAL_TOL = 1e-5
GRAD_REL = 1e-3


def _cam(sc):
    return {'focal': sc['focal'].to(DEV), 'princpt': sc['princpt'].to(DEV)}


def _ident(N):
    return {'R': torch.eye(3, device=DEV)[None].repeat(N, 1, 1), 't': torch.zeros(N, 3, device=DEV)}


def _face_uvs(sc):
    return mo.face_uvs_of(sc['vertex_uv'], sc['face_uv'])


def _check_raster(sc, H, W):
    """pix_to_face / bary / zbuf of get_face_index_map_xy against the oracle; returns (fragments, oracle, clean mask)."""
    verts = sc['verts'].to(DEV)
    fr = exa.get_face_index_map_xy(verts, sc['faces'].numpy(), _cam(sc), (H, W))
    N = verts.shape[0]
    assert fr.pix_to_face.shape == (N, H, W, 1) and fr.pix_to_face.dtype == torch.int64
    assert fr.zbuf.shape == (N, H, W, 1) and fr.bary_coords.shape == (N, H, W, 1, 3) and fr.dists is None
    ref = mo.rasterize(verts.double(), sc['faces'].to(DEV), sc['focal'].to(DEV), sc['princpt'].to(DEV), H, W)
    amb = ref['edge_amb'] | ref['z_amb']
    p2f = fr.pix_to_face[..., 0]
    bad = (p2f != ref['pix_to_face']) & ~amb
    assert int(bad.sum()) == 0, '%d pixels pick another face away from any ambiguity' % int(bad.sum())
    assert float(amb.double().mean()) <= AMB_MAX_FRACTION, 'ambiguous fraction %g' % float(amb.double().mean())
    clean = ~amb & (p2f == ref['pix_to_face'])
    db = (fr.bary_coords[:, :, :, 0].double() - ref['bary']).abs().amax(-1)
    dz = (fr.zbuf[..., 0].double() - ref['zbuf']).abs()
    assert float(db[clean].max()) <= VAL_TOL, 'bary off by %g' % float(db[clean].max())
    assert float(dz[clean].max()) <= VAL_TOL, 'zbuf off by %g' % float(dz[clean].max())
    bg = p2f < 0
    assert bool((fr.zbuf[..., 0][bg] == -1).all()) and bool((fr.bary_coords[bg] == -1).all())
    return fr, ref, clean


def _check_render(sc, H, W, ref, clean):
    verts = sc['verts'].to(DEV)
    N = verts.shape[0]
    mr = exa.MeshRenderer(sc['vertex_uv'].numpy(), sc['face_uv'].numpy())
    out = mr(sc['texture'].to(DEV), verts, sc['faces'].numpy(), dict(_cam(sc), **_ident(N)), (H, W))
    assert out.shape == (N, sc['texture'].shape[1], H, W)
    want, _ = mo.render(verts.double(), sc['faces'].to(DEV), sc['focal'].to(DEV), sc['princpt'].to(DEV), H, W,
                        sc['texture'].to(DEV), _face_uvs(sc).to(DEV), frags=ref)
    d = (out.double() - want).abs().amax(1)
    assert float(d[clean].max()) <= VAL_TOL, 'render off by %g' % float(d[clean].max())
    bg = ref['pix_to_face'] < 0
    assert bool((out.permute(0, 2, 3, 1)[bg & clean] == -1).all())
    # the reference's face mask (model.py:200): identical wherever the oracle's mask value is not within 1e-6 of 1
    m_ref = want[:, 3]
    decided = clean & ((m_ref - 1).abs() > 1e-6)
    assert bool(((out[:, 3] == 1) == (m_ref == 1))[decided].all())
    assert int(((out[:, 3] == 1) & clean).sum()) > 100
    return out, want


@pytest.mark.parametrize('H,W', [(1024, 1024), (540, 960)])
def test_flame_sized_mesh_matches_the_oracle(H, W):
    sc = mo.flame_sized_scene(H, W, seed=0)
    assert sc['verts'].shape[1] == 5124 and sc['faces'].shape[0] == 10240
    fr, ref, clean = _check_raster(sc, H, W)
    assert int((fr.pix_to_face >= 0).sum()) > 0.2 * H * W
    _check_render(sc, H, W, ref, clean)


def _edge_scene():
    """Small scenes in one mesh pair (N = 2 packed): a screen-filling triangle far behind, degenerate faces (a repeated
    vertex, collinear corners), faces behind / across the camera plane, and a level-2 icosphere hanging off the
    top-left corner of the image."""
    H, W = 96, 128
    f, c = 150.0, (W / 2 + 0.3, H / 2 - 0.2)
    v, fc = mo.icosphere(2)
    sph = v * 0.5 + torch.tensor([-0.9, -0.6, 2.5], dtype=torch.float64)
    extra = torch.tensor([[-40.0, -40.0, 9.0], [60.0, -40.0, 9.0], [-40.0, 60.0, 9.0],     # screen-filling, z = 9
                          [0.1, 0.1, 2.0], [0.4, 0.1, 2.0], [0.7, 0.1, 2.0],                # collinear
                          [0.2, 0.2, -1.0], [0.5, 0.2, -1.0], [0.2, 0.5, 1.5]],              # one corner behind
                         dtype=torch.float64)
    V0 = sph.shape[0]
    faces = torch.cat([fc, torch.tensor([[V0, V0 + 1, V0 + 2], [V0 + 3, V0 + 4, V0 + 5], [V0 + 3, V0 + 3, V0 + 4],
                                         [V0 + 6, V0 + 7, V0 + 8]])])
    v1 = torch.cat([sph, extra])
    v2 = v1.clone()
    v2[:V0] += torch.tensor([1.1, 0.9, 0.4], dtype=torch.float64)     # second mesh: the sphere off the bottom-right
    g = torch.Generator().manual_seed(5)
    tt = torch.linspace(0, 1, 16, dtype=torch.float64)
    tv, tu = torch.meshgrid(tt, tt, indexing='ij')
    tex = torch.stack([0.3 + 0.5 * tu, 0.2 + 0.6 * tv, 0.5 + 0.2 * tu * tv, (1.6 - 2 * (tu - tv).abs()).clamp(0, 1)])[None]
    uv = torch.rand(v1.shape[0], 2, generator=g, dtype=torch.float64)
    return {'verts': torch.stack([v1, v2]).float(), 'faces': faces,
            'focal': torch.tensor([[f, f * 1.1]] * 2), 'princpt': torch.tensor([c] * 2),
            'texture': tex.float(), 'vertex_uv': uv.float(), 'face_uv': faces.clone()}, H, W


def test_edge_case_scenes_match_the_oracle():
    sc, H, W = _edge_scene()
    fr, ref, clean = _check_raster(sc, H, W)
    p2f = fr.pix_to_face[..., 0]
    F = sc['faces'].shape[0]
    sph_faces = F - 4
    # the screen-filling triangle shows wherever the sphere does not, in both meshes; nothing else but those two
    for n in range(2):
        fn = p2f[n][p2f[n] >= 0] - n * F
        assert bool(((fn < sph_faces) | (fn == sph_faces)).all())
        assert int((p2f[n] < 0).sum()) == 0 and int((fn < sph_faces).sum()) > 200
    _check_render(sc, H, W, ref, clean)


def _grad_check(got, want):
    got, want = got.double(), want.double()
    rel = float((got - want).norm() / want.norm())
    rn = want.abs().amax(-1)
    ex = ((got - want).abs().amax(-1) - GRAD_REL * rn) / rn.mean()
    assert rel <= GRAD_REL, 'global relative error %g' % rel
    assert float(ex.max()) <= GRAD_REL, 'per-vertex excess %g' % float(ex.max())


def _grads_through_render(sc, H, W, seed):
    verts = sc['verts'].to(DEV)
    N = verts.shape[0]
    _, ref, clean = _check_raster(sc, H, W)
    g = torch.Generator(device=DEV).manual_seed(seed)
    G = torch.randn((N, sc['texture'].shape[1], H, W), generator=g, device=DEV, dtype=torch.float64) * clean[:, None]
    mr = exa.MeshRenderer(sc['vertex_uv'].numpy(), sc['face_uv'].numpy())
    cam = dict(_cam(sc), **_ident(N))
    outs = []
    for _ in range(2):
        v = verts.clone().requires_grad_(True)
        out = mr(sc['texture'].to(DEV), v, sc['faces'].numpy(), cam, (H, W))
        (out * G.float()).sum().backward()
        outs.append(v.grad)
    vr = verts.double().requires_grad_(True)
    want, _ = mo.render(vr, sc['faces'].to(DEV), sc['focal'].to(DEV), sc['princpt'].to(DEV), H, W,
                        sc['texture'].to(DEV), _face_uvs(sc).to(DEV))
    (want * G).sum().backward()
    return outs, vr.grad


def test_render_gradients_match_the_oracle_and_are_deterministic():
    sc = mo.flame_sized_scene(512, 512, seed=2)
    (g1, g2), want = _grads_through_render(sc, 512, 512, seed=3)
    assert torch.equal(g1, g2), 'two backward calls differ'
    assert float(want.abs().max()) > 0
    _grad_check(g1, want)


def test_edge_scene_render_gradients_match_the_oracle():
    sc, H, W = _edge_scene()
    (g1, g2), want = _grads_through_render(sc, H, W, seed=4)
    assert torch.equal(g1, g2)
    _grad_check(g1, want)


@pytest.mark.parametrize('H,W', [(512, 512), (270, 480)])
def test_bary_and_zbuf_gradients_match_the_oracle(H, W):
    sc = mo.flame_sized_scene(H, W, seed=1, N=2)
    verts = sc['verts'].to(DEV)
    _, ref, clean = _check_raster(sc, H, W)
    g = torch.Generator(device=DEV).manual_seed(7)
    Gb = torch.randn((2, H, W, 1, 3), generator=g, device=DEV, dtype=torch.float64) * clean[..., None, None]
    Gz = torch.randn((2, H, W, 1), generator=g, device=DEV, dtype=torch.float64) * clean[..., None]
    grads = []
    for _ in range(2):
        v = verts.clone().requires_grad_(True)
        fr = exa.get_face_index_map_xy(v, sc['faces'].numpy(), _cam(sc), (H, W))
        ((fr.bary_coords * Gb.float()).sum() + (fr.zbuf * Gz.float()).sum()).backward()
        grads.append(v.grad)
    assert torch.equal(grads[0], grads[1])
    vr = verts.double().requires_grad_(True)
    r = mo.rasterize(vr, sc['faces'].to(DEV), sc['focal'].to(DEV), sc['princpt'].to(DEV), H, W)
    ((r['bary'][..., None, :] * Gb).sum() + (r['zbuf'][..., None] * Gz).sum()).backward()
    _grad_check(grads[0], vr.grad)


def test_reference_rgb_face_loss_backpropagates_into_mean_3d_like_the_oracle():
    """model.py:169-173, 200-201 written out: the face render of human_asset['mean_3d'][face_vertex_idx] composited over
    the Gaussian render by the `== 1` mask, L1 against the image; gradient into mean_3d."""
    H, W = 384, 512
    sc = mo.flame_sized_scene(H, W, seed=4)
    V = sc['verts'].shape[1]
    g = torch.Generator().manual_seed(9)
    # world = R^T (cam - t) with a real rotation; mean_3d holds more points than the face uses
    a = torch.randn(3, generator=g, dtype=torch.float64) * 0.3
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    R = torch.matrix_exp(K)
    t = torch.tensor([0.1, -0.05, 0.3], dtype=torch.float64)
    world = (sc['verts'][0].double() - t) @ R                       # rows: R^T (x - t)
    P = V + 700
    face_vertex_idx = torch.randperm(P, generator=g)[:V]
    mean_3d = torch.randn(P, 3, generator=g, dtype=torch.float64)
    mean_3d[face_vertex_idx] = world
    scene_img = torch.rand(1, 3, H, W, generator=g, dtype=torch.float64).to(DEV)
    target = torch.rand(1, 3, H, W, generator=g, dtype=torch.float64).to(DEV)
    cam = {'R': R[None].float().to(DEV), 't': t[None].float().to(DEV), 'focal': sc['focal'].to(DEV),
           'princpt': sc['princpt'].to(DEV)}
    mr = exa.MeshRenderer(sc['vertex_uv'].numpy(), sc['face_uv'].numpy())
    m_hip = mean_3d.float().to(DEV).requires_grad_(True)
    face_render = mr(sc['texture'].to(DEV), m_hip[None, face_vertex_idx.to(DEV), :], sc['faces'].numpy(), cam, (H, W))
    is_face = ((face_render[:, :3] != -1) * (face_render[:, 3:] == 1)).float()
    # the oracle side: same wiring in float64, the same discrete mask (a float of booleans has no gradient)
    m_ref = mean_3d.to(DEV).requires_grad_(True)
    cam_mesh = torch.bmm(R[None].to(DEV), m_ref[None, face_vertex_idx.to(DEV), :].permute(0, 2, 1)).permute(0, 2, 1) + \
        t.to(DEV).view(-1, 1, 3)
    want, ref = mo.render(cam_mesh, sc['faces'].to(DEV), sc['focal'].to(DEV), sc['princpt'].to(DEV), H, W,
                          sc['texture'].to(DEV), _face_uvs(sc).to(DEV))
    amb = ref['edge_amb'] | ref['z_amb'] | ((face_render.detach()[:, 0] == -1) != (want.detach()[:, 0] == -1))
    keep = (~amb).double()[:, None]
    m = is_face.double() * keep
    loss_hip = ((scene_img * (1 - m) + face_render[:, :3].double() * m - target).abs()).mean()
    loss_ref = ((scene_img * (1 - m) + want[:, :3] * m - target).abs()).mean()
    loss_hip.backward()
    loss_ref.backward()
    assert float(m.sum()) > 1000
    assert abs(float(loss_hip) - float(loss_ref)) < 1e-6
    got, wantg = m_hip.grad.double(), m_ref.grad
    assert float(got[~torch.isin(torch.arange(P, device=DEV), face_vertex_idx.to(DEV))].abs().max()) == 0
    _grad_check(got[face_vertex_idx.to(DEV)], wantg[face_vertex_idx.to(DEV)])


def test_texture_gradient_is_refused():
    sc = mo.flame_sized_scene(64, 64)
    mr = mesh.MeshRenderer(sc['vertex_uv'].numpy(), sc['face_uv'].numpy())
    tex = sc['texture'].to(DEV).requires_grad_(True)
    with pytest.raises(NotImplementedError):
        mr(tex, sc['verts'].to(DEV), sc['faces'].numpy(), dict(_cam(sc), **_ident(1)), (64, 64))
