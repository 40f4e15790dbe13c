"""The HIP mesh rasterizer (exavatar_release_amd.mesh, csrc/mesh_raster.hip) at the shapes and edges its kernels branch on.

tests/test_gpu_mesh.py and tests/test_gpu_mesh_shade.py see smooth icospheres of 10 240 faces at large images.  Here the
scenes come from the builders at the end of tests/mesh_oracle.py (checked without a GPU by tests/test_mesh_oracle.py):

A. exact scenes: every decision is the same in float32 and float64 (pixel centres ON edges and vertices, exact z ties,
   an area just above and just below MIN_AREA, faces culled outright), so ``pix_to_face`` must equal the oracle's at EVERY
   pixel -- no ambiguity mask;
B. shapes: F = 0 .. 8193 (the tail word of the face bitmask, the second trip over the mask words), images smaller than
   a tile and ragged in both axes, a batch with a camera and a texture per mesh, off-screen and far faces, depth orders.
   The oracle's ambiguous pixels are capped as in test_gpu_mesh.py, and the builders pick seeds that have none wherever
   the image has fewer than 1000 pixels;
C. the sampler: 1, 3 and 8 channels, maps down to 1 x 1, uv beyond, on and inside [0, 1]; the ``== 1`` mask against
   ``F.grid_sample`` in float32 at every covered pixel; exactly zero gradient under the border clamp;
D. the backward: every cotangent alone, a vertex of 2048 faces, unreferenced vertices, two calls bit for bit;
E. the shaded path and the host's topology cache.

The bar of a gradient is not a number chosen here.  ``mesh_oracle.revalue`` evaluates and differentiates the oracle's
values in float32 at the float64 run's winners; that run's error against the float64 run (relative L2, and the max norm
scaled by norm / sqrt(n), each floored at 2^-24) is what one float32 evaluation of these expressions costs, and the HIP
result -- another float32 evaluation in another order -- must stay within FACTOR = 4 of it (DESIGN.md sections 8j, 8b)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exavatar_release_amd as exa
from exavatar_release_amd import mesh
from tests import helpers
from tests import mesh_oracle as mo
from tests import shade_oracle as so
from tests.test_gpu_mesh import VAL_TOL

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
FACTOR = 4.0
FLOOR = 2.0 ** -24


# ---- plumbing ----------------------------------------------------------------------------------------------------------
def _cam(sc, n=None):
    pick = (lambda t: t) if n is None else (lambda t: t[n:n + 1])
    return {'focal': pick(sc['focal']).to(DEV), 'princpt': pick(sc['princpt']).to(DEV)}


def _full_cam(sc, n=None):
    N = sc['verts'].shape[0] if n is None else 1
    return dict(_cam(sc, n), R=torch.eye(3, device=DEV)[None].repeat(N, 1, 1), t=torch.zeros(N, 3, device=DEV))


def _renderer(sc):
    return exa.MeshRenderer(sc['vertex_uv'].numpy(), sc['face_uv'].numpy())


_oracles = {}


def _oracle(sc):
    """The float64 oracle of a (cached, read-only) scene, on the device, computed once."""
    if id(sc) not in _oracles:
        _oracles[id(sc)] = (sc, mo.rasterize(sc['verts'].to(DEV), sc['faces'].to(DEV), sc['focal'].to(DEV), sc['princpt'].to(DEV),
                                             sc['H'], sc['W']))
    return _oracles[id(sc)][1]


def _check_raster(sc, exact=False):
    """pix_to_face / bary / zbuf of get_face_index_map_xy against the oracle, two calls bit for bit.  ``exact``: equal at
    every pixel, the oracle's ambiguity masks ignored.  Returns (fragments, oracle, clean mask)."""
    verts = sc['verts'].to(DEV)
    N, H, W = verts.shape[0], sc['H'], sc['W']
    fr = exa.get_face_index_map_xy(verts, sc['faces'].numpy(), _cam(sc), (H, W))
    again = exa.get_face_index_map_xy(verts, sc['faces'].numpy(), _cam(sc), (H, W))
    assert fr.pix_to_face.shape == (N, H, W, 1) and fr.zbuf.shape == (N, H, W, 1) and fr.bary_coords.shape == (N, H, W, 1, 3)
    for a, b in zip(fr[:3], again[:3]):
        assert torch.equal(a, b), 'two forward calls differ'
    ref = _oracle(sc)
    p2f = fr.pix_to_face[..., 0]
    if exact:
        amb = torch.zeros_like(p2f, dtype=torch.bool)
    else:
        amb = ref['edge_amb'] | ref['z_amb']
        assert int(amb.sum()) <= N * mo.amb_cap(H, W), '%d ambiguous pixels' % int(amb.sum())
    bad = (p2f != ref['pix_to_face']) & ~amb
    assert int(bad.sum()) == 0, '%d pixels pick another face than the oracle: %s' % (
        int(bad.sum()), [(i, p2f[tuple(i)].item(), ref['pix_to_face'][tuple(i)].item()) for i in torch.nonzero(bad)[:8].tolist()])
    clean = ~amb & (p2f == ref['pix_to_face'])
    cov = clean & (p2f >= 0)
    assert bool(torch.isfinite(fr.zbuf).all()) and bool(torch.isfinite(fr.bary_coords).all())
    if bool(cov.any()):
        db = (fr.bary_coords[:, :, :, 0].double() - ref['bary']).abs().amax(-1)[cov].max()
        dz = (fr.zbuf[..., 0].double() - ref['zbuf']).abs()[cov].max()
        assert float(db) <= VAL_TOL and float(dz) <= VAL_TOL, 'bary off by %g, zbuf by %g' % (float(db), float(dz))
    bg = p2f < 0
    assert bool((fr.zbuf[..., 0][bg] == -1).all()) and bool((fr.bary_coords[bg] == -1).all())
    return fr, ref, clean


def _check_render(sc, ref, clean):
    """MeshRenderer against the oracle's render at the oracle's winners; two calls bit for bit.  Returns the render."""
    verts = sc['verts'].to(DEV)
    H, W = sc['H'], sc['W']
    mr = _renderer(sc)
    out = mr(sc['texture'].to(DEV), verts, sc['faces'].numpy(), _full_cam(sc), (H, W))
    assert torch.equal(out, mr(sc['texture'].to(DEV), verts, sc['faces'].numpy(), _full_cam(sc), (H, W)))
    assert out.shape == (verts.shape[0], sc['texture'].shape[1], H, W) and bool(torch.isfinite(out).all())
    want, _ = mo.render(verts.double(), sc['faces'].to(DEV), sc['focal'].to(DEV), sc['princpt'].to(DEV), H, W,
                        sc['texture'].to(DEV), mo.face_uvs_of(sc['vertex_uv'], sc['face_uv']).to(DEV), frags=ref)
    d = (out.double() - want).abs().amax(1)
    if bool(clean.any()):
        assert float(d[clean].max()) <= VAL_TOL, 'render off by %g' % float(d[clean].max())
    bg = ref['pix_to_face'] < 0
    assert bool((out.permute(0, 2, 3, 1)[bg & clean] == -1).all())
    return out


def _ratio(got, g32, g64):
    """(HIP error) / (the float32 oracle's own error), the larger of the L2 and the scaled max figure; the yardstick too."""
    got, g32, g64 = got.double(), g32.double(), g64.double()
    norm, n = float(g64.norm()), g64.numel()
    if norm == 0.0:
        return (0.0 if not bool(got.any()) else math.inf), 0.0, 0.0
    y_l2 = max(float((g32 - g64).norm()) / norm, FLOOR)
    y_mx = max(float((g32 - g64).abs().max()) / (norm / math.sqrt(n)), FLOOR)
    r = max(float((got - g64).norm()) / (y_l2 * norm), float((got - g64).abs().max()) / (y_mx * norm / math.sqrt(n)))
    return r, y_l2, y_mx


WHICH = ('dzbuf', 'dbary', 'drender', 'all')


def _gradients(sc, which, seed=0, verts=None, faces=None, exact=False):
    """dL/dverts of the HIP path (twice), of the float64 oracle and of its float32 revaluation, for random cotangents of
    zbuf / bary / render (``which``), zeroed where the HIP winners are not the oracle's (ambiguous pixels only: checked)
    and at the oracle's ambiguous pixels -- unless the scene is ``exact``, where nothing is ambiguous."""
    verts = sc['verts'].to(DEV) if verts is None else verts
    faces = sc['faces'] if faces is None else faces
    N, H, W = verts.shape[0], sc['H'], sc['W']
    textured = which in ('drender', 'all') and 'texture' in sc
    cam = (sc['focal'].to(DEV), sc['princpt'].to(DEV))
    v64 = verts.double().requires_grad_(True)
    fr64 = mo.rasterize(v64, faces.to(DEV), *cam, H, W)
    g = torch.Generator(device=DEV).manual_seed(1234 + seed)
    Gz = torch.randn((N, H, W), generator=g, device=DEV, dtype=torch.float64)
    Gb = torch.randn((N, H, W, 3), generator=g, device=DEV, dtype=torch.float64)
    C = sc['texture'].shape[1] if textured else 1
    Gr = torch.randn((N, C, H, W), generator=g, device=DEV, dtype=torch.float64)
    tex = sc['texture'].to(DEV) if textured else None
    fuv = mo.face_uvs_of(sc['vertex_uv'], sc['face_uv']).to(DEV) if textured else None

    def loss(zbuf, bary, render, keep):
        dt = zbuf.dtype
        L = 0
        if which in ('dzbuf', 'all'):
            L = L + (zbuf * (Gz * keep).to(dt)).sum()
        if which in ('dbary', 'all'):
            L = L + (bary * (Gb * keep[..., None]).to(dt)).sum()
        if textured:
            L = L + (render * (Gr * keep[:, None]).to(dt)).sum()
        return L

    hip, keep = [], None
    for _ in range(2):
        v = verts.clone().requires_grad_(True)
        fr = exa.get_face_index_map_xy(v, faces.numpy(), _cam(sc), (H, W))
        out = _renderer(sc)(tex, v, faces.numpy(), _full_cam(sc), (H, W)) if textured else None
        if keep is None:
            amb = (fr64['edge_amb'] | fr64['z_amb']) & (not exact)
            p2f = fr.pix_to_face[..., 0]
            assert int(((p2f != fr64['pix_to_face']) & ~amb).sum()) == 0
            keep = ((p2f == fr64['pix_to_face']) & ~amb).double()
        loss(fr.zbuf[..., 0], fr.bary_coords[:, :, :, 0], out, keep).backward()
        hip.append(v.grad)
    assert torch.equal(hip[0], hip[1]), 'two backward calls differ'
    assert bool(torch.isfinite(hip[0]).all())
    out64 = mo.render(v64, faces.to(DEV), *cam, H, W, tex, fuv, frags=fr64)[0] if textured else None
    loss(fr64['zbuf'], fr64['bary'], out64, keep).backward()
    v32 = verts.clone().requires_grad_(True)
    fr32 = mo.revalue(fr64, v32, faces.to(DEV), *cam)
    out32 = mo.render(v32, faces.to(DEV), *cam, H, W, tex, fuv, frags=fr32)[0] if textured else None
    loss(fr32['zbuf'], fr32['bary'], out32, keep).backward()
    return hip[0], v32.grad, v64.grad


def _check_gradients(tag, sc, which, may_vanish=False, **kw):
    got, g32, g64 = _gradients(sc, which, **kw)
    assert may_vanish or float(g64.abs().max()) > 0, 'the oracle\'s gradient vanishes: nothing is tested'
    r, y_l2, y_mx = _ratio(got, g32, g64)
    print('%s/%s: ratio %.3f (yardstick rel_l2 %.3g rel_max %.3g)' % (tag, which, r, y_l2, y_mx))
    helpers.record_stats('mesh_edges/%s/%s' % (tag, which), {'ratio': r, 'rel_l2': y_l2, 'rel_max': y_mx})
    assert r <= FACTOR, '%s/%s: HIP gradient error is %.2f x the float32 oracle\'s own' % (tag, which, r)
    return got, g64


# ---- A. exact scenes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(mo.exact_scenes()))
def test_exact_scene_equals_the_oracle_at_every_pixel(name):
    sc = mo.exact_scenes()[name]
    fr, ref, _ = _check_raster(sc, exact=True)
    f = fr.pix_to_face[0, :, :, 0]
    # the hand-derived answers of tests/test_mesh_oracle.py, for the decisions no other test reaches
    if name.startswith('quad'):
        assert all(int(f[i, i]) == -1 for i in range(12)) and int(f[2, 5]) == -1 and int(f[5, 8]) == -1 and int((f >= 0).sum()) == 20
    if name == 'fan8':
        assert int(f[6, 6]) == -1 and bool((f[5:8, 5:8] >= 0).sum() == 8)
    if name == 'stack':
        assert int((f == 2).sum()) == 78 and not bool(((f == 5) | (f == 9)).any())
    if name == 'stacks2':
        assert int((f == 4).sum()) == 78 and not bool(torch.isin(f, torch.tensor([1, 3, 6, 7, 8], device=DEV)).any())
    if name == 'tiny':
        assert int(f[2, 2]) == 0 and int((f >= 0).sum()) == 1
    _check_gradients('exact_' + name, sc, 'all', exact=True)


def test_culled_faces_leave_every_output_finite_and_get_exactly_zero_gradient():
    sc = mo.culled_scene()
    fr, ref, _ = _check_raster(sc, exact=True)
    f = fr.pix_to_face[0, :, :, 0]
    assert set(f.flatten().tolist()) == {-1, 0}
    verts = sc['verts'].to(DEV)
    grads = []
    for _ in range(2):
        v = verts.clone().requires_grad_(True)
        r = exa.get_face_index_map_xy(v, sc['faces'].numpy(), _cam(sc), (sc['H'], sc['W']))
        (r.zbuf.sum() + (r.bary_coords * torch.tensor([0.3, -0.7, 1.1], device=DEV)).sum()).backward()
        grads.append(v.grad)
    assert torch.equal(grads[0], grads[1])
    assert bool((grads[0][0, 3:] == 0).all()), 'a culled face got a gradient'
    assert bool(torch.isfinite(grads[0]).all()) and float(grads[0][0, :3].abs().max()) > 0
    # the good face alone is the same render: its gradient against the oracle's (whose autograd would turn the NaN and
    # Inf coordinates of the culled corners into NaN gradients)
    got, g64 = _check_gradients('culled_good_face', sc, 'all', verts=verts[:, :3], faces=sc['faces'][:1], exact=True)
    v = verts.clone().requires_grad_(True)
    r = exa.get_face_index_map_xy(v, sc['faces'].numpy(), _cam(sc), (sc['H'], sc['W']))
    v3 = verts[:, :3].clone().requires_grad_(True)
    r3 = exa.get_face_index_map_xy(v3, sc['faces'][:1].numpy(), _cam(sc), (sc['H'], sc['W']))
    assert torch.equal(r.zbuf, r3.zbuf) and torch.equal(r.bary_coords, r3.bary_coords)


# ---- B. shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nF', mo.FACE_COUNTS)
def test_face_counts_around_the_mask_word_and_trip_boundaries(nF):
    sc = mo.face_count_scene(nF)
    fr, ref, clean = _check_raster(sc)
    assert bool(clean.all())
    f = fr.pix_to_face[0, :, :, 0]
    if nF == 0:
        assert bool((f == -1).all())
        got, g32, g64 = _gradients(sc, 'all')
        assert bool((got == 0).all()) and bool((g64 == 0).all())
        return
    assert int((f == nF - 1).sum()) > 50
    _check_gradients('faces%d' % nF, sc, 'all')


@pytest.mark.parametrize('H,W', mo.IMAGE_SIZES)
def test_image_sizes_below_and_across_the_tile_and_the_cell(H, W):
    sc = mo.shape_scene(H, W)
    fr, ref, clean = _check_raster(sc)
    assert int((fr.pix_to_face >= 0).sum()) == H * W            # the backdrop leaves no hole
    if H * W > 30:
        assert int((fr.pix_to_face[..., 0] < 80).sum()) > 0.1 * H * W and int((fr.pix_to_face[..., 0] == 80).sum()) > 0.1 * H * W
    _check_render(sc, ref, clean)
    _check_gradients('image%dx%d' % (H, W), sc, 'all')


@pytest.mark.parametrize('tex_N', [3, 1])
def test_batch_of_three_cameras_and_textures_equals_three_single_calls(tex_N):
    sc = mo.batch_scene(tex_N)
    assert sc['texture'].shape[0] == tex_N
    fr, ref, clean = _check_raster(sc)
    out = _check_render(sc, ref, clean)
    nF, H, W = sc['faces'].shape[0], sc['H'], sc['W']
    g = torch.Generator(device=DEV).manual_seed(5)
    Gr = torch.randn(out.shape, generator=g, device=DEV)
    Gz = torch.randn((3, H, W, 1), generator=g, device=DEV)
    Gb = torch.randn((3, H, W, 1, 3), generator=g, device=DEV)

    def run(verts, cam, full_cam, tex, sl):
        v = verts.clone().requires_grad_(True)
        r = exa.get_face_index_map_xy(v, sc['faces'].numpy(), cam, (H, W))
        o = _renderer(sc)(tex, v, sc['faces'].numpy(), full_cam, (H, W))
        ((o * Gr[sl]).sum() + (r.zbuf * Gz[sl]).sum() + (r.bary_coords * Gb[sl]).sum()).backward()
        return r, o, v.grad
    verts, tex = sc['verts'].to(DEV), sc['texture'].to(DEV)
    rb, ob, gb = run(verts, _cam(sc), _full_cam(sc), tex, slice(0, 3))
    assert torch.equal(rb.pix_to_face, fr.pix_to_face) and torch.equal(ob, out)
    if tex_N == 3:
        assert not torch.equal(ob[0], ob[1])
    for n in range(3):
        r1, o1, g1 = run(verts[n:n + 1], _cam(sc, n), _full_cam(sc, n), tex[n:n + 1] if tex_N == 3 else tex, slice(n, n + 1))
        p1 = r1.pix_to_face[0]
        assert torch.equal(torch.where(p1 >= 0, p1 + n * nF, p1), rb.pix_to_face[n]), 'mesh %d: pix_to_face' % n
        assert torch.equal(r1.zbuf[0], rb.zbuf[n]) and torch.equal(r1.bary_coords[0], rb.bary_coords[n]), 'mesh %d' % n
        assert torch.equal(o1[0], ob[n]), 'mesh %d: render' % n
        assert torch.equal(g1[0], gb[n]), 'mesh %d: dverts' % n


def test_off_screen_faces_own_no_pixel_and_get_exactly_zero_gradient():
    sc = mo.offscreen_scene()
    fr, ref, clean = _check_raster(sc)
    assert set(fr.pix_to_face.flatten().tolist()) == {-1, 0}
    got, _ = _check_gradients('offscreen', sc, 'all')
    assert bool((got[0, 3:] == 0).all()) and float(got[0, :3].abs().max()) > 0


@pytest.mark.parametrize('name', ['far_corner', 'strip', 'depth', 'crossing'])
def test_far_thin_stacked_and_crossing_faces(name):
    sc = {'far_corner': mo.far_corner_scene, 'strip': mo.strip_scene, 'depth': mo.depth_scene, 'crossing': mo.crossing_scene}[name]()
    fr, ref, clean = _check_raster(sc)
    f = fr.pix_to_face[0, :, :, 0]
    if name == 'far_corner':
        assert int((f == 0).sum()) > 50
    if name == 'strip':
        cols = torch.nonzero((f == 0).any(0)).flatten()
        assert int(cols.min()) >= 1048 and int(cols.max()) <= 1052 and int((f == 0).sum()) > 10 and bool((f == 1).any())
    if name == 'depth':
        assert len(set(f.flatten().tolist())) >= 25 and not bool((f < 0).any())
    if name == 'crossing':
        assert int((f == 0).sum()) > 300 and int((f == 1).sum()) > 300
    _check_gradients(name, sc, 'all')


# ---- C. sampler --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tH,tW', mo.SAMPLER_MAPS)
@pytest.mark.parametrize('C', [1, 3, 8])
def test_sampler_channels_map_sizes_and_uv_placements(C, tH, tW):
    sc = mo.sampler_scene(C, tH, tW)
    assert sc['texture'].shape == (1, C, tH, tW)
    fr, ref, clean = _check_raster(sc)
    assert bool(clean.all())
    out = _check_render(sc, ref, clean)
    # the reference's `== 1` mask against F.grid_sample in float32, fed the kernel's own barycentrics combined as the
    # kernel combines them: (p0 u0 + p1 u1) + p2 u2, one rounding per operation
    p2f = fr.pix_to_face[..., 0]
    cov = p2f >= 0
    p = fr.bary_coords[:, :, :, 0]
    uvs = mo.face_uvs_of(sc['vertex_uv'], sc['face_uv']).to(DEV)[p2f.clamp_min(0)]          # [1,H,W,3,2]
    uv = (p[..., 0, None] * uvs[..., 0, :] + p[..., 1, None] * uvs[..., 1, :]) + p[..., 2, None] * uvs[..., 2, :]
    gs = F.grid_sample(torch.flip(sc['texture'].to(DEV), [2]), uv * 2.0 - 1.0, mode='bilinear', padding_mode='border',
                       align_corners=True)
    one_hip, one_gs = (out[:, C - 1] == 1)[cov], (gs[:, C - 1] == 1)[cov]
    print('sampler C=%d %dx%d: %d of %d covered pixels are 1; max |render - grid_sample| %g' % (
        C, tH, tW, int(one_hip.sum()), int(cov.sum()), float((out - gs).abs().amax(1)[cov].max())))
    assert torch.equal(one_hip, one_gs), '%d pixels disagree on == 1' % int((one_hip != one_gs).sum())
    assert int(one_hip.sum()) > 20 and (tH * tW == 1 or int((~one_hip).sum()) > 20)
    # gradient of the render alone: exactly zero where the clamp is active, alive elsewhere
    got, _ = _check_gradients('sampler_C%d_%dx%d' % (C, tH, tW), sc, 'drender', may_vanish=tH * tW == 1)
    q0 = 4 * mo.FIRST_CLAMPED_PATTERN
    assert bool((got[0, q0:] == 0).all()), 'a clamped sample passed a gradient on'
    if tH > 1 and tW > 1:
        assert float(got[0, :4].abs().max()) > 0


# ---- D. backward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', WHICH)
@pytest.mark.parametrize('name', ['image65x63', 'image130x70', 'batch3'])
def test_every_cotangent_alone_and_all_together(name, which):
    sc = {'image65x63': lambda: mo.shape_scene(65, 63), 'image130x70': lambda: mo.shape_scene(130, 70),
          'batch3': lambda: mo.batch_scene(3)}[name]()
    got, g64 = _check_gradients(name, sc, which, seed=WHICH.index(which))
    assert float(g64.abs().max()) > 0


def test_a_vertex_of_2048_faces_and_unreferenced_vertices():
    sc = mo.fan_scene()
    fr, ref, clean = _check_raster(sc)
    assert len(set(fr.pix_to_face.flatten().tolist())) > 1000
    _check_render(sc, ref, clean)
    for which in WHICH:
        got, g64 = _check_gradients('fan2048', sc, which, seed=WHICH.index(which))
        idx = torch.tensor(mo.FAN_UNREFERENCED, device=DEV)
        assert bool((got[0, idx] == 0).all()), 'an unreferenced vertex got a gradient'
        c = mo.FAN_CENTRE
        print('fan2048/%s: centre vertex HIP %s oracle %s' % (which, got[0, c].tolist(), g64[0, c].tolist()))
        assert float(got[0, c].abs().max()) > 0


# ---- E. shaded path and host ---------------------------------------------------------------------------------------------
def _check_shade(sc):
    verts, faces = sc['verts'].to(DEV), sc['faces']
    N, nF, H, W = verts.shape[0], faces.shape[0], sc['H'], sc['W']
    image, p2f = exa.shade_mesh(verts, faces.numpy(), _cam(sc), (H, W))
    fr = exa.get_face_index_map_xy(verts, faces.numpy(), _cam(sc), (H, W))
    assert torch.equal(p2f, fr.pix_to_face[..., 0]) and image.shape == (N, H, W, 3)
    cov = p2f >= 0
    assert bool((image[~cov] == 1).all()), 'background pixels must hold the background colour exactly'
    n_hip = exa.vertex_normals(verts, faces.numpy())
    if nF == 0:
        assert not bool(cov.any()) and bool((n_hip == 0).all())
        return
    normals, raw = so.vertex_normals(verts, faces)
    norm = torch.from_numpy(np.linalg.norm(raw, axis=-1)).to(DEV)
    d = (n_hip.double() - torch.from_numpy(normals).to(DEV)).abs().amax(-1)
    assert float(d[norm >= 1e-9].max()) <= VAL_TOL, 'normals off by %g' % float(d[norm >= 1e-9].max())
    assert bool((n_hip[norm == 0] == 0).all())
    face = torch.where(cov, p2f - torch.arange(N, device=DEV)[:, None, None] * nF, p2f)
    want, _ = so.shade(verts, faces.to(DEV), torch.from_numpy(normals).to(DEV), face, fr.bary_coords[:, :, :, 0])
    d = (image.double() - want).abs().amax(-1)
    assert float(d[cov].max()) <= VAL_TOL, 'image at the kernel decisions off by %g' % float(d[cov].max())
    # end to end against the oracle's own winners
    ref = _oracle(sc)
    ref_img, _, _ = so.render(verts.double(), faces.to(DEV), sc['focal'].to(DEV), sc['princpt'].to(DEV), H, W, frags=ref)
    amb = ref['edge_amb'] | ref['z_amb']
    assert int(amb.sum()) <= N * mo.amb_cap(H, W) and int(((p2f != ref['pix_to_face']) & ~amb).sum()) == 0
    clean = ~amb & (p2f == ref['pix_to_face'])
    assert float((image.double() - ref_img).abs().amax(-1)[clean].max()) <= VAL_TOL


@pytest.mark.parametrize('nF', mo.FACE_COUNTS)
def test_shaded_render_at_the_face_counts(nF):
    _check_shade(mo.face_count_scene(nF))


@pytest.mark.parametrize('H,W', mo.IMAGE_SIZES)
def test_shaded_render_at_the_image_sizes(H, W):
    _check_shade(mo.shape_scene(H, W))


def test_vertex_normals_of_degenerate_unreferenced_and_2048_face_vertices():
    sc = mo.exact_scenes()['tiny']
    n = exa.vertex_normals(sc['verts'].to(DEV), sc['faces'].numpy())
    # vertices 0 .. 5: the two tiny faces (area 2^-27 .. 2^-26: below the 1e-6 of the normalisation, so not unit, but along
    # -z or +z exactly); 6 .. 8 collinear, 9 .. 10 the repeated-vertex face, 11 .. 12 unreferenced
    assert bool((n[0, 6:] == 0).all()), 'a vertex without a proper face must keep a zero normal'
    assert bool((n[0, :6, :2] == 0).all()) and bool((n[0, :6, 2] != 0).all())
    sc = mo.fan_scene()
    verts = sc['verts'].to(DEV)
    n1, n2 = exa.vertex_normals(verts, sc['faces'].numpy()), exa.vertex_normals(verts, sc['faces'].numpy())
    assert torch.equal(n1, n2)
    want, raw = so.vertex_normals(verts, sc['faces'])
    d = (n1.double() - torch.from_numpy(want).to(DEV)).abs().amax(-1)[0]
    print('fan2048 normals: centre off by %g, worst %g' % (float(d[mo.FAN_CENTRE]), float(d.max())))
    assert float(d[mo.FAN_CENTRE]) <= VAL_TOL and float(d.max()) <= VAL_TOL
    assert bool((n1[0, torch.tensor(mo.FAN_UNREFERENCED, device=DEV)] == 0).all())
    assert abs(float(n1[0, mo.FAN_CENTRE].norm()) - 1) < 1e-6


def _everything(sc, face):
    """pix_to_face, zbuf, bary and dverts of one call with the topology ``face``."""
    v = sc['verts'].to(DEV).clone().requires_grad_(True)
    fr = exa.get_face_index_map_xy(v, face, _cam(sc), (sc['H'], sc['W']))
    (fr.zbuf.sum() + (fr.bary_coords * torch.tensor([0.5, -1.0, 2.0], device=DEV)).sum()).backward()
    return fr.pix_to_face, fr.zbuf.detach(), fr.bary_coords.detach(), v.grad


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_topology_cache_follows_the_contents_of_face():
    sc = mo.shape_scene(15, 17)
    base = sc['faces'].numpy().astype(np.int64).copy()
    other = np.ascontiguousarray(base[::-1][:, [1, 2, 0]])            # other face order, other corner order
    mesh._topologies.clear()
    first = _everything(sc, base)
    want_other = _everything(sc, other.copy())
    assert not torch.equal(first[0], want_other[0])
    # an in-place edit between two calls: the same object, new contents
    face = base.copy()
    assert _same(_everything(sc, face), first)
    face[:] = other
    assert _same(_everything(sc, face), want_other), 'the second call must follow the edited contents'
    # equal contents in a new object (a tensor, too)
    assert _same(_everything(sc, base.copy()), first)
    assert _same(_everything(sc, torch.from_numpy(base.copy())), first)
    # 20 distinct topologies push the first out of the cache (it is cleared beyond 16 entries); then the first again
    keep = [np.ascontiguousarray(np.roll(base, k, axis=0)) for k in range(1, 21)]
    firsts = [_everything(sc, f) for f in keep]
    assert len(mesh._topologies) <= 17
    assert _same(_everything(sc, base), first)
    assert _same(_everything(sc, keep[0]), firsts[0]) and _same(_everything(sc, keep[-1]), firsts[-1])
    # rolled faces are the same surface: same zbuf, face indices shifted
    F0 = base.shape[0]
    p = firsts[2][0]
    assert torch.equal(torch.where(p >= 0, (p - 3) % F0, p), first[0]) and torch.equal(firsts[2][1], first[1])
