"""CPU checks of tests/mesh_oracle.py (the restatement the HIP face render is tested against) against answers derived
independently of it (include/exa_mesh.h itself is checked by tests/test_abi.py)."""
import numpy as np
import pytest
import torch

from exavatar_release_amd import _lib

from tests import mesh_oracle as mo


def _cam(fx, fy, cx, cy):
    return torch.tensor([[fx, fy]], dtype=torch.float64), torch.tensor([[cx, cy]], dtype=torch.float64)


def _unproject(uvz, focal, princpt):
    """camera-space points whose projection is (u, v) at depth z"""
    uvz = torch.as_tensor(uvz, dtype=torch.float64)
    X = (uvz[:, 0] - princpt[0, 0]) * uvz[:, 2] / focal[0, 0]
    Y = (uvz[:, 1] - princpt[0, 1]) * uvz[:, 2] / focal[0, 1]
    return torch.stack((X, Y, uvz[:, 2]), 1)


def test_perspective_bary_and_zbuf_equal_the_ray_triangle_intersection():
    H, W = 20, 24
    focal, princpt = _cam(30.0, 27.0, 11.3, 9.6)
    g = torch.Generator().manual_seed(0)
    tri = torch.tensor([[-0.9, -0.7, 2.0], [1.1, -0.4, 3.5], [0.1, 1.2, 1.4]], dtype=torch.float64)
    tri = tri + 0.05 * torch.randn(3, 3, generator=g, dtype=torch.float64)
    fr = mo.rasterize(tri[None], torch.tensor([[0, 1, 2]]), focal, princpt, H, W)
    cov = torch.nonzero(fr['face'][0] == 0)
    assert cov.shape[0] > 30
    for i, j in cov.tolist():
        # Moeller-Trumbore: origin 0, direction through the pixel centre with unit z
        d = torch.tensor([(j + 0.5 - princpt[0, 0]) / focal[0, 0], (i + 0.5 - princpt[0, 1]) / focal[0, 1], 1.0],
                         dtype=torch.float64)
        e1, e2 = tri[1] - tri[0], tri[2] - tri[0]
        pv = torch.linalg.cross(d, e2)
        det = torch.dot(e1, pv)
        tv = -tri[0]
        u = torch.dot(tv, pv) / det
        qv = torch.linalg.cross(tv, e1)
        v = torch.dot(d, qv) / det
        t = torch.dot(e2, qv) / det
        want = torch.stack((1 - u - v, u, v))
        assert torch.allclose(fr['bary'][0, i, j], want, atol=1e-12, rtol=0)
        assert abs(float(fr['zbuf'][0, i, j] - t)) < 1e-12      # the hit point's z (the ray has unit z)
    assert (fr['bary'][0][fr['face'][0] < 0] == -1).all() and (fr['zbuf'][0][fr['face'][0] < 0] == -1).all()


def test_edge_halfway_between_columns_covers_the_expected_pixels():
    H, W = 12, 16
    focal, princpt = _cam(100.0, 100.0, 8.0, 6.0)
    # screen corners (5, 1), (5, 8), (13, 8): a vertical edge at u = 5, between the centres 4.5 and 5.5; no centre
    # lies on the other two edges (8 (i + .5) = 8 + 7 (j + .5 - 5) has no integer solution)
    verts = _unproject([[5.0, 1.0, 2.0], [5.0, 8.0, 2.0], [13.0, 8.0, 2.0]], focal, princpt)
    fr = mo.rasterize(verts[None], torch.tensor([[0, 1, 2]]), focal, princpt, H, W)
    want = torch.zeros(H, W, dtype=torch.bool)
    for i in range(H):
        for j in range(W):
            x, y = j + 0.5, i + 0.5
            want[i, j] = x > 5 and y < 8 and 8 * (y - 1) > 7 * (x - 5)
    assert want.sum() > 10
    assert torch.equal(fr['face'][0] == 0, want)
    assert not fr['edge_amb'][0].any()


def test_pixel_centres_of_a_non_square_image_with_an_off_centre_principal_point():
    H, W = 6, 10
    focal, princpt = _cam(40.0, 55.0, 3.3, 2.1)
    # a small triangle around screen (7.5, 4.5) = the centre of row 4, column 7, and one around (0.5, 0.5)
    tris = []
    for u0, v0 in ((7.5, 4.5), (0.5, 0.5)):
        tris.append(_unproject([[u0 - 0.3, v0 - 0.2, 1.7], [u0 + 0.3, v0 - 0.2, 1.7], [u0, v0 + 0.3, 1.7]], focal, princpt))
    verts = torch.cat(tris)[None]
    fr = mo.rasterize(verts, torch.tensor([[0, 1, 2], [3, 4, 5]]), focal, princpt, H, W)
    want = torch.full((H, W), -1, dtype=torch.long)
    want[4, 7], want[0, 0] = 0, 1
    assert torch.equal(fr['face'][0], want)
    # all corners at one depth: the perspective-correct barycentrics are the screen ones, solved here from
    # sum_k b_k (u_k, v_k, 1) = (7.5, 4.5, 1)
    M = torch.tensor([[7.2, 7.8, 7.5], [4.3, 4.3, 4.8], [1.0, 1.0, 1.0]], dtype=torch.float64)
    want_b = torch.linalg.solve(M, torch.tensor([7.5, 4.5, 1.0], dtype=torch.float64))
    assert torch.allclose(fr['bary'][0, 4, 7], want_b, atol=1e-12)
    assert abs(float(fr['zbuf'][0, 4, 7]) - 1.7) < 1e-12


def test_nearer_face_wins_and_a_tie_goes_to_the_lower_index():
    H, W = 10, 10
    focal, princpt = _cam(50.0, 50.0, 5.0, 5.0)
    big = [[-1.0, -1.0], [11.0, -1.0], [-1.0, 11.0]]
    near = _unproject([p + [2.0] for p in big], focal, princpt)
    far = _unproject([p + [3.0] for p in big], focal, princpt)
    faces = torch.tensor([[0, 1, 2], [3, 4, 5]])
    for order, nearest in (((far, near), 1), ((near, far), 0)):
        fr = mo.rasterize(torch.cat(order)[None], faces, focal, princpt, H, W)
        cov = fr['face'][0] >= 0
        assert cov.sum() > 40 and (fr['face'][0][cov] == nearest).all()
        assert torch.allclose(fr['zbuf'][0][cov], torch.full_like(fr['zbuf'][0][cov], 2.0))
    # the same triangle twice: exact tie, the lower index wins whatever else the faces hold
    a = _unproject([p + [2.0] for p in big], focal, princpt)
    other = _unproject([[-1.0, -1.0, 2.0], [11.0, -1.0, 2.0], [11.0, 11.0, 2.0]], focal, princpt)
    for faces2, want in ((torch.tensor([[0, 1, 2], [0, 1, 2]]), 0), (torch.tensor([[3, 4, 5], [0, 1, 2], [0, 1, 2]]), None)):
        fr = mo.rasterize(torch.cat((a, other))[None], faces2, focal, princpt, H, W)
        f = fr['face'][0]
        if want is not None:
            assert (f[f >= 0] == 0).all()
        else:   # face 0 (the other triangle, same plane z = 2) overlaps faces 1 and 2 where both cover: 0 wins there
            assert (f[f >= 0] != 2).all() and (f == 0).any() and (f == 1).any()
            assert fr['z_amb'][0][f >= 0].any()


def test_degenerate_and_behind_camera_faces_are_skipped():
    H, W = 8, 8
    focal, princpt = _cam(20.0, 20.0, 4.0, 4.0)
    v = torch.tensor([[-1.0, -1.0, 2.0], [1.0, -1.0, 2.0], [-1.0, 1.0, 2.0], [-1.0, -1.0, -0.5], [0.0, 0.0, 2.0],
                      [1.0, 1.0, 2.0]], dtype=torch.float64)
    faces = torch.tensor([[0, 0, 1], [0, 4, 5], [0, 1, 3], [0, 1, 2]])    # repeated vertex, collinear, behind, fine
    fr = mo.rasterize(v[None], faces, focal, princpt, H, W)
    f = fr['face'][0]
    assert (f[f >= 0] == 3).all() and (f == 3).sum() > 10


def test_oracle_vertex_gradients_match_central_differences():
    H, W = 10, 12
    focal, princpt = _cam(14.0, 13.0, 6.2, 4.9)
    g = torch.Generator().manual_seed(1)
    verts = torch.tensor([[-0.6, -0.5, 2.0], [0.7, -0.35, 2.4], [-0.1, 0.6, 1.7], [0.75, 0.55, 2.6]], dtype=torch.float64)
    faces = torch.tensor([[0, 1, 2], [1, 3, 2]])
    tex = torch.rand(1, 2, 5, 4, generator=g, dtype=torch.float64)
    face_uvs = 0.1 + 0.8 * torch.rand(2, 3, 2, generator=g, dtype=torch.float64)
    Gb = torch.randn(1, H, W, 3, generator=g, dtype=torch.float64)
    Gz = torch.randn(1, H, W, generator=g, dtype=torch.float64)
    Gr = torch.randn(1, 2, H, W, generator=g, dtype=torch.float64)

    def loss(v):
        out, fr = mo.render(v[None], faces, focal, princpt, H, W, tex, face_uvs)
        return (fr['bary'] * Gb).sum() + (fr['zbuf'] * Gz).sum() + (out * Gr).sum(), fr

    v = verts.clone().requires_grad_(True)
    L, fr = loss(v)
    assert not fr['edge_amb'].any() and (fr['face'] >= 0).sum() > 20
    L.backward()
    num = torch.zeros_like(verts)
    h = 1e-7
    for i in range(verts.shape[0]):
        for k in range(3):
            vp, vm = verts.clone(), verts.clone()
            vp[i, k] += h
            vm[i, k] -= h
            (lp, fp), (lm, fm) = loss(vp), loss(vm)
            assert torch.equal(fp['face'], fr['face']) and torch.equal(fm['face'], fr['face'])
            num[i, k] = (lp - lm) / (2 * h)
    assert torch.allclose(v.grad, num, rtol=1e-5, atol=1e-6 * float(num.abs().max()))


def test_workspace_sizes_and_argument_checks():
    s = _lib.mesh_workspace_sizes(2, 10240, 1024, 1024)
    assert s.face_bytes == 2 * 10240 * 64 and s.bin_bytes == 2 * 256 * 320 * 4 and s.grad_bytes == 2 * 10240 * 36
    with pytest.raises(RuntimeError, match='negative'):
        _lib.mesh_workspace_sizes(-1, 1, 1, 1)
    with pytest.raises(RuntimeError, match='8192'):
        _lib.mesh_workspace_sizes(1, 1, 9000, 10)


# ---- the scene builders of tests/test_gpu_mesh_edges.py ------------------------------------------------------------------

def _raster32(sc):
    """One mesh, decided in float32 numpy the way the kernel states it: b_k = E_k * (1 / A) with E_k the float32 edge
    functions, inside when all three b_k > 0, nearest float32 z, strict < in index order.  Returns (face [H,W], number of
    covering faces [H,W], (whether every float32 area is exact and every (face, pixel) is decided by float32 edge
    functions that have the sign -- zero included -- of their float64 values, whether the edge functions are the same numbers))."""
    H, W = sc['H'], sc['W']
    v = sc['verts'][0].numpy()
    f32 = np.float32
    fx, fy = sc['focal'][0].numpy()
    cx, cy = sc['princpt'][0].numpy()
    py, px = np.meshgrid(np.arange(H, dtype=f32) + f32(0.5), np.arange(W, dtype=f32) + f32(0.5), indexing='ij')
    face = np.full((H, W), -1, dtype=np.int64)
    best = np.full((H, W), np.inf, dtype=f32)
    count = np.zeros((H, W), dtype=np.int64)
    exact = bits = True
    with np.errstate(all='ignore'):
        for i, tri in enumerate(sc['faces'].numpy()):
            X, Y, Z = v[tri, 0], v[tri, 1], v[tri, 2]
            x, y = fx * (X / Z) + cx, fy * (Y / Z) + cy                       # float32
            xd, yd = x.astype(np.float64), y.astype(np.float64)

            def edges(x, y, px, py):
                e = [(x[a] - px) * (y[b] - py) - (y[a] - py) * (x[b] - px) for a, b in ((1, 2), (2, 0), (0, 1))]
                return e, (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
            e, A = edges(x, y, px, py)
            if not (np.all(Z > mo.MIN_Z) and np.isfinite(A) and abs(A) >= mo.MIN_AREA and np.all(np.isfinite(x)) and np.all(np.isfinite(y))):
                continue
            ed, Ad = edges(xd, yd, px.astype(np.float64), py.astype(np.float64))
            # every scene but 'tiny' has few enough bits for exact products; at 2^-13 px the products at far pixels need more
            # than 24 bits, and what a decision needs is the SIGN (zero included) of all three edge functions, or of one that
            # says "outside" (on the line through the tiny face's hypotenuse the true value is 2^-27 against products of ~4)
            bits = bits and all(np.array_equal(a.astype(np.float64), b) for a, b in zip(e, ed))
            same = [np.sign(a) == np.sign(b) for a, b in zip(e, ed)]
            out = [m & (np.sign(b) * np.sign(Ad) <= 0) for m, b in zip(same, ed)]          # a right sign that says "outside"
            exact = exact and float(A) == Ad and bool(((same[0] & same[1] & same[2]) | out[0] | out[1] | out[2]).all())
            assert e[0].dtype == f32
            inv = f32(1) / A
            b = [ek * inv for ek in e]
            inside = (b[0] > 0) & (b[1] > 0) & (b[2] > 0)
            w = [b[k] / Z[k] for k in range(3)]
            S = w[0] + w[1] + w[2]
            z = (w[0] / S) * Z[0] + (w[1] / S) * Z[1] + (w[2] / S) * Z[2]
            take = inside & (z < best)
            face[take], best[take] = i, z[take]
            count += inside
    return face, count, (exact, bits)


def _all_exact():
    return dict(mo.exact_scenes(), culled=mo.culled_scene())


@pytest.mark.parametrize('name', sorted(_all_exact()))
def test_exact_scenes_decide_alike_in_float32_and_float64(name):
    sc = _all_exact()[name]
    fr = mo.oracle_of(sc)
    face32, _, (exact, bits) = _raster32(sc)
    assert exact, 'a decision rests on a float32 edge function of the wrong sign: the scene is not exact'
    assert bits or name == 'tiny', 'a float32 edge function is rounded'
    assert np.array_equal(face32, fr['face'][0].numpy())


def test_exact_scenes_give_the_hand_derived_answers():
    S = mo.exact_scenes()
    inner = torch.zeros(12, 12, dtype=torch.bool)
    for i in range(3, 8):
        for j in range(3, 8):
            inner[i, j] = i != j              # strictly inside the quad and off its diagonal
    for name in ('quad_ccw', 'quad_cw'):
        f = mo.oracle_of(S[name])['face'][0]
        assert torch.equal(f >= 0, inner)
        # corner 2 of face 0 and corner 1 of face 1 of the ccw quad is (8.5, 2.5): above the diagonal -> columns > rows
        jj, ii = torch.meshgrid(torch.arange(12), torch.arange(12), indexing='xy')
        assert torch.equal(f[inner], torch.where(jj > ii, 0, 1)[inner])
    f = mo.oracle_of(S['fan8'])['face'][0]
    _, count, _ = _raster32(S['fan8'])
    assert f[6, 6] == -1 and count[6, 6] == 0                   # the fan's centre is the centre of pixel (6, 6)
    ring = [(6 + di, 6 + dj) for di in (-1, 0, 1) for dj in (-1, 0, 1) if (di, dj) != (0, 0)]
    assert all(f[i, j] >= 0 and count[i, j] == 1 for i, j in ring), 'a hole or a double cover next to the centre'
    assert set(f.flatten().tolist()) == set(range(-1, 8))
    assert int((count > 1).sum()) == 0
    f = mo.oracle_of(S['stack'])['face'][0]
    tri = torch.zeros(16, 16, dtype=torch.bool)
    for i in range(16):
        for j in range(16):
            tri[i, j] = i >= 1 and j >= 1 and i + j < 14        # centres with x > 1, y > 1, x + y < 15
    assert torch.equal(f == 2, tri) and not bool(((f == 5) | (f == 9)).any())
    assert bool((f == 0).any()) and bool((f == 1).any()) and bool((f == 3).any())
    f2 = mo.oracle_of(S['stacks2'])['face'][0]
    assert torch.equal(f2 == 4, tri) and not bool(torch.isin(f2, torch.tensor([1, 3, 6, 7, 8])).any())
    want = torch.full((8, 8), -1, dtype=torch.long)
    want[2, 2] = 0
    assert torch.equal(mo.oracle_of(S['tiny'])['face'][0], want)
    fr = mo.oracle_of(mo.culled_scene())
    f = fr['face'][0]
    assert set(f.flatten().tolist()) == {-1, 0} and int((f == 0).sum()) > 10
    assert bool(torch.isfinite(fr['bary']).all()) and bool(torch.isfinite(fr['zbuf']).all())


def _shape_cases():
    return [('faces%d' % F, mo.face_count_scene, (F,)) for F in mo.FACE_COUNTS] + \
        [('image%dx%d' % hw, mo.shape_scene, hw) for hw in mo.IMAGE_SIZES] + \
        [('batch3', mo.batch_scene, (3,)), ('batch1', mo.batch_scene, (1,)), ('offscreen', mo.offscreen_scene, ()),
         ('far_corner', mo.far_corner_scene, ()), ('strip', mo.strip_scene, ()), ('depth', mo.depth_scene, ()),
         ('crossing', mo.crossing_scene, ()), ('fan', mo.fan_scene, ())] + \
        [('sampler%dx%d' % m, mo.sampler_scene, (3,) + m) for m in mo.SAMPLER_MAPS]


@pytest.mark.parametrize('name,fn,args', _shape_cases(), ids=[c[0] for c in _shape_cases()])
def test_shape_scenes_stay_under_the_ambiguity_cap(name, fn, args):
    sc = fn(*args)
    H, W = sc['H'], sc['W']
    fr = mo.oracle_of(sc, block=8 if name.startswith('faces') else 32)
    n = int((fr['edge_amb'] | fr['z_amb']).sum())
    assert n == sc['n_amb'] and n <= mo.amb_cap(H, W)
    if H * W < 1000 or name.startswith(('faces', 'image', 'batch', 'offscreen', 'far', 'strip', 'sampler')):
        assert n == 0, 'the GPU test excludes nothing in this case'
    assert mo.amb_cap(30, 30) == 0 and mo.amb_cap(1, 37) == 0 and mo.amb_cap(32, 48) == 1 and mo.amb_cap(130, 70) == 9


@pytest.mark.parametrize('F', mo.FACE_COUNTS)
def test_face_count_scenes_show_the_faces_the_mask_words_end_on(F):
    sc = mo.face_count_scene(F)
    assert sc['faces'].shape[0] == F
    fr = mo.oracle_of(sc, block=8)
    f = fr['face'][0]
    if F == 0:
        assert bool((f == -1).all())
        return
    last = f == F - 1
    assert int(last[:, 40:].sum()) > 50, 'face F - 1 must be the only cover somewhere'
    assert bool((f[:, 40:][~last[:, 40:]] == -1).all())
    shown = set(f.flatten().tolist()) - {-1}
    if F > 1:
        assert int((f[:, :40] >= 0).sum()) > int(last[:, :40].sum())
    if F >= 8191:
        # face F - 1 is the NEAREST of several covers on some pixels: recount the covers there
        _, count, _ = _raster32(sc)
        assert int((last.numpy() & (count > 1)).sum()) > 0
        assert len([i for i in shown if i % 32 == 31]) > 20 and len(shown) > 1000
    if F >= 33:
        assert 31 in shown


def test_off_screen_faces_own_no_pixel_and_the_strip_face_sits_near_column_1050():
    f = mo.oracle_of(mo.offscreen_scene())['face'][0]
    assert set(f.flatten().tolist()) == {-1, 0}
    f = mo.oracle_of(mo.strip_scene())['face'][0]
    cols = torch.nonzero((f == 0).any(0)).flatten()
    assert int(cols.min()) >= 1048 and int(cols.max()) <= 1052 and bool((f == 1).any())
    f = mo.oracle_of(mo.far_corner_scene())['face'][0]
    assert int((f == 0).sum()) > 50 and int((f == 1).sum()) > 50
    f = mo.oracle_of(mo.crossing_scene())['face'][0]
    assert int((f == 0).sum()) > 300 and int((f == 1).sum()) > 300 and not bool((f < 0).any())
    f = mo.oracle_of(mo.depth_scene())['face'][0]
    assert len(set(f.flatten().tolist())) >= 25


def test_fan_scene_has_one_long_vertex_list_and_unreferenced_vertices():
    sc = mo.fan_scene()
    faces = sc['faces']
    assert faces.shape[0] == 2048 and bool((faces == mo.FAN_CENTRE).any(1).all())
    assert not bool(torch.isin(faces, torch.tensor(mo.FAN_UNREFERENCED)).any())
    assert sc['verts'].shape[1] == max(mo.FAN_UNREFERENCED) + 1
    f = mo.oracle_of(sc)['face'][0]
    assert len(set(f.flatten().tolist())) > 1000            # the centre's gradient is a sum over > 1000 live faces


def test_sampler_scene_clamps_where_it_says():
    sc = mo.sampler_scene(3, 16, 16)
    fuv = mo.face_uvs_of(sc['vertex_uv'], sc['face_uv']).double()                # what the sampler sees
    for q, (ua, ub, va, vb) in enumerate(mo.UV_PATTERNS):
        got = fuv[2 * q:2 * q + 2].reshape(-1, 2)
        assert set(got[:, 0].tolist()) == {ua, ub} and set(got[:, 1].tolist()) == {va, vb}, 'the flip of v must be exact'
        clamped_u, clamped_v = max(ua, ub) <= 0 or min(ua, ub) >= 1, max(va, vb) <= 0 or min(va, vb) >= 1
        assert (clamped_u and clamped_v) == (q >= mo.FIRST_CLAMPED_PATTERN)
    f = mo.oracle_of(sc)['face'][0]
    assert set(f.flatten().tolist()) == set(range(-1, 32))


def test_float32_revalue_keeps_the_winners_and_differs_by_rounding_only():
    sc = mo.shape_scene(15, 17)
    args = (sc['faces'], sc['focal'], sc['princpt'])
    v64 = sc['verts'].double().requires_grad_(True)
    fr = mo.rasterize(v64, *args, sc['H'], sc['W'])
    v32 = sc['verts'].clone().requires_grad_(True)
    fr32 = mo.revalue(fr, v32, *args)
    assert fr32['bary'].dtype == torch.float32 and fr32['face'] is fr['face']
    assert float((fr32['bary'].double() - fr['bary']).detach().abs().max()) < 1e-5
    fuv = mo.face_uvs_of(sc['vertex_uv'], sc['face_uv'])
    out64, _ = mo.render(v64, *args, sc['H'], sc['W'], sc['texture'], fuv, frags=fr)
    out32, _ = mo.render(v32, *args, sc['H'], sc['W'], sc['texture'], fuv, frags=fr32)
    assert out64.dtype == torch.float64 and out32.dtype == torch.float32
    G = torch.randn(out64.shape, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    (out64 * G).sum().backward()
    (out32 * G.float()).sum().backward()
    rel = float((v32.grad.double() - v64.grad).norm() / v64.grad.norm())
    assert 0 < rel < 1e-4
