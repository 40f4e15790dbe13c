"""CPU checks of tests/mesh_oracle.py (the restatement the HIP face render is tested against) against answers derived
independently of it (include/exa_mesh.h itself is checked by tests/test_abi.py)."""
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
