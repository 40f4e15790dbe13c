"""Brute-force float64 restatement of the face render (``exavatar_release_amd.mesh``), differentiable by autograd.

Test infrastructure only: the package never imports it.  The semantics are those of the docstring of
``exavatar_release_amd/mesh.py``: every pixel centre (j + 0.5, i + 0.5) tested against every face (a face whose screen
bbox misses a block of pixels cannot contain any of their centres, so blocks only meet the faces whose bbox they touch),
all three screen barycentrics > 0, nearest perspective-correct z and the lower index on a tie, then the uv interpolation
and ``F.grid_sample`` of the flipped map.  Works on any device (the GPU tests run it on the GPU in float64).  ``revalue``
repeats the differentiable half in float32 at the float64 winners (the yardstick of tests/test_gpu_mesh_edges.py's
gradient checks); the scene builders of that module are at the end of this file.
"""
import functools
import math

import torch
import torch.nn.functional as F

MIN_Z = 1e-6
MIN_AREA = 1e-8
EDGE_EPS = 1e-5       # a pixel centre this close (in barycentric units) to a covering face's edge is ambiguous
Z_EPS = 1e-6          # two covering faces whose z differ by less than this (relative) make a pixel ambiguous


def project(verts, focal, princpt):
    """verts [N,V,3] camera space -> screen x, y [N,V] and z [N,V]: u = fx X / Z + cx, v = fy Y / Z + cy."""
    X, Y, Z = verts[..., 0], verts[..., 1], verts[..., 2]
    return focal[:, 0:1] * X / Z + princpt[:, 0:1], focal[:, 1:2] * Y / Z + princpt[:, 1:2], Z


def _corners(verts, faces, focal, princpt):
    x, y, z = project(verts, focal, princpt)
    return x[:, faces], y[:, faces], z[:, faces]          # each [N, F, 3]


def _bary(fx, fy, px, py):
    """screen barycentrics of pixel centres (px, py) in faces with corners (fx, fy) [..., 3]: b_k = E_k / A."""
    def cross(k1, k2):
        return (fx[..., k1] - px) * (fy[..., k2] - py) - (fy[..., k1] - py) * (fx[..., k2] - px)
    area = (fx[..., 1] - fx[..., 0]) * (fy[..., 2] - fy[..., 0]) - (fy[..., 1] - fy[..., 0]) * (fx[..., 2] - fx[..., 0])
    e = torch.stack((cross(1, 2), cross(2, 0), cross(0, 1)), -1)
    return e / area[..., None]


def _perspective(b, z):
    w = b / z
    p = w / w.sum(-1, keepdim=True)
    return p, (p * z).sum(-1)


def rasterize(verts, faces, focal, princpt, H, W, block=32):
    """verts [N,V,3], faces [F,3] int64, focal / princpt [N,2]; all converted to float64.

    Returns a dict: ``pix_to_face`` [N,H,W] (packed n * F + f, -1), ``face`` [N,H,W] (unpacked, -1), ``bary`` [N,H,W,3]
    and ``zbuf`` [N,H,W] (-1 at background; differentiable in ``verts``), ``edge_amb`` / ``z_amb`` [N,H,W] bool."""
    verts = verts.double()
    focal, princpt = focal.double().reshape(-1, 2).expand(verts.shape[0], 2), princpt.double().reshape(-1, 2).expand(verts.shape[0], 2)
    faces = faces.long().to(verts.device)
    N, nF = verts.shape[0], faces.shape[0]
    dev = verts.device
    face = torch.full((N, H, W), -1, dtype=torch.long, device=dev)
    edge_amb = torch.zeros((N, H, W), dtype=torch.bool, device=dev)
    z_amb = torch.zeros((N, H, W), dtype=torch.bool, device=dev)
    with torch.no_grad():
        cx, cy, cz = _corners(verts, faces, focal, princpt)
        area = (cx[..., 1] - cx[..., 0]) * (cy[..., 2] - cy[..., 0]) - (cy[..., 1] - cy[..., 0]) * (cx[..., 2] - cx[..., 0])
        valid = (cz > MIN_Z).all(-1) & (area.abs() >= MIN_AREA) & torch.isfinite(area) & \
            torch.isfinite(cx).all(-1) & torch.isfinite(cy).all(-1)
        for n in range(N):
            ids = torch.nonzero(valid[n]).flatten()
            if ids.numel() == 0:
                continue
            fxn, fyn, fzn = cx[n, ids], cy[n, ids], cz[n, ids]
            x0, x1 = fxn.min(-1).values - 1, fxn.max(-1).values + 1
            y0, y1 = fyn.min(-1).values - 1, fyn.max(-1).values + 1
            for r0 in range(0, H, block):
                for c0 in range(0, W, block):
                    r1, c1 = min(r0 + block, H), min(c0 + block, W)
                    sel = torch.nonzero((x1 >= c0) & (x0 <= c1) & (y1 >= r0) & (y0 <= r1)).flatten()
                    if sel.numel() == 0:
                        continue
                    yy, xx = torch.meshgrid(torch.arange(r0, r1, device=dev), torch.arange(c0, c1, device=dev), indexing='ij')
                    px, py = (xx.flatten().double() + 0.5)[:, None], (yy.flatten().double() + 0.5)[:, None]
                    b = _bary(fxn[sel][None], fyn[sel][None], px, py)                 # [P, Fc, 3]
                    inside = (b > 0).all(-1)
                    _, zp = _perspective(b, fzn[sel][None])
                    zs = torch.where(inside, zp, torch.full_like(zp, math.inf))
                    zmin = zs.min(1).values
                    idx = ids[sel][None].expand_as(zs)
                    win = torch.where(inside & (zs == zmin[:, None]), idx, torch.full_like(idx, nF)).min(1).values
                    win = torch.where(win == nF, torch.full_like(win, -1), win)
                    near = ((b > -EDGE_EPS).all(-1) & (b.min(-1).values < EDGE_EPS)).any(1)
                    close = (inside & (zs <= zmin[:, None] * (1 + Z_EPS))).sum(1) >= 2
                    face[n, r0:r1, c0:c1] = win.view(r1 - r0, c1 - c0)
                    edge_amb[n, r0:r1, c0:c1] = near.view(r1 - r0, c1 - c0)
                    z_amb[n, r0:r1, c0:c1] = close.view(r1 - r0, c1 - c0)
    bary, zbuf = _values(verts, faces, focal, princpt, face)
    packed = torch.where(face >= 0, face + torch.arange(N, device=dev)[:, None, None] * nF, face)
    return {'pix_to_face': packed, 'face': face, 'bary': bary, 'zbuf': zbuf, 'edge_amb': edge_amb, 'z_amb': z_amb}


def _values(verts, faces, focal, princpt, face):
    """The winners' barycentrics [N,H,W,3] and z [N,H,W] (-1 at background) through autograd, in ``verts``' dtype."""
    N, H, W = face.shape
    dev, dt = verts.device, verts.dtype
    cov = face >= 0
    nn_, ii, jj = torch.nonzero(cov, as_tuple=True)
    ff = face[cov]
    x, y, z = project(verts, focal, princpt)
    fv = faces[ff]                                                      # [K, 3]
    b = _bary(x[nn_[:, None], fv], y[nn_[:, None], fv], jj.to(dt) + 0.5, ii.to(dt) + 0.5)
    p, zp = _perspective(b, z[nn_[:, None], fv])
    bary = torch.full((N, H, W, 3), -1.0, dtype=dt, device=dev).index_put((nn_, ii, jj), p)
    zbuf = torch.full((N, H, W), -1.0, dtype=dt, device=dev).index_put((nn_, ii, jj), zp)
    return bary, zbuf


def revalue(frags, verts, faces, focal, princpt, dtype=torch.float32):
    """The differentiable half of ``rasterize`` again in ``dtype``: the winners stay those of ``frags`` (a float64 run),
    the barycentrics and z -- and whatever ``render(..., frags=...)`` builds on them -- are evaluated, and differentiated
    by autograd, in ``dtype``.  The float32 run is the yardstick of the gradient checks: its error against the float64
    run is what one float32 evaluation of these expressions costs."""
    N = verts.shape[0]
    verts = verts.to(dtype)
    focal, princpt = focal.to(dtype).reshape(-1, 2).expand(N, 2), princpt.to(dtype).reshape(-1, 2).expand(N, 2)
    bary, zbuf = _values(verts, faces.long().to(verts.device), focal, princpt, frags['face'])
    return dict(frags, bary=bary, zbuf=zbuf)


def render(verts, faces, focal, princpt, H, W, texture, face_uvs, frags=None):
    """TexturesUV.sample_textures of the reference's MeshRenderer, background -1: texture [1 or N, C, Ht, Wt], face_uvs
    [F,3,2] (pytorch3d's uv, v up).  Returns (render [N,C,H,W], fragments dict): float64, or the dtype of ``revalue``'s
    fragments when ``frags`` come from there."""
    if frags is None:
        frags = rasterize(verts, faces, focal, princpt, H, W)
    N = verts.shape[0]
    face = frags['face']
    cov = face >= 0
    dt = frags['bary'].dtype                                            # float64, or revalue's
    uvs = face_uvs.to(dt).to(verts.device)[face.clamp_min(0)]           # [N,H,W,3,2]
    uv = (frags['bary'].clamp_min(0)[..., None] * uvs).sum(-2)
    uv = torch.where(cov[..., None], uv, torch.zeros_like(uv))
    tex = texture.to(dt).to(verts.device).expand(N, -1, -1, -1)
    out = F.grid_sample(torch.flip(tex, [2]), uv * 2.0 - 1.0, mode='bilinear', padding_mode='border', align_corners=True)
    out = torch.where(cov[:, None], out, torch.full_like(out, -1.0))
    return out, frags


# ---- test scenes -------------------------------------------------------------------------------------------------------
def icosphere(level):
    """Unit icosphere: the icosahedron subdivided ``level`` times (p3d_standins.SubdivideMeshes), re-projected onto the
    sphere after every step.  level 4: 2 562 vertices, 5 120 faces."""
    from exavatar_release_amd.p3d_standins import Meshes, SubdivideMeshes
    t = (1.0 + 5 ** 0.5) / 2
    v = torch.tensor([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                      [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=torch.float64)
    f = torch.tensor([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2],
                      [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11],
                      [6, 2, 10], [8, 6, 7], [9, 8, 1]], dtype=torch.int64)
    v = v / v.norm(dim=1, keepdim=True)
    for _ in range(level):
        m = SubdivideMeshes()(Meshes(v[None], f[None]))
        v, f = m.verts_padded()[0], m.faces_padded()[0]
        v = v / v.norm(dim=1, keepdim=True)
    return v, f


def flame_sized_scene(H, W, seed=0, N=1):
    """~FLAME-sized face mesh (5 124 vertices, 10 240 faces): two perturbed level-4 icospheres, the second partly behind
    the first, in front of a pinhole camera that frames them at H x W.  Returns a dict of float32 CPU tensors: verts
    [N,V,3] (camera space), faces [F,3], focal / princpt [N,2], texture [1,4,256,256] (RGB + a 0/1 mask), vertex_uv
    [V,2] and face_uv [F,3] (a different index set from faces)."""
    g = torch.Generator().manual_seed(seed)
    v, f = icosphere(4)
    V = v.shape[0]
    parts, faces = [], []
    for k, (c, r) in enumerate((((0.0, 0.0, 3.0), 0.8), ((0.45, 0.25, 3.7), 0.6))):
        bump = 1 + 0.03 * torch.randn(V, 1, generator=g, dtype=torch.float64)
        parts.append(v * bump * r + torch.tensor(c, dtype=torch.float64))
        faces.append(f + k * V)
    verts = torch.cat(parts)[None].repeat(N, 1, 1)
    for n in range(1, N):
        verts[n] += 0.05 * n * torch.tensor([1.0, -0.5, 0.2], dtype=torch.float64)
    faces = torch.cat(faces)
    s = min(H, W)
    focal = torch.tensor([[1.4 * s, 1.4 * s]], dtype=torch.float64).repeat(N, 1)
    princpt = torch.tensor([[W / 2 + 0.37, H / 2 - 0.21]], dtype=torch.float64).repeat(N, 1)
    # spherical uv (slightly beyond [0, 1] so the border clamp is exercised), stored under a permuted index set
    p = torch.cat([v, v])
    uv = torch.stack(((torch.atan2(p[:, 1], p[:, 0]) / (2 * math.pi) + 0.5), torch.acos(p[:, 2].clamp(-1, 1)) / math.pi), 1)
    uv = uv * 1.04 - 0.02
    perm = torch.randperm(2 * V, generator=g)
    vertex_uv = torch.empty_like(uv)
    vertex_uv[perm] = uv
    face_uv = perm[faces]
    # a smooth texture (|d value / d uv| <= ~3): fp32 uv carries ~1e-6 of rounding, so the render's 1e-5 bar measures
    # the sampler, not the texture's steepness.  Channel 3 is a mask with a plateau of exact 1.0 and linear ramps.
    tt = torch.linspace(0, 1, 256, dtype=torch.float64)
    tv, tu = torch.meshgrid(tt, tt, indexing='ij')
    ph = torch.rand(3, generator=g, dtype=torch.float64) * 2 * math.pi
    tex = torch.stack([0.5 + 0.25 * torch.sin(2 * math.pi * (0.7 * tu + 0.4 * tv * (c + 1) / 3) + ph[c]) for c in range(3)]
                      + [(2.5 - 3.0 * ((tu - 0.5).abs() + (tv - 0.45).abs())).clamp(0, 1)])[None]
    f32 = lambda t: t.float()      # noqa: E731
    return {'verts': f32(verts), 'faces': faces, 'focal': f32(focal), 'princpt': f32(princpt), 'texture': f32(tex),
            'vertex_uv': f32(vertex_uv), 'face_uv': face_uv}


def face_uvs_of(vertex_uv, face_uv):
    """The corner uvs MeshRenderer.forward hands the sampler: vertex_uv with v flipped (layer.py:53), per face."""
    vu = torch.stack((vertex_uv[:, 0], 1 - vertex_uv[:, 1]), 1)
    return vu[face_uv]


# ---- scenes of tests/test_gpu_mesh_edges.py ----------------------------------------------------------------------------
# Every builder returns a dict of float32 CPU tensors -- verts [N,V,3], faces [F,3], focal / princpt [N,2] -- plus 'H', 'W'
# and, where the render is tested, texture [1 or N,C,Ht,Wt], vertex_uv [U,2], face_uv [F,3].  The builders run the float64
# oracle on the CPU and are cached: the tests treat their results as read-only.
AMB_MAX_FRACTION = 1e-3       # the cap of tests/test_gpu_mesh.py on oracle-ambiguous pixels ...


def amb_cap(H, W):
    """... as a pixel count; ZERO for an image of fewer than 1000 pixels (one pixel of 900 would be more than 0.1 %)."""
    return 0 if H * W < 1000 else int(AMB_MAX_FRACTION * H * W)


def unproject(uvz, focal, princpt):
    """camera-space points [K,3] (float64) whose projection is the screen point (u, v) at depth z, rows of ``uvz``."""
    uvz = torch.as_tensor(uvz, dtype=torch.float64).reshape(-1, 3)
    return torch.stack(((uvz[:, 0] - princpt[0]) * uvz[:, 2] / focal[0], (uvz[:, 1] - princpt[1]) * uvz[:, 2] / focal[1],
                        uvz[:, 2]), 1)


def _scene(verts, faces, focal, princpt, H, W, **extra):
    verts = torch.as_tensor(verts, dtype=torch.float64)
    verts = verts[None] if verts.dim() == 2 else verts
    N = verts.shape[0]
    cam = lambda c: torch.as_tensor(c, dtype=torch.float64).reshape(-1, 2).expand(N, 2).float().contiguous()  # noqa: E731
    faces = torch.as_tensor(faces, dtype=torch.int64).reshape(-1, 3)
    return dict({'verts': verts.float(), 'faces': faces, 'focal': cam(focal), 'princpt': cam(princpt), 'H': H, 'W': W}, **extra)


def oracle_of(sc, block=32):
    """``rasterize`` of a scene dict on the scene's own device."""
    return rasterize(sc['verts'], sc['faces'], sc['focal'], sc['princpt'], sc['H'], sc['W'], block=block)


def _first_clean(build, cap=0, block=32, seeds=64):
    """The scene of the first seed whose float64 oracle calls at most ``cap`` pixels ambiguous (``n_amb`` of them)."""
    for seed in range(seeds):
        sc = build(seed)
        fr = oracle_of(sc, block)
        n = int((fr['edge_amb'] | fr['z_amb']).sum())
        if n <= cap:
            return dict(sc, seed=seed, n_amb=n)
    raise RuntimeError('no seed below %d gives a scene with at most %d ambiguous pixels' % (seeds, cap))


def smooth_texture(n, C, tH, tW, seed=0):
    """[n,C,tH,tW] float64: bilinear ramps with slopes below 1 per unit of uv (fp32 uv carries ~1e-6 of rounding; the
    1e-5 bar then measures the sampler, not the map's steepness); the last channel is a mask with a plateau of exact
    1.0 and linear ramps to 0, as the reference's face mask.  Map k > 0 differs from map 0 in every channel."""
    g = torch.Generator().manual_seed(1000 + seed)
    tv, tu = torch.meshgrid(torch.linspace(0, 1, tH, dtype=torch.float64) if tH > 1 else torch.zeros(1, dtype=torch.float64),
                            torch.linspace(0, 1, tW, dtype=torch.float64) if tW > 1 else torch.zeros(1, dtype=torch.float64),
                            indexing='ij')
    maps = []
    for k in range(n):
        co = torch.rand(C, 4, generator=g, dtype=torch.float64)
        ch = [0.2 + 0.3 * co[c, 0] + 0.4 * co[c, 1] * tu + 0.4 * co[c, 2] * tv - 0.3 * co[c, 3] * tu * tv for c in range(C - 1)]
        ch.append((1.6 - 0.25 * k - 2 * (tu - tv).abs()).clamp(0, 1))
        maps.append(torch.stack(ch))
    return torch.stack(maps)


def _with_uv(sc, seed, tex_N=1, C=4, tH=16, tW=16):
    """random vertex uvs a little beyond [0, 1] (a permuted index set, as FLAME's) and ``tex_N`` smooth maps"""
    g = torch.Generator().manual_seed(77 + seed)
    V = sc['verts'].shape[1]
    perm = torch.randperm(V, generator=g)
    uv = torch.rand(V, 2, generator=g, dtype=torch.float64) * 1.1 - 0.05
    vertex_uv = torch.empty_like(uv)
    vertex_uv[perm] = uv
    return dict(sc, texture=smooth_texture(tex_N, C, tH, tW, seed).float(), vertex_uv=vertex_uv.float(), face_uv=perm[sc['faces']])


# -- A. exact scenes: focal 1, every Z a power of two, princpt and every screen corner dyadic with few bits.  X = (u - cx) Z
# is then exact in float32, the projection returns u exactly, and every edge function is an exact product in float32 and
# float64 alike: no decision is ambiguous, not even a pixel centre ON an edge (tests/test_mesh_oracle.py proves it).
EXACT_CAM = ((1.0, 1.0), (3.5, 2.25))


def _exact(tris, H, W, faces=None, extra_verts=0):
    """tris: list of three (u, v, z) corners each; one vertex per distinct corner in order of appearance"""
    pts, index, fl = [], {}, []
    for t in tris:
        ids = []
        for c in t:
            c = tuple(float(x) for x in c)
            if c not in index:
                index[c] = len(pts)
                pts.append(c)
            ids.append(index[c])
        fl.append(ids)
    verts = unproject(pts, *EXACT_CAM)
    verts = torch.cat([verts, torch.tensor([[0.25, -0.5, 2.0]], dtype=torch.float64).repeat(extra_verts, 1)])
    sc = _scene(verts, fl if faces is None else faces, EXACT_CAM[0], EXACT_CAM[1], H, W)
    assert torch.equal(sc['verts'][0].double(), verts), 'an exact scene must survive the cast to float32'
    return sc


@functools.lru_cache(maxsize=None)
def exact_scenes():
    """name -> scene (ISSUE A.1 - A.4; A.5 is ``culled_scene``).  What each must give is asserted in test_mesh_oracle.py."""
    out = {}
    # 1. a quad whose outer edges, diagonal and corners all pass through pixel centres; both windings
    q = [(2.5, 2.5, 2), (8.5, 2.5, 2), (8.5, 8.5, 2), (2.5, 8.5, 2)]
    out['quad_ccw'] = _exact([(q[0], q[1], q[2]), (q[0], q[2], q[3])], 12, 12)
    out['quad_cw'] = _exact([(q[0], q[2], q[1]), (q[0], q[3], q[2])], 12, 12)
    # 2. a fan of 8 faces around the pixel centre (6.5, 6.5); the spokes miss the centres of the 8 neighbours
    c = (6.5, 6.5, 4)
    ring = [(4.5, 1), (3.5, 3), (-1, 4.5), (-3, 3.5), (-4.5, -1), (-3.5, -3), (1, -4.5), (3, -3.5)]
    ring = [(c[0] + dx, c[1] + dy, 4) for dx, dy in ring]
    out['fan8'] = _exact([(c, ring[k], ring[(k + 1) % 8]) for k in range(8)], 13, 13)
    # 3. the same face three times at scattered indices among others; then a far stack below a near one in index order
    T1 = ((1, 1, 1), (14, 1, 1), (1, 14, 1))
    T2 = ((1, 1, 2), (14, 1, 2), (1, 14, 2))
    o1 = ((6, 6, 4), (15, 7, 4), (7, 15, 4))
    o2 = ((0, 9, 4), (9, 12, 4), (2, 16, 4))
    o3 = ((9, 0, 8), (16, 2, 8), (12, 9, 8))
    out['stack'] = _exact([o1, o2, T1, o3, o1, T1, o2, o3, o1, T1], 16, 16)
    out['stacks2'] = _exact([o1, T2, o2, T2, T1, o3, T2, T1, T1, o1], 16, 16)
    # 4. |A| = 2^-26 >= MIN_AREA around the centre (2.5, 2.5): drawn; |A| = 2^-27 < MIN_AREA around (5.5, 5.5): skipped; a
    # collinear face and a repeated-vertex face; two vertices that no face references
    e = 2.0 ** -13
    a0, b0 = 2.5 - e / 4, 5.5 - e / 8
    out['tiny'] = _exact([((a0, a0, 1), (a0 + e, a0, 1), (a0, a0 + e, 1)), ((b0, b0, 1), (b0 + e, b0, 1), (b0, b0 + e / 2, 1)),
                          ((1, 6, 2), (2, 6, 2), (3.5, 6, 2)), ((6, 1, 2), (6, 1, 2), (7, 3, 2))], 8, 8, extra_verts=2)
    return out


@functools.lru_cache(maxsize=None)
def culled_scene():
    """ISSUE A.5: one good face (0) and six faces culled outright, each on vertices of its own: a corner at Z = 0, one
    at Z < 0, a NaN Z, a NaN X, X = +Inf, Y = -Inf.  Exact like the others."""
    good = unproject([(1, 1, 2), (7, 1.5, 2), (1.5, 7, 4)], *EXACT_CAM)
    bad = []
    for k, (axis, val) in enumerate(((2, 0.0), (2, -1.0), (2, math.nan), (0, math.nan), (0, math.inf), (1, -math.inf))):
        t = unproject([(2, 2, 2), (6, 2, 2), (2, 6, 2)], *EXACT_CAM)
        t[k % 3, axis] = val
        bad.append(t)
    verts = torch.cat([good] + bad)
    return _scene(verts, torch.arange(verts.shape[0]).view(-1, 3), EXACT_CAM[0], EXACT_CAM[1], 8, 8)


# -- B. shapes
FACE_COUNTS = (0, 1, 31, 32, 33, 8191, 8192, 8193)
IMAGE_SIZES = ((1, 1), (1, 37), (37, 1), (15, 17), (16, 16), (17, 15), (63, 65), (64, 64), (65, 63), (130, 70))


@functools.lru_cache(maxsize=None)
def face_count_scene(F):
    """ISSUE B.1, 32 x 48: F - 1 small triangles, each around one pixel centre of columns 0 .. 39 with its edges at least
    0.1 px from every centre, in seven layers at depths [2 + l, 2.3 + l], dealt out in random order (so the index order
    is scrambled against position and depth); face F - 1 is one large triangle at depth ~3.6 whose hypotenuse crosses
    the image: the nearest wherever layers 0 and 1 have no triangle, the only cover in columns 40 .. 47.  One vertex set per
    face.  F = 0 keeps three vertices that nothing references."""
    H, W, cols = 32, 48, 40
    focal, princpt = (40.0, 44.0), (22.3, 17.6)

    def build(seed):
        g = torch.Generator().manual_seed(seed * 100003 + F)
        if F == 0:
            return _scene(torch.tensor([[0.0, 0.0, 2.0], [0.1, 0.0, 2.0], [0.0, 0.1, 2.0]]), torch.zeros((0, 3)), focal, princpt, H, W)
        n = F - 1
        slot = torch.randperm(7 * H * cols, generator=g)[:n]
        layer, i, j = slot // (H * cols), (slot % (H * cols)) // cols, slot % cols
        base = torch.tensor([[-0.3, -0.2], [0.3, -0.2], [0.0, 0.35]], dtype=torch.float64)
        uv = torch.stack((j + 0.5, i + 0.5), 1)[:, None, :] + base + (torch.rand(n, 3, 2, generator=g, dtype=torch.float64) - 0.5) * 0.1
        z = 2.0 + layer[:, None] + 0.3 * torch.rand(n, 3, generator=g, dtype=torch.float64)
        z[31::32] = 1.4 + (z[31::32] - z[31::32].floor())      # the last bit of every full mask word: in front of layer 0
        jit = torch.rand(3, generator=g, dtype=torch.float64)
        big = torch.tensor([[-20.0, -15.0, 3.6], [75.0 + jit[0], -15.0, 3.7], [-20.0, 50.0 + jit[1], 3.65]], dtype=torch.float64)
        uvz = torch.cat([torch.cat((uv, z[..., None]), -1).view(-1, 3), big])
        return _scene(unproject(uvz, focal, princpt), torch.arange(3 * F).view(F, 3), focal, princpt, H, W)
    return _first_clean(build, 0, block=8)


def _sphere_and_backdrop(g, H, W, focal, princpt, at=(0.15, 0.2)):
    """a perturbed level-1 icosphere (42 vertices, 80 faces) centred on screen (at[0] W, at[1] H) -- it hangs over the
    left and the top border -- and face 80: one triangle behind it that covers the whole image"""
    v, f = icosphere(1)
    s = max(min(H, W), 8)
    c = unproject([[at[0] * W, at[1] * H, 3.0]], focal, princpt)[0]
    R = 0.45 * s * 3.0 / focal[0]
    sph = v * R * (1 + 0.03 * torch.randn(v.shape[0], 1, generator=g, dtype=torch.float64)) + c
    j = torch.rand(6, generator=g, dtype=torch.float64)
    back = unproject([[-W - 5 - j[0], -H - 5 - j[1], 8.0], [3 * W + 5 + j[2], -H - 5 - j[3], 8.5], [-W - 5 - j[4], 3 * H + 5 + j[5], 7.5]],
                     focal, princpt)
    V0 = sph.shape[0]
    return torch.cat([sph, back]), torch.cat([f, torch.tensor([[V0, V0 + 1, V0 + 2]])])


@functools.lru_cache(maxsize=None)
def shape_scene(H, W):
    """ISSUE B.2: an off-centre principal point, the sphere over two borders, the backdrop face; with uvs and a 4 x 16 x 16
    texture for the render and its gradients."""
    s = float(max(min(H, W), 8))
    focal, princpt = (2.0 * s, 2.2 * s), (0.37 * W + 0.3, 0.61 * H - 0.2)

    def build(seed):
        g = torch.Generator().manual_seed(seed * 7919 + 131 * H + W)
        verts, faces = _sphere_and_backdrop(g, H, W, focal, princpt)
        return _with_uv(_scene(verts, faces, focal, princpt, H, W), seed)
    return _first_clean(build, amb_cap(H, W))


@functools.lru_cache(maxsize=None)
def batch_scene(tex_N=3):
    """ISSUE B.3: N = 3 meshes of one topology at 40 x 56, three focal / princpt pairs, ``tex_N`` = 3 or 1 textures."""
    H, W = 40, 56
    focal = ((70.0, 75.0), (90.0, 80.0), (60.0, 66.0))
    princpt = ((20.3, 25.1), (30.7, 15.2), (26.4, 21.9))
    at = ((0.15, 0.2), (0.3, 0.1), (0.05, 0.4))

    def build(seed):
        g = torch.Generator().manual_seed(seed * 31 + 5)
        parts = [_sphere_and_backdrop(g, H, W, focal[n], princpt[n], at[n]) for n in range(3)]
        sc = _scene(torch.stack([p[0] for p in parts]), parts[0][1], focal, princpt, H, W)
        return _with_uv(sc, seed, tex_N=tex_N)
    return _first_clean(build, amb_cap(H, W))


@functools.lru_cache(maxsize=None)
def offscreen_scene():
    """ISSUE B.4a, 24 x 32: face 0 is visible; faces 1 .. 4 lie wholly left of, right of, above and below the image, each
    within half a pixel of the border (so their bboxes still touch the border pixels); 5 .. 8 the same, 100 px away."""
    H, W = 24, 32
    focal, princpt = (30.0, 33.0), (15.2, 12.7)
    tri = [[(8.2, 5.1, 2.0), (25.3, 8.4, 3.0), (12.1, 20.2, 2.5)]]
    for d in (0.2, 100.0):
        tri += [[(-12, 5, 2), (-d, 9, 3), (-7, 17, 2.5)], [(W + d, 4, 2), (W + 14, 11, 2.2), (W + 6, 19, 3)],
                [(5, -9, 2), (20, -d, 2.1), (28, -11, 3)], [(4, H + d, 2), (17, H + 8, 2.4), (29, H + 3, 2.2)]]
    uvz = torch.tensor(tri, dtype=torch.float64).view(-1, 3)
    sc = _scene(unproject(uvz, focal, princpt), torch.arange(27).view(9, 3), focal, princpt, H, W)
    return _first_clean(lambda seed: sc, 0, seeds=1)


@functools.lru_cache(maxsize=None)
def far_corner_scene():
    """ISSUE B.4b, 24 x 32: face 0 has one corner 1e6 px to the right and still crosses the image as a thin wedge (its near
    corners are 50 px left of the image: the far corner's barycentric is then above EDGE_EPS at every pixel); face 1 is a
    backdrop."""
    H, W = 24, 32
    focal, princpt = (30.0, 33.0), (15.2, 12.7)

    def build(seed):
        g = torch.Generator().manual_seed(seed + 40)
        j = torch.rand(4, generator=g, dtype=torch.float64)
        uvz = [(-50.0, 8.8 + j[0], 2.0), (1e6, 11.5 + j[1], 4.0), (-50.0, 14.6 + j[2], 2.0),
               (-40.0, -30.0, 6.0), (90.0 + j[3], -30.0, 6.5), (-40.0, 80.0, 7.0)]
        return _scene(unproject(uvz, focal, princpt), [[0, 1, 2], [3, 4, 5]], focal, princpt, H, W)
    return _first_clean(build, 0)


@functools.lru_cache(maxsize=None)
def strip_scene():
    """ISSUE B.4c, 16 x 1100: one thin face near column 1050, 1033 px from the principal point, and one at the left end."""
    H, W = 16, 1100
    focal, princpt = (64.0, 64.0), (17.3, 8.4)

    def build(seed):
        g = torch.Generator().manual_seed(seed + 50)
        j = torch.rand(6, generator=g, dtype=torch.float64)
        uvz = [(1048.3 + j[0], 2.2, 2.0), (1051.9, 7.1 + j[1], 2.5), (1049.2 + j[2], 13.6, 3.0),
               (2.1 + j[3], 1.2, 2.0), (9.7, 3.3 + j[4], 2.2), (4.4 + j[5], 12.8, 2.1)]
        return _scene(unproject(uvz, focal, princpt), [[0, 1, 2], [3, 4, 5]], focal, princpt, H, W)
    return _first_clean(build, 0)


@functools.lru_cache(maxsize=None)
def depth_scene():
    """ISSUE B.5a, 40 x 48: 64 concentric triangles over the same pixels, the nearer the smaller (each shows in a ring about
    0.7 px wide), depths 0.25 apart, index order scrambled."""
    H, W = 40, 48
    focal, princpt = (50.0, 52.0), (25.7, 18.4)

    def build(seed):
        g = torch.Generator().manual_seed(seed + 60)
        perm = torch.randperm(64, generator=g)
        uvz = torch.zeros(64, 3, 3, dtype=torch.float64)
        for r in range(64):
            phi = torch.rand(1, generator=g, dtype=torch.float64) * 2 * math.pi
            rho = 2 * (3 + 0.66 * r)
            for k in range(3):
                a = phi + 2 * math.pi * k / 3
                uvz[perm[r], k] = torch.tensor([24.2 + rho * math.cos(a), 19.7 + rho * math.sin(a), 2 + 0.25 * r + 0.05 * k])
        return _scene(unproject(uvz.view(-1, 3), focal, princpt), torch.arange(192).view(64, 3), focal, princpt, H, W)
    return _first_clean(build, amb_cap(H, W))


@functools.lru_cache(maxsize=None)
def crossing_scene():
    """ISSUE B.5b, 40 x 48: two faces that both cover the image, one receding to the right and one to the left: the winner
    changes along a line, which ``z_amb`` marks where a pixel centre comes within 1e-6 (relative) of it."""
    H, W = 40, 48
    focal, princpt = (50.0, 52.0), (25.7, 18.4)

    def build(seed):
        g = torch.Generator().manual_seed(seed + 70)
        j = torch.rand(4, generator=g, dtype=torch.float64)
        uvz = [(-10.0, -10.0, 2.0), (110.0 + j[0], -10.0, 6.0), (-10.0, 100.0 + j[1], 2.0),
               (-10.5, -10.2, 5.0), (111.0 + j[2], -9.0, 1.5), (-9.0, 101.0 + j[3], 5.0)]
        return _scene(unproject(uvz, focal, princpt), [[0, 1, 2], [3, 4, 5]], focal, princpt, H, W)
    return _first_clean(build, amb_cap(H, W))


# -- C. sampler
# (u_a, u_b, v_a, v_b) of one quad in the SAMPLER's uv (v already flipped): all dyadic, so MeshRenderer's 1 - v is exact
UV_PATTERNS = ((-0.25, 1.25, -0.25, 1.25), (0, 1, 0, 1), (0, 0, -0.25, 1.25), (1, 1, -0.25, 1.25), (-0.25, 1.25, 0, 0),
               (-0.25, 1.25, 1, 1), (0.25, 0.25, 0, 1), (0.5, 0.5, 0.25, 0.75), (0, 1, 0.75, 0.75),
               # from here on the border clamp is active in both axes at every pixel (or the other axis is exactly 0)
               (-0.5, -0.125, -0.5, -0.125), (1.125, 1.5, -0.5, -0.125), (-0.5, -0.125, 1.125, 1.5), (1.125, 1.5, 1.125, 1.5),
               (-0.5, -0.125, 0, 0), (1.125, 1.5, 0, 0), (0, 0, 1.125, 1.5))
FIRST_CLAMPED_PATTERN = 9
SAMPLER_MAPS = ((1, 1), (1, 5), (5, 1), (2, 2), (16, 16))


@functools.lru_cache(maxsize=None)
def sampler_scene(C, tH, tW):
    """ISSUE C, 30 x 30: a 4 x 4 grid of quads (2 faces and 4 vertices of its own each, depths 2 .. 3), quad q textured with
    UV_PATTERNS[q]: uv beyond [0, 1] on each side, exactly 0 and 1, on the texel centres of a 5-wide map, and quads
    where the clamp is active everywhere.  Quad q owns vertices 4 q .. 4 q + 3 and faces 2 q, 2 q + 1."""
    H = W = 30
    focal, princpt = (40.0, 42.0), (13.7, 16.2)
    g = torch.Generator().manual_seed(90)
    uvz, uvs, faces = [], [], []
    for q, (ua, ub, va, vb) in enumerate(UV_PATTERNS):
        x0, y0 = 1.3 + 7 * (q % 4), 1.45 + 7 * (q // 4)
        z = 2 + torch.rand(4, generator=g, dtype=torch.float64)
        uvz += [(x0, y0, z[0]), (x0 + 6.1, y0, z[1]), (x0 + 6.1, y0 + 6.1, z[2]), (x0, y0 + 6.1, z[3])]
        uvs += [(ua, 1 - va), (ub, 1 - va), (ub, 1 - vb), (ua, 1 - vb)]           # vertex_uv: v before MeshRenderer's flip
        faces += [(4 * q, 4 * q + 1, 4 * q + 2), (4 * q, 4 * q + 2, 4 * q + 3)]
    sc = _scene(unproject(uvz, focal, princpt), faces, focal, princpt, H, W)
    sc = dict(sc, texture=smooth_texture(1, C, tH, tW, seed=C).float(), vertex_uv=torch.tensor(uvs, dtype=torch.float32),
              face_uv=sc['faces'].clone())
    return _first_clean(lambda seed: sc, 0, seeds=1)


# -- D. a long CSR list
@functools.lru_cache(maxsize=None)
def fan_scene():
    """ISSUE D.2, 64 x 64: 2048 faces around vertex 3 -- sixteen turns of 128 faces, turn t reaching 6 + 1.5 t px from the
    centre and receding faster than turn t - 1, so every turn shows in a ring of its own -- in scrambled index order;
    vertices 0, 1, 2 and the last two are referenced by no face."""
    H = W = 64
    focal, princpt = (60.0, 60.0), (30.1, 33.4)

    def build(seed):
        g = torch.Generator().manual_seed(seed + 80)
        cx, cy, zc = 32.3, 31.6, 2.0
        uvz, faces = [(5.0, 5.0, 2.0)] * 3 + [(cx, cy, zc)], []
        for t in range(16):
            R = 6 + 1.5 * t
            zt = 1.0 / (1.0 / zc - (0.004 + 0.0004 * t) * R)
            first = len(uvz)
            for k in range(128):
                a = 2 * math.pi * (k + 0.37 * t + 0.4 * (float(torch.rand(1, generator=g)) - 0.5)) / 128
                r = R + 0.4 * (float(torch.rand(1, generator=g)) - 0.5)
                uvz.append((cx + r * math.cos(a), cy + r * math.sin(a), zt))
            faces += [(3, first + k, first + (k + 1) % 128) for k in range(128)]
        uvz += [(50.0, 50.0, 2.0)] * 2
        faces = torch.tensor(faces)[torch.randperm(2048, generator=g)]
        return _with_uv(_scene(unproject(uvz, focal, princpt), faces, focal, princpt, H, W), seed)
    return _first_clean(build, amb_cap(H, W))


FAN_CENTRE, FAN_UNREFERENCED = 3, (0, 1, 2, 2052, 2053)
