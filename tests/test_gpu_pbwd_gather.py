"""The gather of the per-Gaussian backward (csrc/preprocess_bwd.hip, `stream_gather`) at its corners: small scenes on a
128 x 128 image, through the public renderer in exact mode, gradients against the CPU oracle with the bars of
tests/helpers.py.  Every case asserts from the READ-BACK splat records (row 3: instance count and first slot) that its corner
really occurred: a wave's stream is the concatenation of the instances of its 64 Gaussians (those with a radius and fewer
than COOP_MIN = 64 instances), staged GCH = 256 slots at a time, the first GCAP = 512 with one request for all their flags.

The backward of an OVERFLOWED forward goes through ``StaticRender(on_overflow='raise')``, the one surface that queues a
backward behind such a forward (the autograd surfaces raise from the forward call)."""
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import rasterizer as rz
from exavatar_release_amd import scenes, stats
from exavatar_release_amd.camera import make_raster_matrices
from oracle import raster_oracle as ro
from tests.helpers import assert_grads_close, gaussians_near_pixels, rotation_grad_scale

pytestmark = pytest.mark.gpu

KEYS = ('mean_3d', 'scale', 'rotation', 'opacity', 'rgb')
H = W = 128
F = 128.0
GCH, GCAP, COOP_MIN = 256, 512, 64


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from exavatar_release_amd import _lib
    _lib.load()
    old = (exa.config.mode, exa.config.fixed_capacity, exa.config.keep_debug)
    exa.config.mode, exa.config.fixed_capacity, exa.config.keep_debug = 'exact', None, True
    yield torch.device('cuda:0')
    exa.config.mode, exa.config.fixed_capacity, exa.config.keep_debug = old
    rz._debug_last.clear()


def _splats(n, seed, px_sigma=(0.6, 4.5), box=(10.0, 118.0), z=(2.5, 3.5), opacity=(0.2, 0.7)):
    """n isotropic-ish Gaussians with centres inside the image and a projected sigma of px_sigma pixels."""
    g = torch.Generator().manual_seed(seed)
    r = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g)      # noqa: E731
    zz = r(z[0], z[1], n)
    u, v = r(box[0], box[1], n), r(box[0], box[1], n)
    sig = r(px_sigma[0], px_sigma[1], n)
    q = torch.randn(n, 4, generator=g)
    return {'mean_3d': torch.stack(((u - W / 2) / F * zz, (v - H / 2) / F * zz, zz), 1),
            'scale': (sig * zz / F)[:, None] * r(0.8, 1.25, n, 3),
            'rotation': q / q.norm(dim=1, keepdim=True),
            'opacity': r(opacity[0], opacity[1], n, 1), 'rgb': r(0.0, 1.0, n, 3)}


def _take(a, idx):
    return {k: v[idx].clone() for k, v in a.items()}


def _cat(*parts):
    return {k: torch.cat([p[k] for p in parts]) for k in KEYS}


def _records(P):
    """(instances, first slot, radius) of the most recent forward's P Gaussians, from its splat records."""
    rec = rz._debug_last['geom'][: P * 64].view(torch.int32).view(P, 16).cpu().to(torch.int64)
    return rec[:, 14], rec[:, 15], rec[:, 3]


def _touched():
    cap = int(rz._debug_last['capacity'])
    o, n = stats.bin_offsets(cap)['touched']
    return rz._debug_last['bin'][o:o + n].cpu()


def _stream(n, radius, w):
    """Length of the gather stream of wave w."""
    m = torch.where((radius > 0) & (n < COOP_MIN), n, torch.zeros_like(n))
    return int(m[64 * w:64 * w + 64].sum())


def _check(dev, a, seed=0):
    """Render + backward on the GPU and on the oracle, gradients within the bars; returns the read-back records (instances,
    first slot, radius), the `touched` bytes and the GPU leaves with their gradients."""
    P = a['mean_3d'].shape[0]
    cam = scenes.neutral_camera(H, W, focal=F)
    g = torch.Generator().manual_seed(100 + seed)
    G, bg = torch.randn(3, H, W, generator=g), torch.rand(3, generator=g)
    ag = {k: v.to(dev).requires_grad_(True) for k, v in a.items()}
    out = exa.GaussianRenderer()(ag, (H, W), {k: v.to(dev) for k, v in cam.items()}, bg.to(dev))
    recs = _records(P)
    (out['img'] * G.to(dev)).sum().backward()
    tch = _touched()                                 # (the flags are the backward blend's: read behind it)
    ac = {k: v.clone().requires_grad_(True) for k, v in a.items()}
    ref = ro.render(ac, (H, W), cam, bg, return_aux=True)
    (ref['img'] * G).sum().backward()
    assert torch.equal(out['radius'].cpu(), ref['radius']), 'radii differ'
    near = gaussians_near_pixels(ref['aux']['pre'], ro.ambiguous_pixel_mask(ref['aux'], H, W))
    for k in KEYS:
        assert_grads_close(ag[k].grad, ac[k].grad, k, near,
                           abs_scale=rotation_grad_scale(ac['scale'], ac['scale'].grad) if k == 'rotation' else 0.0)
    assert_grads_close(out['mean_2d'].grad, ref['mean_2d'].grad, 'mean_2d', near)
    return recs + (tch, ag)


_POOL = {}


def _pool(dev):
    """600 candidate splats and their instance counts (a splat's count depends on the splat alone), rendered once."""
    if not _POOL:
        a = _splats(600, seed=1)
        cam = scenes.neutral_camera(H, W, focal=F)
        with torch.no_grad():
            exa.GaussianRenderer()({k: v.to(dev) for k, v in a.items()}, (H, W), {k: v.to(dev) for k, v in cam.items()},
                                   torch.zeros(3, device=dev))
        n, _, rad = _records(600)
        assert bool((rad > 0).all()) and int(n.min()) >= 1 and int(n.max()) < COOP_MIN
        _POOL['a'], _POOL['n'] = a, n
    return _POOL['a'], _POOL['n']


def _wave_of(dev, target, seed):
    """Indices of 64 pool splats whose instance counts add up to exactly `target`: a subset sum over (picked, instances)
    on the pool in a seeded order, walked back from (64, target)."""
    _, n = _pool(dev)
    order = torch.randperm(600, generator=torch.Generator().manual_seed(seed)).tolist()
    reach = torch.zeros(65, target + 1, dtype=torch.bool)
    reach[0, 0] = True
    before = []
    for i in order:
        c = int(n[i])
        before.append(reach)
        nxt = reach.clone()
        if c <= target:
            nxt[1:, c:] |= reach[:-1, :target + 1 - c]
        reach = nxt
    assert bool(reach[64, target]), 'no 64 splats of the pool add up to %d instances' % target
    k, t, pick = 64, target, []
    for i, b in zip(reversed(order), reversed(before)):
        if not bool(b[k, t]):                        # not reachable without splat i: it is part of the sum
            pick.append(i)
            k, t = k - 1, t - int(n[i])
    assert k == 0 and t == 0 and len(pick) == 64
    return torch.tensor(pick)


@pytest.mark.parametrize('target', [GCH, GCH + 1, 2 * GCH + 8, 3 * GCH + 40])
def test_stream_lengths_around_the_chunk_and_the_cap(dev, target):
    """Wave 0's stream is exactly one chunk, one chunk and a slot, just over two chunks (= just over the cap: the per-chunk
    requests take over for the third) and over three chunks; 100 more splats behind it leave a partly filled last wave."""
    pool, _ = _pool(dev)
    a = _cat(_take(pool, _wave_of(dev, target, seed=target)), _splats(100, seed=2))
    n, off, rad, _, _ = _check(dev, a, seed=target)
    assert _stream(n, rad, 0) == target and bool((rad[:64] > 0).all()) and int(n[:64].max()) < COOP_MIN
    assert a['mean_3d'].shape[0] % 64 != 0 and _stream(n, rad, 2) > 0


def test_lanes_without_instances_and_a_wave_of_them(dev):
    """Wave 0: every second Gaussian off screen or behind the camera; wave 1: only such Gaussians; wave 2: visible ones."""
    a = _splats(64 * 2 + 50, seed=3)
    gone = torch.cat((torch.arange(1, 64, 2), torch.arange(64, 128)))
    a['mean_3d'][gone[0::2], 0] = 40.0               # far off screen
    a['mean_3d'][gone[1::2], 2] = -1.0               # behind the camera
    n, off, rad, _, _ = _check(dev, a, seed=3)
    assert bool((rad[gone] == 0).all()) and bool((rad[0:64:2] > 0).all())
    assert _stream(n, rad, 0) > 0 and _stream(n, rad, 1) == 0 and _stream(n, rad, 2) > 0


@pytest.mark.parametrize('P', [37, 64 + 1, 3 * 64 + 63])
def test_partly_filled_last_wave(dev, P):
    n, off, rad, _, _ = _check(dev, _splats(P, seed=4 + P), seed=P)
    assert P % 64 != 0 and _stream(n, rad, (P - 1) // 64) > 0 and int(rad[P - 1]) > 0


def test_heavy_splat_among_small_ones(dev):
    """One splat of >= COOP_MIN instances (its own whole-wave path) in the middle of a wave of small ones."""
    a = _splats(100, seed=5, px_sigma=(0.6, 2.5))
    a['scale'][10] = torch.tensor([0.45, 0.40, 0.35])
    a['mean_3d'][10] = torch.tensor([0.05, -0.03, 3.0])
    a['opacity'][10] = 0.35
    n, off, rad, _, _ = _check(dev, a, seed=5)
    assert int(n[10]) >= COOP_MIN and int(torch.cat((n[:10], n[11:64])).max()) < COOP_MIN and _stream(n, rad, 0) > 0


def test_hidden_splats_have_instances_but_no_flag(dev):
    """Unflagged slots inside a stream: four opaque sheets at z = 1 (alpha is capped at 0.99: T < 1e-4 behind the second) cover
    40 small splats at z >= 3; 60 more splats lie in front of the sheets and are blended.  The covered splats have instances; the
    case asserts from the read-back flags that unflagged slots of theirs AND flagged slots of the front splats occur in the same
    waves, that at least one covered splat has no flagged slot at all, and that every such splat's gradients are exact zeros
    (an unflagged slot adds +0).  (Not every covered splat is flag-free in this scene: the flags are what the backward blend
    left, and the gradients of all 104 splats are held against the oracle like everywhere else.)"""
    front = _splats(4, seed=6)
    front['mean_3d'] = torch.tensor([[0.0, 0.0, 1.0 + 0.01 * i] for i in range(4)])
    front['scale'] = torch.full((4, 3), 2.0)         # (sigma 256 px: alpha = 0.99 over the whole box of the covered ones)
    front['opacity'] = torch.ones(4, 1)
    hidden = _splats(40, seed=7, px_sigma=(0.8, 2.0), box=(48.0, 80.0), z=(3.0, 3.5))
    a = _cat(_splats(30, seed=8, z=(0.5, 0.8)), hidden, front, _splats(30, seed=9, z=(0.5, 0.8)))
    n, off, rad, tch, ag = _check(dev, a, seed=6)
    h = list(range(30, 70))
    flagged = lambda i: int((tch[int(off[i]):int(off[i] + n[i])] != 0).sum())      # noqa: E731
    assert bool((rad[h] > 0).all()) and bool((n[h] > 0).all()) and int(n[h].max()) < COOP_MIN
    assert sum(int(n[i]) - flagged(i) for i in h) > 0, 'no unflagged slot among the covered splats'
    assert sum(flagged(i) for i in range(30)) > 0, 'no flagged slot among the front splats'
    clean = [i for i in h if flagged(i) == 0]
    assert clean, 'no covered splat without a flagged slot'
    idx = torch.tensor(clean, device=dev)
    assert all(bool((ag[k].grad[idx] == 0).all()) for k in KEYS), 'a splat without a flagged slot has a gradient'


def test_constant_prefix_ending_inside_a_wave(dev):
    """grad_first = 37: Gaussians 0 .. 36 of wave 0 are constants of the gather's wave, 37 .. are trained."""
    nS = 37
    scene, human = _splats(nS, seed=10), _splats(120, seed=11)
    cam = scenes.neutral_camera(H, W, focal=F)
    cam_d = {k: t.to(dev) for k, t in cam.items()}
    g = torch.Generator().manual_seed(12)
    G, bg = torch.randn(3, H, W, generator=g), torch.rand(3, generator=g)
    s1 = {k: v.to(dev).requires_grad_(True) for k, v in scene.items()}
    h1 = {k: v.to(dev).requires_grad_(True) for k, v in human.items()}
    o1 = exa.render_many(exa.GaussianRenderer(), [(h1, (H, W), cam_d, bg.to(dev), None, s1)])[0]
    (o1['img'] * G.to(dev)).sum().backward()
    rad = o1['radius'].cpu()
    # the instance counts: a splat's count depends on the splat alone, so they are read back from a plain render of the
    # concatenation (same radii as the prefix render's) -- both sides of the boundary inside wave 0 have instances
    with torch.no_grad():
        exa.GaussianRenderer()({k: torch.cat((scene[k], human[k])).to(dev) for k in KEYS}, (H, W), cam_d, bg.to(dev))
    n, _, rad_rec = _records(nS + 120)
    assert torch.equal(rad_rec, rad.to(torch.int64)) and rad.shape[0] == nS + 120 and nS % 64 != 0
    assert int(n[:nS].min()) > 0 and int(n[nS:64].min()) > 0 and int(n[:64].max()) < COOP_MIN
    assert all(s1[k].grad is None for k in KEYS)
    h3 = {k: v.clone().requires_grad_(True) for k, v in human.items()}
    ref = ro.render({k: torch.cat((scene[k], h3[k])) for k in KEYS}, (H, W), cam, bg, return_aux=True)
    (ref['img'] * G).sum().backward()
    near = gaussians_near_pixels(ref['aux']['pre'], ro.ambiguous_pixel_mask(ref['aux'], H, W))[nS:]
    for k in KEYS:
        assert_grads_close(h1[k].grad, h3[k].grad, k, near,
                           abs_scale=rotation_grad_scale(h3['scale'], h3['scale'].grad) if k == 'rotation' else 0.0)
    assert_grads_close(o1['mean_2d'].grad, ref['mean_2d'].grad[nS:], 'mean_2d', near)


@pytest.mark.parametrize('K', [2, 5])
def test_summed_views_equal_the_single_view_calls(dev, K):
    """K views of the same Gaussians in one batch (K = 5: a second row of workgroups and the group scratch): every view's
    image and mean_2d gradient bit for bit what the single call gives, the summed gradients equal to the sum of the single
    calls' up to the order of the K additions (2e-6 of the tensor's magnitude, the bar of
    tests/test_gpu_parity.py::test_batched_views_equal_single_renders_and_sum_gradients)."""
    pool, _ = _pool(dev)
    a = _cat(_take(pool, _wave_of(dev, 2 * GCH + 8, seed=77)), _splats(100, seed=13))
    cams = [scenes.ring_camera(H, W, v, 40, radius=3.0, center=(0.0, 0.0, 3.0), focal=F) for v in range(K)]
    to_dev = lambda c: {k: v.to(dev) for k, v in c.items()}      # noqa: E731
    g = torch.Generator().manual_seed(14)
    Gs = [torch.randn(3, H, W, generator=g).to(dev) for _ in range(K)]
    bg = torch.rand(3, generator=g).to(dev)
    rend = exa.GaussianRenderer()
    a_seq = {k: v.to(dev).requires_grad_(True) for k, v in a.items()}
    outs_seq = []
    streams = []
    for c in cams:
        outs_seq.append(rend(a_seq, (H, W), to_dev(c), bg))
        n, _, rad = _records(164)
        streams.append(_stream(n, rad, 0))
    assert max(streams) > GCH, streams                  # (more than one chunk in at least one of the views)
    sum((o['img'] * G).sum() for o, G in zip(outs_seq, Gs)).backward()
    a_bat = {k: v.to(dev).requires_grad_(True) for k, v in a.items()}
    outs_bat = exa.render_views(rend, a_bat, (H, W), [to_dev(c) for c in cams], bg)
    sum((o['img'] * G).sum() for o, G in zip(outs_bat, Gs)).backward()
    for ob, os_ in zip(outs_bat, outs_seq):
        assert torch.equal(ob['img'], os_['img']) and torch.equal(ob['radius'], os_['radius'])
        assert torch.equal(ob['mean_2d'].grad, os_['mean_2d'].grad)
    for k in KEYS:
        gb, gs = a_bat[k].grad, a_seq[k].grad
        mag = float(gs.abs().max()) if k != 'rotation' else rotation_grad_scale(a_seq['scale'], a_seq['scale'].grad)
        assert float((gb - gs).abs().max()) <= 2e-6 * mag, k


def test_sh_degree_3(dev):
    """The SH instantiation of the kernel over a two-chunk wave."""
    pool, _ = _pool(dev)
    a = _cat(_take(pool, _wave_of(dev, GCH + 1, seed=5)), _splats(70, seed=15))
    P = 134
    sh = scenes.sh_from_rgb(a['rgb'], 3, seed=3, rest_sigma=0.3)
    cam = scenes.neutral_camera(H, W, focal=F)
    g = torch.Generator().manual_seed(16)
    G, bg = torch.randn(3, H, W, generator=g), torch.rand(3, generator=g)
    tanx, tany, view, proj, campos = make_raster_matrices(cam, (H, W))
    st = exa.GaussianRasterizationSettings(H, W, tanx, tany, bg.to(dev), 1.0, view.to(dev), proj.to(dev), 3, campos.to(dev),
                                           False, False)
    ag = {k: a[k].to(dev).requires_grad_(True) for k in ('mean_3d', 'scale', 'rotation', 'opacity')}
    shg = sh.to(dev).requires_grad_(True)
    m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
    col = exa.GaussianRasterizer(st)(means3D=ag['mean_3d'], means2D=m2, opacities=ag['opacity'], shs=shg,
                                     scales=ag['scale'], rotations=ag['rotation'])[0]
    n, _, rad = _records(P)
    assert _stream(n, rad, 0) == GCH + 1
    (col * G.to(dev)).sum().backward()
    ac = {k: a[k].clone().requires_grad_(True) for k in ('mean_3d', 'scale', 'rotation', 'opacity')}
    shc = sh.clone().requires_grad_(True)
    ref = ro.rasterize(ac['mean_3d'], torch.zeros(P, 3), ac['opacity'], shs=shc, scales=ac['scale'],
                       rotations=ac['rotation'], settings=ro.settings_from_camera(cam, (H, W), bg, 3), return_aux=True)
    (ref[0] * G).sum().backward()
    assert_grads_close(shg.grad, shc.grad, 'shs')
    for k in ac:
        assert_grads_close(ag[k].grad, ac[k].grad, k)


def test_backward_of_an_overflowed_forward_writes_zeros(dev):
    """A buffer a quarter of what the render needs, ``on_overflow='raise'``: the forward polls nothing, the backward is
    queued behind it, ``check()`` raises -- the header says overflow, and every gradient array, filled with 7 before, holds
    exact zeros (the overflowed forward left no lists behind).  The same object with enough room then gives gradients."""
    a = {k: v.to(dev).contiguous() for k, v in _cat(_splats(200, seed=17)).items()}
    P = 200
    cam = scenes.neutral_camera(H, W, focal=F)
    tanx, tany, view, proj, campos = make_raster_matrices(cam, (H, W))
    st = exa.GaussianRasterizationSettings(H, W, tanx, tany, torch.zeros(3, device=dev), 1.0, view.to(dev).contiguous(),
                                           proj.to(dev).contiguous(), 0, campos.to(dev).contiguous(), False, False)
    G = torch.randn(3, H, W, generator=torch.Generator().manual_seed(18)).to(dev)
    need = exa.required_capacity(a['mean_3d'], a['opacity'], a['scale'], a['rotation'], colors_precomp=a['rgb'], settings=st)
    assert need > 4 * 64
    shapes = {'means3D': (P, 3), 'means2D': (P, 3), 'opacities': (P, 1), 'scales': (P, 3), 'rotations': (P, 4),
              'colors_precomp': (P, 3)}
    for cap, overflow in ((need // 4, True), (need, False)):
        with exa.StaticRender(a['mean_3d'], a['opacity'], a['scale'], a['rotation'], colors_precomp=a['rgb'], image_size=(H, W),
                              capacity=cap, train=True, on_overflow='raise') as sr:
            v = sr.add_view(st, dL_dcolor=G)
            out = sr.add_grad_outputs(**{k: torch.full(sh, 7.0, device=dev) for k, sh in shapes.items()})
            sr.forward(v)
            sr.backward(out)
            if overflow:
                with pytest.raises(RuntimeError, match='needed %d instances' % need):
                    sr.check()
            else:
                sr.check()
            hdr = rz.read_header(sr._slots[0].tile)
            assert bool(hdr[1]) == overflow                      # (the header's overflow word, as the kernel reads it)
            assert bool((sr.radii > 0).any())                    # (the radii are written before the overflow is known)
            got = sr.grad_outputs(out)
            if overflow:
                assert all(bool((got[k] == 0).all()) for k in shapes), 'gradients of an overflowed render'
            else:
                assert all(bool((got[k] != 7.0).all()) for k in shapes)
                assert float(got['means3D'].abs().max()) > 0
