"""The HIP backward against the HIP forward's OWN discrete decisions, on every pixel.

The backward replays the forward's decisions (skip alpha < 1/255, skip power > 0, stop when T (1 - alpha) < 1e-4) over a
compacted list and builds R from the forward's checkpointed C_fin / T_final (csrc/blend.h, csrc/render_bwd.hip): a replay
that disagrees with its forward anywhere gives a wrong gradient.  The other parity tests compare against oracles that
take their own decisions and therefore mask the pixels near a threshold.  Here the decisions are READ OFF the HIP forward
(tests/helpers.py extract_weights: w [P, H, W] from one-hot colour probes, keep = w > 0) and handed to the float64
decision oracle (tests/decision_oracle.py).  Images, depth, mask and every weight are held to IMG_TOL on every pixel and
all six gradients to GRAD_REL_TOL without any ambiguity mask.

Cases: the seeded edge-case fuzz; needles (the groups of four that keep the "power > 0" guard) with dead entries and safe
correlated splats at opacity 0.5 / 0.25 a few 1e-4 px off pixel centres between them; a ladder of opacities around 1/255
on pixel centres; stacks that stop pixels at every position of a group of four and at list entries 63 / 64 / 65; lists
longer than three 64-entry batches; the in-kernel SH colour; batches of 8 jobs (heterogeneous, and shared tensors)."""
import os

import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import scenes
from exavatar_release_amd.rasterizer import rasterize_gaussians_batch
from exavatar_release_amd.renderer import _raster_job
from oracle import raster_oracle as ro
from tests import decision_oracle as do
from tests.decision_oracle import KEYS
from tests.helpers import (IMG_TOL, assert_grads_close, extract_weights, fuzz_case, record_stats, rotation_grad_scale)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from exavatar_release_amd import _lib
    _lib.load()
    exa.config.mode = 'exact'
    exa.config.fixed_capacity = None
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return torch.device('cuda:0')


def _cam(cam, dev):
    return {k: v.to(dev) for k, v in cam.items()}


def hip_weights(dev, a, H, W, cam, perm=None):
    """(w [P, H, W], mask [H, W]) of the HIP forward of ``a`` (rgb probes, background 0, no autograd)."""
    geo = {k: a[k].to(dev) for k in ('mean_3d', 'scale', 'rotation', 'opacity')}
    camd, zero = _cam(cam, dev), torch.zeros(3, device=dev)
    masks = []

    def render_rgb(rgb):
        with torch.no_grad():
            out = exa.GaussianRenderer()({**geo, 'rgb': rgb.to(dev)}, (H, W), camd, zero)
        masks.append(out['mask'][0].cpu())
        return out['img']
    w = extract_weights(render_rgb, a['mean_3d'].shape[0], perm)
    assert all(torch.equal(m, masks[0]) for m in masks), 'the probes changed the mask: colour entered a decision'
    return w, masks[0]


def decisions(dev, a, H, W, cam):
    """keep [P, H, W] of the HIP forward, with the probe's own checks: the weights add up to the mask, and another
    grouping of the probes reads the same decisions."""
    P = a['mean_3d'].shape[0]
    w, mask = hip_weights(dev, a, H, W, cam)
    assert float((w.sum(0) - mask.double()).abs().max()) <= 1e-6, 'sum of the weights != mask'
    w2, _ = hip_weights(dev, a, H, W, cam, torch.randperm(P, generator=torch.Generator().manual_seed(P + H)))
    assert torch.equal(w2 > 0, w > 0), 'another probe grouping read other decisions'
    return w, mask


def _loss(o, G, Gd, Ga):
    return (o['img'] * G).sum() + (o['depthmap'] * Gd).sum() + (o['mask'] * Ga).sum()


def _assert_planes(tag, got, ref, w_hip=None, pix=None):
    """Image, depth, mask (and every weight) at IMG_TOL on every pixel, or on the pixels of ``pix`` [H, W]."""
    st = {}
    for k in ('img', 'depthmap', 'mask'):
        d = (got[k].detach().cpu().double() - ref[k].detach()).abs().amax(0)
        d = float(d.max() if pix is None else d[pix].max())
        st[k] = d
        assert d <= IMG_TOL, '%s: %s off by %.3e' % (tag, k, d)
    if w_hip is not None:
        d = (w_hip - ref['w']).abs()
        d = float(d.max() if pix is None else d[:, pix].max())
        st['w'] = d
        assert d <= IMG_TOL, '%s: a blend weight off by %.3e' % (tag, d)
    return st


def _assert_grads(tag, got, ref, st):
    """got / ref: dicts of gradients (KEYS or the SH keys, plus 'mean_2d'); rotation with its natural magnitude."""
    for k in got:
        abs_scale = rotation_grad_scale(ref['_scale'], ref['scale']) if k == 'rotation' else 0.0
        st['grad_' + k] = assert_grads_close(got[k], ref[k], '%s %s' % (tag, k), abs_scale=abs_scale)['max_rel']


def check_case(dev, tag, a, H, W, cam, bg, G, Gd, Ga, w=None, exclude=None):
    """HIP render + backward against the decision oracle with the HIP forward's decisions.  Returns (stats, w).
    ``exclude`` (bool [P]): Gaussians whose pixels are left out -- the pixels where one of them has a weight get a zero
    loss gradient and are not compared; every gradient is still checked."""
    if w is None:
        w, _ = decisions(dev, a, H, W, cam)
    pix = None
    if exclude is not None:
        pix = ~(w[exclude] > 0).any(0)
        G, Gd, Ga = G * pix, Gd * pix, Ga * pix
    ag = {k: v.to(dev).requires_grad_(True) for k, v in a.items()}
    out = exa.GaussianRenderer()(ag, (H, W), _cam(cam, dev), bg.to(dev))
    _loss(out, G.to(dev), Gd.to(dev), Ga.to(dev)).backward()
    vis = out['radius'].cpu() > 0
    t = {k: v.clone().double().requires_grad_(True) for k, v in a.items()}
    ref = do.render(t, (H, W), cam, bg, w > 0, vis)
    _loss(ref, G.double(), Gd.double(), Ga.double()).backward()
    st = {'H': H, 'W': W, 'P': int(a['mean_3d'].shape[0]), 'pairs': int((w > 0).sum())}
    if pix is not None:
        st['pixels_left_out'] = int((~pix).sum())
    st.update(_assert_planes(tag, out, ref, w, pix))
    got = {k: ag[k].grad for k in KEYS}
    got['mean_2d'] = out['mean_2d'].grad
    want = {k: t[k].grad for k in KEYS}
    want['mean_2d'] = ref['mean_2d'].grad
    want['_scale'] = t['scale'].detach()
    _assert_grads(tag, got, want, st)
    return st, w


def _grads_of(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(3, H, W, generator=g), torch.randn(1, H, W, generator=g), torch.randn(1, H, W, generator=g)


# ---- scene construction -----------------------------------------------------------------------------------------
def place(a, idx, tx, ty, cam, H, W):
    """Move Gaussians ``idx`` (keeping their depth) so that their float32 pixel centres -- what the HIP preprocess
    computes, bit for bit (raster_oracle.preprocess in float32) -- are as close as float32 allows to (tx, ty)."""
    f = float(cam['focal'][0])
    z = a['mean_3d'][idx, 2].double()
    x0 = ((tx.double() - W / 2.0 + 0.5) / f * z).float()
    y0 = ((ty.double() - H / 2.0 + 0.5) / f * z).float()
    steps = torch.arange(-96, 97, dtype=torch.int32)
    n, m = idx.numel(), steps.numel()
    xs = (x0.view(torch.int32)[:, None] + steps[None]).view(torch.float32)        # float32 neighbours (same sign)
    ys = (y0.view(torch.int32)[:, None] + steps[None]).view(torch.float32)
    mu = torch.stack((xs.reshape(-1), ys.reshape(-1), z.float()[:, None].expand(n, m).reshape(-1)), 1)
    s = ro.settings_from_camera(cam, (H, W), torch.zeros(3))
    with torch.no_grad():
        pre = ro.preprocess(mu, None, None, torch.full((n * m, 3), 0.01), torch.tensor([[1.0, 0, 0, 0]]).expand(n * m, 4),
                            None, s, torch.float32)
    ex = (pre['px'].double().view(n, m) - tx.double()[:, None]).abs().argmin(1)
    ey = (pre['py'].double().view(n, m) - ty.double()[:, None]).abs().argmin(1)
    a['mean_3d'][idx, 0] = xs[torch.arange(n), ex]
    a['mean_3d'][idx, 1] = ys[torch.arange(n), ey]


def _needles(a, idx, depths, g):
    """Needles of tests/helpers.py needle_scene (conics that blend.h conic_safe calls unsafe) at the given depths."""
    for i, d, s in zip(idx, depths, (12.0, 30.0, 100.0, 40.0)):
        a['scale'][i] = torch.tensor([s, 1e-4, 1e-4])
        a['mean_3d'][i] = torch.tensor([0.1 * (i % 4) - 0.2, 0.05 * (i % 4) - 0.1, 0.0]) * d / 3.0 + torch.tensor([0, 0, d])
        q = torch.randn(4, generator=g)
        a['rotation'][i] = q / q.norm()
        a['opacity'][i] = 0.6


def guard_scene():
    """Four needles at depths 2.2 .. 4.0; 96 dead entries (opacity 1/300: they cover sub-tiles and never reach 1/255, so
    the backward's compacted list drops them and regroups what follows); and, interleaved in depth, 192 safe splats
    correlated along x = y (minor axis at the 0.3 px^2 floor, major sigma 2 .. 5 px) at opacity exactly 0.5 and 0.25,
    each centred on a pixel centre plus an offset (dx, dy), 0.5e-4 <= |dx|, |dy| <= 3e-4 px, with dx dy > 0.  There the
    quadratic form is a few 1e-8 while lop = log2(opacity) sits at a binade boundary: fp32 rounding can put p2 one ulp
    above lop, which the "power > 0" guard then skips -- at the splat's own centre pixel, where its weight is largest.
    Returns (assets, H, W, cam, S = indices of the safe splats, their centre pixels [192, 2] as (x, y))."""
    H, W, f = 48, 64, 100.0
    cam = scenes.neutral_camera(H, W, focal=f)
    g = torch.Generator().manual_seed(2024)
    nN, nD, nS = 4, 96, 192
    P = nN + nD + nS
    a = scenes.dist_a_random(P, H, W, seed=17, focal=f, z_range=(2.0, 4.2))
    _needles(a, range(nN), (2.2, 2.8, 3.4, 4.0), g)
    D = torch.arange(nN, nN + nD)
    a['opacity'][D] = 1.0 / 300.0
    a['scale'][D] = (4.0 + 4.0 * torch.rand(nD, 1, generator=g)) * a['mean_3d'][D, 2:3] / f
    S = torch.arange(nN + nD, P)
    gx, gy = torch.meshgrid(torch.arange(2, W, 4), torch.arange(2, H, 4), indexing='xy')
    offs = torch.tensor([0.5e-4, 1e-4, 1.5e-4, 2e-4, 2.5e-4, 3e-4])
    k = torch.arange(nS)
    sign = torch.where(k % 2 == 0, 1.0, -1.0)
    ox, oy = sign * offs[k % 6], sign * offs[(k // 6) % 6]
    major = torch.tensor([2.0, 3.0, 5.0])[(k // 36) % 3]
    z = a['mean_3d'][S, 2]
    a['scale'][S] = torch.stack((major * z / f, torch.full_like(z, 1e-4), torch.full_like(z, 1e-4)), 1)
    c, s_ = torch.cos(torch.tensor(torch.pi / 8)), torch.sin(torch.tensor(torch.pi / 8))     # +45 deg about the view axis
    a['rotation'][S] = torch.tensor([float(c), 0.0, 0.0, float(s_)])
    a['opacity'][S] = torch.where(k % 4 < 2, 0.5, 0.25).view(-1, 1)
    place(a, S, gx.reshape(-1)[:nS].float() + ox, gy.reshape(-1)[:nS].float() + oy, cam, H, W)
    centres = torch.stack((gx.reshape(-1)[:nS], gy.reshape(-1)[:nS]), 1)
    return a, H, W, cam, S, centres


def bar_opacities(n):
    """float32 opacities 1/255 - 6 ulp, ..., 1/255 + (n - 7) ulp."""
    base = torch.tensor([1.0 / 255.0], dtype=torch.float32).view(torch.int32)
    return (base + torch.arange(-6, n - 6, dtype=torch.int32)).view(torch.float32)


def threshold_scene():
    """One stack of equal, isotropic splats (sigma 2 px, depths 2.0 + 0.002 j) per second 8 x 8 sub-tile, centred on a
    pixel: with opacity o = 1 - 1e-4^(1 / (m + 0.5)) the centre pixel stops at list entry m -- m = 4 .. 7 (every position
    of a group of four), 60 .. 63, 64 and 65 (the 64-entry batch boundary), 128 -- and the pixels around it later.  One
    stack of 220 faint splats (lists longer than three batches).  16 splats centred exactly on pixel centres, alone there,
    with opacities 1/255 - 6 ulp .. 1/255 + 9 ulp (bar_opacities): the kernel's alpha there is exp2(log2(opacity)), which
    need not round back to the opacity, so the ladder straddles alpha == ALPHA_MIN."""
    H, W, f = 32, 64, 100.0
    cam = scenes.neutral_camera(H, W, focal=f)
    stops = [4, 5, 6, 7, 60, 61, 62, 63, 64, 65, 128]
    sizes = [m + 6 for m in stops] + [220]
    slots = [(sx, sy) for sy in range(4) for sx in range(8) if (sx + sy) % 2 == 0]          # 16 sub-tiles, 16 px apart
    n_bar = 16
    P = sum(sizes) + n_bar
    a = scenes.dist_a_random(P, H, W, seed=23, focal=f)
    a['rotation'][:] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    start, tx, ty = 0, [], []
    for si, n in enumerate(sizes):
        sx, sy = slots[si]
        r = torch.arange(start, start + n)
        z = 2.0 + 0.002 * torch.arange(n, dtype=torch.float32)
        a['mean_3d'][r, 2] = z
        a['scale'][r] = (2.0 * z / f).view(-1, 1).expand(n, 3)
        o = 0.03 if n == 220 else 1.0 - 1e-4 ** (1.0 / (stops[si] + 0.5))
        a['opacity'][r] = o
        tx += [8 * sx + 4] * n
        ty += [8 * sy + 4] * n
        start += n
    r = torch.arange(start, P)
    a['mean_3d'][r, 2] = 2.5
    a['scale'][r] = (1.5 * 2.5 / f)
    a['opacity'][r] = bar_opacities(n_bar).view(-1, 1)
    for j in range(n_bar):
        sx, sy = slots[len(sizes) + j // 4]
        tx.append(8 * sx + 1 + 4 * (j % 2))
        ty.append(8 * sy + 1 + 4 * ((j // 2) % 2))
    place(a, torch.arange(P), torch.tensor(tx, dtype=torch.float32), torch.tensor(ty, dtype=torch.float32), cam, H, W)
    return a, H, W, cam, stops, r


# ---- tests ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('trial', range(int(os.environ.get('EXA_FUZZ_TRIALS', '16'))))
def test_fuzz_backward_follows_the_forward_decisions(dev, trial):
    """tests/helpers.py fuzz_case: every trial checks every gradient (no trial is excused by a flipped or ambiguous
    decision: the decisions are the HIP forward's own)."""
    a, H, W, cam, G, Gd, Ga, bg = fuzz_case(trial)
    st, _ = check_case(dev, 'fuzz %d' % trial, a, H, W, cam, bg, G, Gd, Ga)
    record_stats('decisions_fuzz_%d' % trial, st)


def test_power_guard_groups_align_between_the_passes(dev):
    """csrc/blend.h power_guard4 applies the "power > 0" skip where a conic is unsafe; the forward groups the list in fours,
    the backward the compacted list.  A guard that reached a SAFE splat grouped with a needle (or a dead needle entry)
    would skip it in one pass and not in the other, at its own centre pixel.  The needles' own pixels are left out
    (check_case ``exclude``): there the float32 conic of a > 10^6 : 1 needle differs from the float64 one by percents, a
    matter of precision, not of decisions.  Every weight of the safe splats and every gradient is checked."""
    a, H, W, cam, S, centres = guard_scene()
    with torch.no_grad():
        pre = ro.preprocess(a['mean_3d'], None, None, a['scale'], a['rotation'], None,
                            ro.settings_from_camera(cam, (H, W), torch.zeros(3)), torch.float32)
    cn = pre['conic'] * -torch.tensor([0.5, 1.0, 0.5]) * 1.4426950408889634          # as staged: (ca, cb, cc)
    tr = cn[:, 0] + cn[:, 2]
    safe = (cn[:, 0] <= 0) & (cn[:, 2] <= 0) & (4 * cn[:, 0] * cn[:, 2] - cn[:, 1] ** 2 >= 1e-5 * tr * tr)
    assert int((~safe[:4]).sum()) >= 3 and bool(safe[S].all()), 'needles must be unsafe, the correlated splats safe'
    assert int((pre['radius'][:4] > 300).sum()) >= 3
    off = torch.stack(((pre['px'][S] - centres[:, 0]).abs(), (pre['py'][S] - centres[:, 1]).abs()), 1)
    assert float(off.max()) <= 3.1e-4
    G, Gd, Ga = _grads_of(H, W, 99)
    bg = torch.rand(3, generator=torch.Generator().manual_seed(98))
    w, _ = decisions(dev, a, H, W, cam)
    needles = torch.zeros(a['mean_3d'].shape[0], dtype=torch.bool)
    needles[:4] = True
    # the suspect, read off the forward: safe splats with no weight at their own centre pixel although the pixel is not
    # left out and still blends entries behind them (alpha there ~ opacity >> 1/255)
    w_c = w[S, centres[:, 1], centres[:, 0]]
    skipped_own = int((w_c == 0).sum())
    st, _ = check_case(dev, 'guard', a, H, W, cam, bg, G, Gd, Ga, w=w, exclude=needles)
    st.update({'safe_skipped_at_own_centre': skipped_own, 'safe': int(S.numel()),
               'needles_blended': int((w[:4] > 0).flatten(1).any(1).sum()), 'dead_blended': int((w[4:100] > 0).sum())})
    record_stats('decisions_guard', st)
    assert st['dead_blended'] == 0, 'the dead entries must never be blended'
    assert st['needles_blended'] >= 3
    assert st['pixels_left_out'] < H * W // 4
    # a safe conic never takes the guard (blend.h power_guard4 is per entry): with alpha ~ opacity at its own centre, no safe
    # splat may be skipped there (a group-wide guard skipped those whose p2 rounds one ulp above lop)
    assert skipped_own == 0, '%d safe splats skipped at their own centre pixel' % skipped_own


def test_thresholds_and_batch_boundaries(dev):
    a, H, W, cam, stops, bar = threshold_scene()
    G, Gd, Ga = _grads_of(H, W, 31)
    bg = torch.rand(3, generator=torch.Generator().manual_seed(32))
    st, w = check_case(dev, 'thresholds', a, H, W, cam, bg, G, Gd, Ga)
    # the scene does what it says.  At the centre pixel of the stack that stops at entry m, entries 0 .. m - 1 have a
    # weight and entry m (the first with T (1 - alpha) < 1e-4) and everything behind it have none
    starts = [0]
    for m in stops:
        starts.append(starts[-1] + m + 6)
    slots = [(sx, sy) for sy in range(4) for sx in range(8) if (sx + sy) % 2 == 0]
    for si, m in enumerate(stops):
        cx, cy = 8 * slots[si][0] + 4, 8 * slots[si][1] + 4
        taken = w[starts[si]:starts[si] + m + 6, cy, cx] > 0
        assert taken[:m].all() and not taken[m:].any(), 'stack %d: blended %s' % (m, taken.int().tolist())
    # the longest stack: more than three batches of blended entries at its centre
    n_blended = (w > 0).sum(0)
    st['max_blended_per_pixel'] = int(n_blended.max())
    assert st['max_blended_per_pixel'] > 3 * 64
    # the 1/255 ladder: alone at its centre pixel (T = 1) a splat's weight IS its alpha.  Some rung is skipped, and some
    # rung is blended with alpha exactly ALPHA_MIN (the skip is alpha < 1/255, not <=)
    bx = torch.tensor([8 * slots[len(stops) + 1 + j // 4][0] + 1 + 4 * (j % 2) for j in range(len(bar))])
    by = torch.tensor([8 * slots[len(stops) + 1 + j // 4][1] + 1 + 4 * ((j // 2) % 2) for j in range(len(bar))])
    alpha_min = float(torch.tensor(1.0 / 255.0, dtype=torch.float32))
    w_bar = w[bar, by, bx]
    st['bar_alpha_at_centre'] = w_bar.tolist()
    assert bool((w_bar == 0).any()), 'no rung of the 1/255 ladder is skipped'
    assert bool((w_bar == alpha_min).any()), 'no rung of the 1/255 ladder has alpha == ALPHA_MIN at its centre'
    assert bool(((w_bar == 0) | (w_bar >= alpha_min)).all())
    record_stats('decisions_thresholds', st)


@pytest.mark.parametrize('deg', [1, 2, 3])
def test_in_kernel_sh_follows_the_forward_decisions(dev, deg):
    """The threshold scene coloured by the rasterizer's own SH evaluation: decisions taken from the rgb probes (colour enters
    none of them: the SH render's mask equals the probes' bit for bit), then the SH gradients."""
    a, H, W, cam, _, _ = threshold_scene()
    P = a['mean_3d'].shape[0]
    g = torch.Generator().manual_seed(40 + deg)
    rgb = 0.3 + 0.4 * torch.rand(P, 3, generator=g)
    sh = scenes.sh_from_rgb(rgb, deg, seed=deg, rest_sigma=0.05)
    s = ro.settings_from_camera(cam, (H, W), torch.zeros(3), deg)
    raw = ro.eval_sh_color(deg, sh.double(), a['mean_3d'].double(), s.campos.double())
    assert float(raw.min()) > 0.05, 'no colour may clamp'
    w, mask = decisions(dev, a, H, W, cam)
    G, Gd, Ga = _grads_of(H, W, 50 + deg)
    bg = torch.rand(3, generator=g)
    geo = {k: a[k] for k in ('mean_3d', 'scale', 'rotation', 'opacity')}
    ag = {k: v.to(dev).requires_grad_(True) for k, v in geo.items()}
    ag['sh'] = sh.to(dev).requires_grad_(True)
    out = exa.GaussianRenderer()({**ag, 'sh_degree': deg}, (H, W), _cam(cam, dev), bg.to(dev))
    assert torch.equal(out['mask'][0].detach().cpu(), mask), 'the SH render took other decisions than the rgb probes'
    _loss(out, G.to(dev), Gd.to(dev), Ga.to(dev)).backward()
    t = {k: v.clone().double().requires_grad_(True) for k, v in geo.items()}
    sht = sh.clone().double().requires_grad_(True)
    ref = do.render(t, (H, W), cam, bg, w > 0, out['radius'].cpu() > 0, sh=sht, sh_degree=deg)
    _loss(ref, G.double(), Gd.double(), Ga.double()).backward()
    st = _assert_planes('sh%d' % deg, out, ref)
    got = {k: ag[k].grad for k in ('mean_3d', 'scale', 'rotation', 'opacity', 'sh')}
    got['mean_2d'] = out['mean_2d'].grad
    want = {k: t[k].grad for k in ('mean_3d', 'scale', 'rotation', 'opacity')}
    want.update({'sh': sht.grad, 'mean_2d': ref['mean_2d'].grad, '_scale': t['scale'].detach()})
    _assert_grads('sh%d' % deg, got, want, st)
    record_stats('decisions_sh%d' % deg, st)


def _batch_check(dev, tag, scenes_, shared):
    """scenes_: 8 x (a, H, W, cam, bg, G, Gd, Ga).  One rasterize_gaussians_batch call; every job against the decision
    oracle with the decisions of its own single-render extraction; gradients summed over the jobs."""
    ws = [decisions(dev, a, H, W, cam)[0] for a, H, W, cam, *_ in scenes_]
    if shared:
        one = {k: v.to(dev).requires_grad_(True) for k, v in scenes_[0][0].items()}
        ags = [one] * len(scenes_)
    else:
        ags = [{k: v.to(dev).requires_grad_(True) for k, v in sc[0].items()} for sc in scenes_]
    jobs = [_raster_job(ag, (H, W), _cam(cam, dev), bg.to(dev)) for ag, (_, H, W, cam, bg, *_r) in zip(ags, scenes_)]
    outs = rasterize_gaussians_batch(jobs)
    loss = 0.0
    for (col, radii, depth, alpha), (_, H, W, cam, bg, G, Gd, Ga) in zip(outs, scenes_):
        loss = loss + _loss({'img': col, 'depthmap': depth, 'mask': alpha}, G.to(dev), Gd.to(dev), Ga.to(dev))
    loss.backward()
    ts = [{k: v.clone().double().requires_grad_(True) for k, v in scenes_[0][0].items()}] * len(scenes_) if shared else \
        [{k: v.clone().double().requires_grad_(True) for k, v in sc[0].items()} for sc in scenes_]
    loss64 = 0.0
    refs = []
    for j, ((col, radii, depth, alpha), (a, H, W, cam, bg, G, Gd, Ga), w, t) in enumerate(zip(outs, scenes_, ws, ts)):
        ref = do.render(t, (H, W), cam, bg, w > 0, radii.cpu() > 0)
        _assert_planes('%s job %d' % (tag, j), {'img': col, 'depthmap': depth, 'mask': alpha}, ref)
        loss64 = loss64 + _loss(ref, G.double(), Gd.double(), Ga.double())
        refs.append(ref)
    loss64.backward()
    st = {'jobs': len(scenes_), 'shared': shared}
    for j, (job, ref) in enumerate(zip(jobs, refs)):
        assert_grads_close(job['means2D'].grad, ref['mean_2d'].grad, '%s job %d mean_2d' % (tag, j))
    for j in range(1 if shared else len(scenes_)):
        got = {k: ags[j][k].grad for k in KEYS}
        want = {k: ts[j][k].grad for k in KEYS}
        want['_scale'] = ts[j]['scale'].detach()
        _assert_grads('%s job %d' % (tag, j), got, want, st)
    return st


def test_batch_of_8_heterogeneous_jobs(dev):
    """Eight different scenes and image sizes in one batched call (fuzz trials 0 .. 7)."""
    sc = []
    for trial in range(8):
        a, H, W, cam, G, Gd, Ga, bg = fuzz_case(trial)
        sc.append((a, H, W, cam, bg, G, Gd, Ga))
    record_stats('decisions_batch_heterogeneous', _batch_check(dev, 'batch', sc, shared=False))


def test_batch_of_8_views_of_shared_tensors(dev):
    """Eight views of the SAME tensors: the backward sums the views inside the per-Gaussian kernel (K > 4: the group
    scratch of jobs 4 .. 7 is used); every view has its own decisions."""
    H, W, f = 40, 56, 100.0
    a = scenes.dist_a_random(240, H, W, seed=61, focal=f, z_range=(2.0, 4.0))
    a['opacity'][4:40] = 1.0 / 255.0
    sc = []
    for v in range(8):
        cam = scenes.ring_camera(H, W, v, 40, radius=3.0, center=(0.0, 0.0, 3.0), focal=f)
        G, Gd, Ga = _grads_of(H, W, 70 + v)
        sc.append((a, H, W, cam, torch.rand(3, generator=torch.Generator().manual_seed(80 + v)), G, Gd, Ga))
    record_stats('decisions_batch_shared', _batch_check(dev, 'shared batch', sc, shared=True))
