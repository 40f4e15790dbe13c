"""Shared helpers of the parity tests: tolerances are BASELINE.json's (image L-inf 1e-4, grads 1e-3 rel)."""
import json
import os

import torch

IMG_TOL = 1e-4        # per-pixel L-infinity on colour / depth / alpha (north_star)
GRAD_REL_TOL = 1e-3   # relative gradient error (north_star)
# Pixels whose discrete decisions (alpha >= 1/255, T < 1e-4, power > 0) sit within 1e-4 (relative) of their
# threshold may flip one decision between two fp32 implementations.  The budget is data driven: the small synthetic
# scenes measure <= 2e-4 of their pixels, the full-size BASELINE workloads assert their own measured counts
# (tests/test_gpu_fullsize.py).
AMBIGUOUS_MAX_FRACTION = 2.5e-3
AMBIGUOUS_TOL = 2e-2            # such a pixel may flip one alpha >= 1/255 / T < 1e-4 decision
# ... and only a handful of them actually do (measured on MI355X: 0-6 pixels off by > 1e-4 out of up to 9 145 ambiguous
# ones, profiles/r02_parity.md): at most max(3, 1 %) of the ambiguous pixels may exceed IMG_TOL
AMBIGUOUS_OFF_MIN, AMBIGUOUS_OFF_FRACTION = 3, 0.01
# per-Gaussian gradient check: |g_i - r_i|_inf <= 1e-3 |r_i|_inf + GAUSS_FLOOR * mean_j |r_j|_inf  (an absolute floor
# for Gaussians whose net gradient is a small difference of large per-pixel contributions; measured need <= 6e-4).
# Gaussians whose 3-sigma square covers an AMBIGUOUS pixel are checked against GAUSS_FLOOR_AMBIGUOUS instead: a
# legitimately flipped alpha / stop decision at that pixel changes exactly their gradients (measured <= 3.6e-2).
GAUSS_FLOOR = 1e-3
GAUSS_FLOOR_AMBIGUOUS = 1e-1


def grad_rel_err(got, ref, abs_scale=0.0):
    """max-norm and L2 relative errors of a gradient tensor.  ``abs_scale``: the natural magnitude of this gradient
    when the reference itself is (near) zero -- e.g. dL/d(rotation) of isotropic Gaussians is EXACTLY zero in the
    oracle while any other evaluation order leaves rounding noise of a few ulp of |dL/d(scale)| * |scale|."""
    ref = ref.double()
    got = got.double()
    scale = ref.abs().max().clamp_min(max(abs_scale, 1e-30))
    l2s = ref.norm().clamp_min(max(abs_scale * ref.numel() ** 0.5, 1e-30))
    return float((got - ref).abs().max() / scale), float((got - ref).norm() / l2s)


def per_gaussian_excess(got, ref, near_ambiguous=None, abs_scale=0.0):
    """max over Gaussians of (|g_i - r_i|_inf - 1e-3 |r_i|_inf) / mean_j |r_j|_inf: the absolute floor (in units of the
    mean per-Gaussian gradient magnitude) a per-Gaussian 1e-3-relative check needs.  Returns (clean, ambiguous): the
    maximum over the Gaussians away from / near ambiguous pixels (``near_ambiguous``: bool [P] or None)."""
    ref = ref.double().reshape(ref.shape[0], -1)
    got = got.double().reshape(got.shape[0], -1)
    if ref.shape[0] == 0:
        return 0.0, 0.0
    rn = ref.abs().amax(1)
    en = (got - ref).abs().amax(1)
    scale = rn.mean().clamp_min(max(abs_scale, 1e-30))
    ex = (en - GRAD_REL_TOL * rn) / scale
    if near_ambiguous is None or not bool(near_ambiguous.any()):
        return float(ex.max()), 0.0
    clean = ex[~near_ambiguous]
    return (float(clean.max()) if clean.numel() else 0.0), float(ex[near_ambiguous].max())


def gaussians_near_pixels(pre, mask):
    """bool [P]: Gaussians whose 3-sigma square (oracle pixel centre +- radius) covers a pixel of ``mask`` [H, W]."""
    ys, xs = torch.nonzero(mask.bool(), as_tuple=True)
    P = pre['px'].shape[0]
    near = torch.zeros(P, dtype=torch.bool)
    if ys.numel() == 0 or P == 0:
        return near
    px, py = pre['px'].detach().float(), pre['py'].detach().float()
    r = pre['radius'].float() + 1.0
    for i in range(0, ys.numel(), 256):          # [256, P] blocks
        x, y = xs[i:i + 256].float()[:, None], ys[i:i + 256].float()[:, None]
        near |= (((px[None] - x).abs() <= r[None]) & ((py[None] - y).abs() <= r[None])).any(0)
    return near & (pre['radius'] > 0)


def image_stats(got, ref, ambiguous):
    got = got.detach().cpu().float()
    ref = ref.detach().cpu().float()
    d = (got - ref).abs()
    if d.dim() == 3:
        d = d.amax(0)
    amb = ambiguous.bool()
    strict = d.clone()
    strict[amb] = 0
    return {'n_ambiguous': int(amb.sum()), 'n_pixels': int(amb.numel()),
            'linf_unambiguous': float(strict.max()) if strict.numel() else 0.0,
            'linf_ambiguous': float(d[amb].max()) if amb.any() else 0.0,
            'n_ambiguous_off': int((d[amb] > IMG_TOL).sum()) if amb.any() else 0}


def assert_image_close(got, ref, ambiguous, name='img', max_ambiguous=None, stats=None):
    st = stats if stats is not None else image_stats(got, ref, ambiguous)
    budget = max_ambiguous if max_ambiguous is not None else AMBIGUOUS_MAX_FRACTION * ambiguous.numel()
    assert st['n_ambiguous'] <= budget, '%s: %d ambiguous pixels (budget %g)' % (name, st['n_ambiguous'], budget)
    assert st['linf_unambiguous'] <= IMG_TOL, '%s: L-inf %.3e on unambiguous pixels' % (name, st['linf_unambiguous'])
    assert st['linf_ambiguous'] <= AMBIGUOUS_TOL, '%s: ambiguous pixel off by %.3e' % (name, st['linf_ambiguous'])
    off_budget = max(AMBIGUOUS_OFF_MIN, AMBIGUOUS_OFF_FRACTION * st['n_ambiguous'])
    assert st['n_ambiguous_off'] <= off_budget, '%s: %d ambiguous pixels differ by > 1e-4 (budget %g)' % (
        name, st['n_ambiguous_off'], off_budget)
    return st


def grad_stats(got, ref, near_ambiguous=None, abs_scale=0.0):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    mx, l2 = grad_rel_err(got, ref, abs_scale)
    clean, amb = per_gaussian_excess(got, ref, near_ambiguous, abs_scale)
    return {'max_rel': mx, 'l2_rel': l2, 'per_gaussian_floor_needed': clean, 'per_gaussian_floor_needed_near_ambiguous': amb}


def rotation_grad_scale(scale, scale_grad_ref):
    """Natural magnitude of dL/d(rotation): |dL/d(scale)| * |scale| (both enter Sigma = R S S^T R^T the same way)."""
    return float(scale_grad_ref.detach().abs().max() * scale.detach().abs().max())


def assert_grads_close(got, ref, name, near_ambiguous=None, per_gaussian=True, abs_scale=0.0):
    """Global 1e-3 relative (max-norm and L2) and -- for [P, ...] tensors -- per Gaussian."""
    st = grad_stats(got, ref, near_ambiguous, abs_scale)
    assert st['max_rel'] <= GRAD_REL_TOL and st['l2_rel'] <= GRAD_REL_TOL, \
        'grad %s: max-rel %.3e, L2-rel %.3e' % (name, st['max_rel'], st['l2_rel'])
    if per_gaussian:
        assert st['per_gaussian_floor_needed'] <= GAUSS_FLOOR, \
            'grad %s: per-Gaussian error exceeds 1e-3 relative + floor (needs floor %.3e)' % (name, st['per_gaussian_floor_needed'])
        assert st['per_gaussian_floor_needed_near_ambiguous'] <= GAUSS_FLOOR_AMBIGUOUS, \
            'grad %s: per-Gaussian error near ambiguous pixels (needs floor %.3e)' % (name, st['per_gaussian_floor_needed_near_ambiguous'])
    return st


def record_stats(tag, stats):
    """Append measured parity statistics to gpurun_out/parity_stats.jsonl (when that directory exists: GPU box runs)."""
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gpurun_out')
    if os.path.isdir(d):
        with open(os.path.join(d, 'parity_stats.jsonl'), 'a') as f:
            f.write(json.dumps({'tag': tag, **stats}) + '\n')


def clamped_scene(H, W, f):
    """400 random Gaussians, the first 40 large ones 35-65 % outside the frustum: the +-1.3 tanfov clamp is active
    for them and they still reach into the image (non-zero gradients)."""
    from exavatar_release_amd import scenes
    a = scenes.dist_a_random(400, H, W, seed=5, focal=f)
    g = torch.Generator().manual_seed(9)
    for i in range(40):
        z = 3.0 + torch.rand(1, generator=g).item()
        side = 1 if i % 2 else -1
        if i % 4 < 2:
            u = side * (0.5 * W / f) * (1.35 + 0.3 * torch.rand(1, generator=g).item())
            a['mean_3d'][i] = torch.tensor([u * z, 0.1 * side, z])
        else:
            u = side * (0.5 * H / f) * (1.4 + 0.2 * torch.rand(1, generator=g).item())
            a['mean_3d'][i] = torch.tensor([0.1 * side, u * z, z])
        a['scale'][i] = torch.tensor([0.5, 0.45, 0.4])
        a['opacity'][i] = 0.6
    return a


def fuzz_case(trial):
    """Seeded random scene salted with edge cases -- opacity 0 / 1 / at the 1/255 bar, scales x1e-4 .. x300, centres at,
    just beyond, before and behind the 0.2 near plane and exactly ON the camera plane, unnormalised quaternions, ragged image
    sizes -- plus all three image gradients.  Shared by the CPU fuzz of the two oracles (tests/test_c_oracle.py) and the GPU
    fuzz of the HIP path (tests/test_gpu_edge_cases.py).  Returns (assets, H, W, cam, G, Gd, Ga, bg)."""
    from exavatar_release_amd import scenes
    g = torch.Generator().manual_seed(1000 + trial)
    H, W = int(torch.randint(9, 70, (1,), generator=g)), int(torch.randint(9, 90, (1,), generator=g))
    P = int(torch.randint(8, 300, (1,), generator=g))
    f = float(torch.rand(1, generator=g) * 150 + 20)
    a = scenes.dist_a_random(P, H, W, seed=trial, focal=f, z_range=(0.1, 8.0))
    n = max(1, P // 8)
    idx = torch.randperm(P, generator=g)
    pick = lambda vals, m: torch.tensor(vals)[torch.randint(0, len(vals), (m,), generator=g)]      # noqa: E731
    a['opacity'][idx[:n]] = pick([0.0, 1.0, 1 / 255.0, 0.0039, 0.0040], n).view(-1, 1)
    a['scale'][idx[n:2 * n]] *= pick([1e-4, 1e-2, 30.0, 300.0], n).view(-1, 1)
    a['mean_3d'][idx[2 * n:3 * n], 2] = pick([0.2, 0.2000001, 0.19, -1.0, 0.0], n)
    a['rotation'][idx[3 * n:4 * n]] *= 3.0
    cam = scenes.ring_camera(H, W, trial % 7, 7, radius=3.0, center=(0.0, 0.0, 3.0), focal=f) if trial % 2 else \
        scenes.neutral_camera(H, W, focal=f)
    G, Gd, Ga = torch.randn(3, H, W, generator=g), torch.randn(1, H, W, generator=g), torch.randn(1, H, W, generator=g)
    bg = torch.rand(3, generator=g)
    return a, H, W, cam, G, Gd, Ga, bg


def extract_weights(render_rgb, P, perm=None):
    """w [P, H, W] (float64): the blend weight the forward gave every (Gaussian, pixel) pair, read off the forward itself.
    ``render_rgb(rgb)`` renders the scene with colours ``rgb`` [P, 3] and background 0 and returns its image [3, H, W].
    Three Gaussians per render carry the one-hot colours (1, 0, 0), (0, 1, 0), (0, 0, 1), all others black: channel c of
    that image is exactly the weight of the c-th of them (every other term is an exact 0).  ceil(P / 3) renders;
    ``perm``: the order in which the Gaussians are grouped.  Colour enters no decision, so the grouping must not
    matter, and a blended pair has w >= (1/255) 1e-4 > 0: ``keep = w > 0``."""
    order = torch.arange(P) if perm is None else perm
    w = None
    for s in range(0, P, 3):
        grp = order[s:s + 3]
        rgb = torch.zeros(P, 3)
        rgb[grp, torch.arange(grp.numel())] = 1.0
        img = render_rgb(rgb).detach().cpu().double()
        if w is None:
            w = torch.zeros(P, img.shape[1], img.shape[2], dtype=torch.float64)
        w[grp] = img[:grp.numel()]
    return w


def needle_scene():
    """The scene of tests/test_gpu_edge_cases.py::test_needle_conics_keep_the_power_guard: needles of 350 .. 3 000 px (conics
    that blend.h conic_safe calls unsafe) among 56 ordinary splats.  Returns (assets, H, W, cam, bg, G)."""
    from exavatar_release_amd import scenes
    H, W, f = 40, 56, 100.0
    a = scenes.dist_a_random(60, H, W, seed=5, focal=f, z_range=(2.0, 4.0))
    g = torch.Generator().manual_seed(77)
    for i, s in enumerate((12.0, 30.0, 100.0, 40.0)):
        a['scale'][i] = torch.tensor([s, 1e-4, 1e-4])
        a['mean_3d'][i] = torch.tensor([0.1 * i - 0.2, 0.05 * i - 0.1, 3.0])
        q = torch.randn(4, generator=g)
        a['rotation'][i] = q / q.norm()
        a['opacity'][i] = 0.6
    cam, bg = scenes.neutral_camera(H, W, focal=f), torch.rand(3, generator=g)
    G = torch.randn(3, H, W, generator=g)
    return a, H, W, cam, bg, G


LOSS_CONTENT = ('uniform', 'photo', 'bright', 'white')


def loss_content(kind, shape, seed=0):
    """(x, y): a rendered image and its target, float32 [B, C, H, W] on the CPU, of one content class of the image-loss
    tests.  'uniform': independent U(0, 1).  'photo': ramps, a hard edge, exact 0 and 1 flats, a textured patch, and
    x == y bit for bit on the left third.  'bright': 0.98 +- 0.002 with the target within 0.001 (sigma^2 = E[x^2] - mu^2
    cancels).  'white': 1 - U(0, 0.004) with a third of the pixels exactly 1."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)

    def r():
        return torch.rand(shape, generator=g)
    if kind == 'uniform':
        return r(), r()
    if kind == 'bright':
        x = 0.98 + 0.002 * (2 * r() - 1)
        return x, x + 0.001 * (2 * r() - 1)
    if kind == 'white':
        x, y = 1 - 0.004 * r(), 1 - 0.004 * r()
        x[r() < 0.33] = 1.0
        y[r() < 0.33] = 1.0
        return x, y
    assert kind == 'photo', kind
    yy = torch.linspace(0, 1, H)[:, None]
    xx = torch.linspace(0, 1, W)[None, :]
    base = (0.15 + 0.5 * (0.7 * xx + 0.3 * yy)).expand(B, C, H, W).clone()
    base += 0.05 * torch.arange(C, dtype=torch.float32)[None, :, None, None]
    base[..., :, (2 * W) // 3:] += 0.2                                       # hard vertical edge
    base[..., H // 4:H // 2 + 1, W // 2:(3 * W) // 4 + 1] = 1.0              # exact flats
    base[..., (3 * H) // 4:, :W // 4 + 1] = 0.0
    tex = (yy * H // 3 + xx * W // 3).floor().remainder(2).bool().expand(B, C, H, W)
    base = torch.where(tex & (base > 0.0) & (base < 1.0), base + 0.1 * r(), base).clamp(0, 1)
    x = (base + 0.03 * (r() - 0.5)).clamp(0, 1)
    keep = (base == 0.0) | (base == 1.0)
    keep[..., :, :W // 3] = True                                             # x == y bit for bit
    return torch.where(keep, base, x), base


# ---- the five renders of an iteration, three ways (tests/test_gpu_edge_cases.py, tests/test_gpu_size_paths.py)
def iteration_case(dev, scene, human, refined, H, W, f, bg, seed, cam=None):
    """render_iteration three ways: merge (composites from the sources' sorted lists), constant prefix (round 2) and the
    reference's own formulation (five renders of torch.cat((scene.detach(), human)))."""
    import exavatar_release_amd as exa
    from exavatar_release_amd import scenes
    KEYS = ('mean_3d', 'scale', 'rotation', 'opacity', 'rgb')
    _to = lambda d, dev_: {k: v.to(dev_).requires_grad_(True) for k, v in d.items()}      # noqa: E731
    cam = cam or scenes.neutral_camera(H, W, focal=f)
    camd = {k: t.to(dev) for k, t in cam.items()}
    g = torch.Generator().manual_seed(seed)
    G = [torch.randn(3, H, W, generator=g).to(dev) for _ in range(5)]
    Gd = [torch.randn(1, H, W, generator=g).to(dev) for _ in range(5)]
    rend = exa.GaussianRenderer()
    res = {}
    for how in ('merge', 'prefix', 'reference'):
        s, h, r = _to(scene, dev), _to(human, dev), _to(refined, dev)
        if how == 'reference':
            cat = lambda a_, b_: {k: torch.cat((a_[k].detach(), b_[k])) for k in KEYS}      # noqa: E731
            jobs = [(s, (H, W), camd), (h, (H, W), camd, bg), (cat(s, h), (H, W), camd), (r, (H, W), camd, bg), (cat(s, r), (H, W), camd)]
            outs = [rend(*j) for j in jobs]
        else:
            out = exa.render_iteration(rend, s, h, r, (H, W), camd, bg, merge=(how == 'merge'))
            outs = [out[k] for k in exa.ITERATION_RENDERS]
        sum((o['img'] * Gi).sum() + (o['depthmap'] * Gdi).sum() + o['mask'].sum() for o, Gi, Gdi in zip(outs, G, Gd)).backward()
        torch.cuda.synchronize()
        m2 = [o['mean_2d'].grad.clone() for o in outs]
        if how == 'reference':                       # the composites' probes cover cat(scene, human): keep the human rows
            nS = scene['mean_3d'].shape[0]
            m2[2], m2[4] = m2[2][nS:], m2[4][nS:]
        res[how] = dict(imgs=[o[k].detach().clone() for o in outs for k in ('img', 'depthmap', 'mask')],
                        radii=[o['radius'].clone() for o in outs], m2=m2,
                        grads=[t[k].grad.clone() for t in (s, h, r) for k in KEYS])
    return res


def assert_iteration_agrees(res):
    ref = res['reference']
    for how in ('merge', 'prefix'):
        got = res[how]
        for i, (x, y) in enumerate(zip(got['imgs'], ref['imgs'])):
            assert torch.equal(x, y), '%s image %d' % (how, i)
        for x, y in zip(got['radii'], ref['radii']):
            assert torch.equal(x, y)
        for i, (x, y) in enumerate(zip(got['grads'] + got['m2'], ref['grads'] + ref['m2'])):
            scale = float(y.abs().max())
            assert float((x - y).abs().max()) <= 1e-5 * scale + 1e-30, '%s grad %d: %g of %g' % (how, i, float((x - y).abs().max()), scale)
