"""The paths whose guards the kernels' prologues sit next to (csrc/common.h, "prologue discipline"): every step kernel reads
its job record and its descriptor words up front, so each load that moved sits right behind the test that makes its address
valid -- workgroups beyond a job's own chunks / cells / sub-tiles in a batch of unequal jobs, pointers that are null in plain
renders (``dL_ddepth``, ``dL_dalpha``, ``splats2``, ``src_*``, ``shs``), the entry ranges of an overflowed render, workspaces
that hold another render's context.  Outputs are what they were: every case is held against the CPU oracle with the bars of
``tests/helpers.py`` and, where the project already holds an equality (a job of a batch = the job alone, ``StaticRender`` = the
autograd surface, repair = exact mode, composite images = the concatenation's), bit for bit.

Sizes: at most 3 000 Gaussians on 200 x 136 pixels (4 x 3 cells, 17 sub-tile rows: padding sub-tiles in the border cells,
three chunks of 1 024 Gaussians).  The oracle of that scene is computed once and shared."""
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import rasterizer as rz
from exavatar_release_amd import scenes
from exavatar_release_amd.camera import make_raster_matrices
from oracle import raster_oracle as ro
from tests.helpers import assert_grads_close, assert_image_close, gaussians_near_pixels, rotation_grad_scale

pytestmark = pytest.mark.gpu

KEYS = ('mean_3d', 'scale', 'rotation', 'opacity', 'rgb')
STATIC_NAMES = {'mean_3d': 'means3D', 'scale': 'scales', 'rotation': 'rotations', 'opacity': 'opacities', 'rgb': 'colors_precomp'}
H1, W1, F1 = 136, 200, 260.0


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from exavatar_release_amd import _lib
    _lib.load()          # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


def _to(d, dev, grad=True):
    return {k: v.to(dev).requires_grad_(grad) for k, v in d.items()}


def _settings(cam, H, W, bg, dev, sh_degree=0):
    tanx, tany, view, proj, campos = make_raster_matrices(cam, (H, W))
    return exa.GaussianRasterizationSettings(H, W, tanx, tany, bg, 1.0, view.to(dev).contiguous(), proj.to(dev).contiguous(),
                                             sh_degree, campos.to(dev).contiguous(), False, False)


class _Case:
    """One scene with its image gradients and, computed once, the oracle's render and gradients (all three image gradients
    given, and the colour gradient alone)."""

    def __init__(self, assets, H, W, cam, bg, seed):
        self.a, self.H, self.W, self.cam, self.bg = assets, H, W, cam, bg
        g = torch.Generator().manual_seed(seed)
        self.G, self.Gd, self.Ga = (torch.randn(n, H, W, generator=g) for n in (3, 1, 1))
        self._ref = None

    def ref(self):
        if self._ref is None:
            leaves = {k: v.clone().requires_grad_(True) for k, v in self.a.items()}
            out = ro.render(leaves, (self.H, self.W), self.cam, self.bg, return_aux=True)
            names = list(KEYS)
            inputs = [leaves[k] for k in names] + [out['mean_2d']]

            def grads(loss, keep):                                       # (nothing visible: the images are constants)
                if not loss.requires_grad:
                    return [None] * len(inputs)
                return torch.autograd.grad(loss, inputs, retain_graph=keep, allow_unused=True)
            full = grads((out['img'] * self.G).sum() + (out['depthmap'] * self.Gd).sum() + (out['mask'] * self.Ga).sum(), True)
            colour = grads((out['img'] * self.G).sum(), False)
            zero = lambda t, like: torch.zeros_like(like) if t is None else t      # noqa: E731
            amb = ro.ambiguous_pixel_mask(out['aux'], self.H, self.W)
            self._ref = dict(img=out['img'].detach(), depth=out['depthmap'].detach(), alpha=out['mask'].detach(),
                             radius=out['radius'], amb=amb, near=gaussians_near_pixels(out['aux']['pre'], amb), leaves=leaves,
                             full={k: zero(t, i) for k, t, i in zip(names + ['mean_2d'], full, inputs)},
                             colour={k: zero(t, i) for k, t, i in zip(names + ['mean_2d'], colour, inputs)})
        return self._ref

    def assert_oracle(self, img, depth, alpha, radii, grads, which='full', name=''):
        """The bars of tests/helpers.py: images 1e-4 off the ambiguous pixels, radii equal, gradients 1e-3 relative globally
        and per Gaussian.  ``grads``: {asset key or 'mean_2d': tensor}; ``which``: the oracle gradient set ('full' / 'colour')."""
        r = self.ref()
        assert_image_close(img, r['img'], r['amb'], name + ' img')
        assert_image_close(depth, r['depth'], r['amb'], name + ' depth')
        assert_image_close(alpha, r['alpha'], r['amb'], name + ' alpha')
        assert torch.equal(radii.cpu(), r['radius']), name + ' radii'
        for k, got in grads.items():
            ref = r[which][k]
            scale = rotation_grad_scale(r['leaves']['scale'], r[which]['scale']) if k == 'rotation' else 0.0
            assert_grads_close(got.reshape(ref.shape), ref, name + ' ' + k, r['near'], abs_scale=scale)


@pytest.fixture(scope='module')
def main_case():
    """3 000 Gaussians (three chunks) on 200 x 136: the first job of every test here."""
    g = torch.Generator().manual_seed(11)
    return _Case(scenes.dist_a_random(3000, H1, W1, seed=31, focal=F1), H1, W1, scenes.neutral_camera(H1, W1, focal=F1),
                 torch.rand(3, generator=g), 12)


def _loss(o, c, dev, depth_alpha=True):
    loss = (o['img'] * c.G.to(dev)).sum()
    if depth_alpha:
        loss = loss + (o['depthmap'] * c.Gd.to(dev)).sum() + (o['mask'] * c.Ga.to(dev)).sum()
    return loss


def _render(dev, cases, batched, depth_alpha=True):
    """The cases as ONE batched call or one call each; -> per case (output dict, asset leaves), gradients filled."""
    rend = exa.GaussianRenderer()
    leaves = [_to(c.a, dev) for c in cases]
    jobs = [(a, (c.H, c.W), {k: v.to(dev) for k, v in c.cam.items()}, c.bg.to(dev)) for a, c in zip(leaves, cases)]
    outs = exa.render_many(rend, jobs) if batched else [rend(*j) for j in jobs]
    sum(_loss(o, c, dev, depth_alpha) for o, c in zip(outs, cases)).backward()
    torch.cuda.synchronize()
    return list(zip(outs, leaves))


def _assert_same(got, ref, name):
    (og, lg), (orf, lr) = got, ref
    for k in ('img', 'depthmap', 'mask', 'radius', 'is_vis'):
        assert torch.equal(og[k], orf[k]), '%s: %s differs' % (name, k)
    assert torch.equal(og['mean_2d'].grad, orf['mean_2d'].grad), name + ': mean_2d gradient differs'
    for k in KEYS:
        assert torch.equal(lg[k].grad, lr[k].grad), '%s: gradient of %s differs' % (name, k)


def _grads_of(o, leaves):
    return {**{k: leaves[k].grad for k in KEYS}, 'mean_2d': o['mean_2d'].grad}


@pytest.mark.parametrize('mode', ['exact', 'capacity'])
def test_jobs_of_unequal_size_in_one_batched_call(dev, main_case, mode):
    """Three jobs that differ in chunks, cells and sub-tiles share every launch: the grids are the largest job's, so the two
    small jobs have workgroups beyond their own chunks, cells * parts and sub-tiles + ordering workgroups in every kernel,
    and the third (everything behind the camera) has no instance at all.  Every job = the job alone, bit for bit, in both
    batch orders; against the oracle; and the headers say that the jobs are what the test means them to be."""
    small = _Case(scenes.dist_a_random(40, 64, 64, seed=32, focal=90.0), 64, 64, scenes.neutral_camera(64, 64, focal=90.0),
                  torch.tensor([0.2, 0.5, 0.1]), 13)
    behind_a = scenes.dist_a_random(1100, 40, 72, seed=33, focal=100.0)
    behind_a['mean_3d'][:, 2] = -behind_a['mean_3d'][:, 2].abs() - 0.5
    behind = _Case(behind_a, 40, 72, scenes.neutral_camera(40, 72, focal=100.0), torch.tensor([0.9, 0.1, 0.4]), 14)
    cases = [main_case, small, behind]
    exa.config.keep_debug = True
    exa.config.mode = 'exact'
    exa.config.fixed_capacity = None
    singles_exact = _render(dev, cases[:1], False)
    need = rz.last_header()[0]
    if mode == 'capacity':
        exa.config.mode = 'capacity'
    caps = [need + 128, 16384, 64]

    def run(order, batched):
        if mode == 'capacity':
            exa.config.fixed_capacity = [caps[i] for i in order] if batched else None
        res = [None] * len(cases)
        if batched:
            for i, r in zip(order, _render(dev, [cases[i] for i in order], True)):
                res[i] = r
        else:
            for i in order:
                if mode == 'capacity':
                    exa.config.fixed_capacity = caps[i]
                res[i] = _render(dev, [cases[i]], False)[0]
        return res
    singles = run([0, 1, 2], False)
    _assert_same(singles[0], singles_exact[0], 'capacity mode against exact mode' if mode == 'capacity' else 'exact mode twice')
    batch = run([0, 1, 2], True)
    hdr_behind = dict(zip(rz.HEADER_FIELDS, rz.last_header()))           # (the header of the call's LAST job)
    batch_rev = run([2, 1, 0], True)
    hdr_main = dict(zip(rz.HEADER_FIELDS, rz.last_header()))
    assert hdr_behind['num_instances'] == 0 and hdr_behind['num_rendered'] == 0 and hdr_behind['num_visible'] == 0 \
        and hdr_behind['active_cells'] == 0 and hdr_behind['overflow'] == 0, hdr_behind
    assert hdr_main['active_cells'] > 1 and hdr_main['num_rendered'] == need and hdr_main['overflow'] == 0, hdr_main
    for i, name in enumerate(('3 000 on 200 x 136', '40 on 64 x 64', '1 100 behind the camera')):
        _assert_same(batch[i], singles[i], name + ' (batch order 0 1 2)')
        _assert_same(batch_rev[i], singles[i], name + ' (batch order 2 1 0)')
    for c, (o, leaves), name in zip(cases, batch, ('main', 'small', 'behind')):
        c.assert_oracle(o['img'], o['depthmap'], o['mask'], o['radius'], _grads_of(o, leaves), 'full', name)
    o, leaves = batch[2]
    assert int(o['radius'].abs().sum()) == 0 and all(float(leaves[k].grad.abs().max()) == 0.0 for k in KEYS)


def _static(dev, c, capacity, **kw):
    a = {k: v.to(dev) for k, v in c.a.items()}
    sr = exa.StaticRender(a['mean_3d'], a['opacity'], a['scale'], a['rotation'], colors_precomp=a['rgb'],
                          image_size=(c.H, c.W), capacity=capacity, **kw)
    return sr, a


def _static_grads(sr, out=0):
    g = sr.grad_outputs(out)
    return {**{k: g[STATIC_NAMES[k]] for k in KEYS}, 'mean_2d': g['means2D']}


def _assert_static_equals(sr, ref, name, grads=True, out=0):
    o, leaves = ref
    assert torch.equal(sr.color, o['img'].detach()) and torch.equal(sr.depth, o['depthmap'].detach()) \
        and torch.equal(sr.alpha, o['mask'].detach()), name + ': images differ'
    assert torch.equal(sr.radii, o['radius']), name + ': radii differ'
    if grads:
        got = _static_grads(sr, out)
        for k in KEYS:
            assert torch.equal(got[k].view_as(leaves[k].grad), leaves[k].grad), '%s: gradient of %s differs' % (name, k)
        assert torch.equal(got['mean_2d'], o['mean_2d'].grad), name + ': mean_2d gradient differs'


def test_overflow_is_repaired_or_raised_with_a_backward_queued(dev, main_case):
    """Capacity 64 where the render needs thousands of instances: the binning kernels find the overflow word in their
    second trip and must touch no entry range of that render.  'repair': the same bits as exact mode.  'raise': the forward
    and the backward queued behind it run through on the overflowed workspaces, check() raises, the process goes on."""
    c = main_case
    exa.config.mode = 'exact'
    ref = _render(dev, [c], False)[0]
    st = _settings(c.cam, c.H, c.W, c.bg.to(dev), dev)
    a = {k: v.to(dev) for k, v in c.a.items()}
    need = exa.required_capacity(a['mean_3d'], a['opacity'], a['scale'], a['rotation'], colors_precomp=a['rgb'], settings=st)
    assert need > 20 * 64, need                                          # far more than the 64 the buffers hold
    G, Gd, Ga = c.G.to(dev), c.Gd.to(dev), c.Ga.to(dev)
    sr, _ = _static(dev, c, 64, on_overflow='repair')
    with sr:
        v = sr.add_view(st, dL_dcolor=G, dL_ddepth=Gd, dL_dalpha=Ga)
        sr.forward(v)
        sr.backward()
        sr.check()
        assert sr.repairs == 1 and sr.capacity >= need
        _assert_static_equals(sr, ref, 'repaired render against exact mode')
        c.assert_oracle(sr.color, sr.depth, sr.alpha, sr.radii, _static_grads(sr), 'full', 'repaired')
    sr, _ = _static(dev, c, 64, on_overflow='raise')
    with sr:
        v = sr.add_view(st, dL_dcolor=G, dL_ddepth=Gd, dL_dalpha=Ga)
        sr.forward(v)
        sr.backward()                                                    # queued behind the overflowed forward
        with pytest.raises(RuntimeError, match='needed %d instances' % need):
            sr.check()
        torch.cuda.synchronize()                                         # no fault behind it: the process goes on
    sr, _ = _static(dev, c, need, on_overflow='raise')
    with sr:
        v = sr.add_view(st, dL_dcolor=G, dL_ddepth=Gd, dL_dalpha=Ga)
        sr.forward(v)
        sr.backward()
        sr.check()
        _assert_static_equals(sr, ref, 'the render after the raised overflow')


def test_no_grad_forward_then_training_forward_on_the_same_workspaces(dev, main_case):
    """A forward without the stored context (the inference blend: no checkpoints, no masks, no backward order) and a training
    forward take turns on ONE set of workspaces, for two cameras: each finds the other's leftovers in the header, the
    owner records, the order words and the checkpoints.  Every render = a fresh one, bit for bit; a backward after each
    training forward."""
    c = main_case
    exa.config.mode = 'exact'
    cam2 = scenes.ring_camera(c.H, c.W, 2, 9, radius=3.0, center=(0.0, 0.0, 3.5), focal=F1)
    other = _Case(c.a, c.H, c.W, cam2, c.bg, 12)
    other.G, other.Gd, other.Ga = c.G, c.Gd, c.Ga
    fresh = [_render(dev, [c], False)[0], _render(dev, [other], False)[0]]
    bg = c.bg.to(dev)
    sts = [_settings(c.cam, c.H, c.W, bg, dev), _settings(cam2, c.H, c.W, bg, dev)]
    a = {k: v.to(dev) for k, v in c.a.items()}
    need = exa.required_capacity(a['mean_3d'], a['opacity'], a['scale'], a['rotation'], colors_precomp=a['rgb'], settings=sts)
    G, Gd, Ga = c.G.to(dev), c.Gd.to(dev), c.Ga.to(dev)
    sr, _ = _static(dev, c, need)
    with sr:
        views = [sr.add_view(st, dL_dcolor=G, dL_ddepth=Gd, dL_dalpha=Ga) for st in sts]
        for view, train in ((0, False), (0, True), (1, False), (0, True), (1, True), (0, False), (1, True)):
            sr.train = train                                             # (what selects store_ctx of the forward call)
            sr.forward(views[view])
            sr.train = True
            if train:
                sr.backward()
            sr.check()
            _assert_static_equals(sr, fresh[view], 'view %d, %s the context' % (view, 'with' if train else 'without'), grads=train)
            if view == 0:
                c.assert_oracle(sr.color, sr.depth, sr.alpha, sr.radii, _static_grads(sr) if train else {}, 'full',
                                'train' if train else 'no_grad')


def test_one_small_composite(dev):
    """Scene plus human through the composite instantiations (the blends' TWO / PREFIX code, ``splats2`` and ``src_*`` set,
    compose.hip's merged lists): images and radii equal the render of the concatenation bit for bit and the gradients agree
    with it as tests/test_gpu_edge_cases.py holds it for larger scenes (1e-5 of the largest entry); against the oracle on
    the concatenation with the bars of tests/helpers.py."""
    H, W, f = 96, 128, 150.0
    scene = scenes.dist_a_random(1500, H, W, seed=81, focal=f)
    human = scenes.dist_a_random(800, H, W, seed=82, focal=f, z_range=(2.0, 4.0))
    cam = scenes.ring_camera(H, W, 2, 9, radius=3.0, center=(0.0, 0.0, 3.0), focal=f)
    camd = {k: t.to(dev) for k, t in cam.items()}
    g = torch.Generator().manual_seed(83)
    G, Gd = torch.randn(3, H, W, generator=g), torch.randn(1, H, W, generator=g)
    bg = torch.ones(3)
    exa.config.mode = 'exact'
    rend = exa.GaussianRenderer()

    def loss(o):
        return (o['img'] * G.to(dev)).sum() + (o['depthmap'] * Gd.to(dev)).sum() + o['mask'].sum()
    s, h, r = _to(scene, dev), _to(human, dev), _to(human, dev)
    o = exa.render_iteration(rend, s, h, r, (H, W), camd, bg.to(dev), merge=True)['scene_human']
    loss(o).backward()
    s2, h2 = _to(scene, dev), _to(human, dev)
    cat = {k: torch.cat((s2[k].detach(), h2[k])) for k in KEYS}
    oc = rend(cat, (H, W), camd, bg.to(dev))
    loss(oc).backward()
    torch.cuda.synchronize()
    nS = scene['mean_3d'].shape[0]
    for k in ('img', 'depthmap', 'mask', 'radius'):
        assert torch.equal(o[k], oc[k]), k
    for k in KEYS:
        scale = float(h2[k].grad.abs().max())
        assert float((h[k].grad - h2[k].grad).abs().max()) <= 1e-5 * scale + 1e-30, k
        assert s[k].grad is None                                         # the scene is a constant of the composite
    m2 = oc['mean_2d'].grad[nS:]
    assert float((o['mean_2d'].grad - m2).abs().max()) <= 1e-5 * float(m2.abs().max()) + 1e-30
    h3 = {k: v.clone().requires_grad_(True) for k, v in human.items()}
    ref = ro.render({k: torch.cat((scene[k], h3[k])) for k in KEYS}, (H, W), cam, bg, return_aux=True)
    ((ref['img'] * G).sum() + (ref['depthmap'] * Gd).sum() + ref['mask'].sum()).backward()
    amb = ro.ambiguous_pixel_mask(ref['aux'], H, W)
    assert_image_close(o['img'], ref['img'], amb, 'img')
    assert_image_close(o['depthmap'], ref['depthmap'], amb, 'depth')
    assert_image_close(o['mask'], ref['mask'], amb, 'alpha')
    assert torch.equal(o['radius'].cpu(), ref['radius'])
    near = gaussians_near_pixels(ref['aux']['pre'], amb)[nS:]
    for k in KEYS:
        assert_grads_close(h[k].grad, h3[k].grad, k, near,
                           abs_scale=rotation_grad_scale(h3['scale'], h3['scale'].grad) if k == 'rotation' else 0.0)
    assert_grads_close(o['mean_2d'].grad, ref['mean_2d'].grad[nS:], 'mean_2d', near)


def test_sh_degree_3_at_300_gaussians(dev):
    """In-kernel SH colours at degree 3, P = 300: one partly filled 256-thread preprocess workgroup behind a full one (the
    staged coefficient blocks, `shs` set and `colors_precomp` null, the camera position next to the matrices).  Against the
    oracle; ``StaticRender`` = the autograd surface bit for bit."""
    H, W, f, P = 72, 88, 110.0, 300
    a = scenes.dist_a_random(P, H, W, seed=41, focal=f)
    sh = scenes.sh_from_rgb(a['rgb'], 3, seed=4, rest_sigma=0.3)
    cam = scenes.ring_camera(H, W, 3, 40, radius=4.0, center=(0, 0, 4.0), focal=f)
    g = torch.Generator().manual_seed(42)
    G, bg = torch.randn(3, H, W, generator=g), torch.rand(3, generator=g)
    exa.config.mode = 'exact'
    st = _settings(cam, H, W, bg.to(dev), dev, 3)
    ag = {k: v.to(dev).requires_grad_(True) for k, v in a.items() if k != 'rgb'}
    shg = sh.to(dev).contiguous().requires_grad_(True)
    m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
    col, rad, dep, alp = exa.GaussianRasterizer(st)(means3D=ag['mean_3d'], means2D=m2, opacities=ag['opacity'], shs=shg,
                                                     scales=ag['scale'], rotations=ag['rotation'])
    (col * G.to(dev)).sum().backward()
    ac = {k: v.clone().requires_grad_(True) for k, v in a.items()}
    shc = sh.clone().requires_grad_(True)
    ref = ro.rasterize(ac['mean_3d'], torch.zeros(P, 3), ac['opacity'], shs=shc, scales=ac['scale'], rotations=ac['rotation'],
                       settings=ro.settings_from_camera(cam, (H, W), bg, 3), return_aux=True)
    (ref[0] * G).sum().backward()
    amb = ro.ambiguous_pixel_mask(ref[4], H, W)
    assert_image_close(col, ref[0], amb, 'img')
    assert torch.equal(rad.cpu(), ref[1])
    near = gaussians_near_pixels(ref[4]['pre'], amb)
    assert_grads_close(shg.grad, shc.grad, 'shs', near)
    for k in ('mean_3d', 'scale', 'rotation', 'opacity'):
        assert_grads_close(ag[k].grad, ac[k].grad, k, near,
                           abs_scale=rotation_grad_scale(ac['scale'], ac['scale'].grad) if k == 'rotation' else 0.0)
    d = {k: v.detach() for k, v in ag.items()}
    with exa.StaticRender(d['mean_3d'], d['opacity'], d['scale'], d['rotation'], shs=shg.detach(), image_size=(H, W),
                          capacity=64) as sr:                             # (repaired inside the first forward)
        v = sr.add_view(st, dL_dcolor=G.to(dev))
        sr.forward(v)
        sr.backward()
        sr.check()
        assert torch.equal(sr.color, col.detach()) and torch.equal(sr.depth, dep.detach()) and torch.equal(sr.alpha, alp.detach())
        assert torch.equal(sr.radii, rad)
        assert torch.equal(sr.grads['shs'], shg.grad) and torch.equal(sr.grads['means3D'], ag['mean_3d'].grad)
        assert torch.equal(sr.grads['means2D'], m2.grad)


def test_depth_and_alpha_gradients_given_then_absent(dev, main_case):
    """``dL_ddepth`` and ``dL_dalpha`` both given (the blend backward's depth instantiation, both pointers read), then both
    absent (both null in the job record: the plain instantiation must not read through them).  Against the oracle's two
    gradient sets; ``StaticRender`` = the autograd surface bit for bit, one object per combination on the same inputs."""
    c = main_case
    exa.config.mode = 'exact'
    st = _settings(c.cam, c.H, c.W, c.bg.to(dev), dev)
    a = {k: v.to(dev) for k, v in c.a.items()}
    need = exa.required_capacity(a['mean_3d'], a['opacity'], a['scale'], a['rotation'], colors_precomp=a['rgb'], settings=st)
    for depth_alpha, which in ((True, 'full'), (False, 'colour'), (True, 'full')):
        o, leaves = _render(dev, [c], False, depth_alpha)[0]
        c.assert_oracle(o['img'], o['depthmap'], o['mask'], o['radius'], _grads_of(o, leaves), which, which)
        sr, _ = _static(dev, c, need)
        with sr:
            v = sr.add_view(st, dL_dcolor=c.G.to(dev), dL_ddepth=c.Gd.to(dev) if depth_alpha else None,
                            dL_dalpha=c.Ga.to(dev) if depth_alpha else None)
            sr.forward(v)
            sr.backward()
            sr.check()
            _assert_static_equals(sr, (o, leaves), 'StaticRender, image gradients: ' + which)
