"""GPU tests of the render chain at the image sizes where its launches change path (tests/size_cases.py; the table's path
bits and oracle budgets are checked on the CPU by tests/test_size_cases.py).

(a) every case forward + backward against the C oracle at the project's bars, two-stage and fused, with the timing slots
    saying which scan launches really ran -- which ties ``exa_raster_launch_paths`` to what was launched;
(b) the fused call (merged walk at 257 .. 1023 cells) against the two-stage protocol (scan launches) bit for bit;
(c) the five renders of an iteration -- the composite's range scan in 2, 4 and 16 trips -- three ways, the composite against
    the C oracle, and a GraphedIteration replay;
(d) the sub-tile lists themselves against the per-pixel alpha rule (tests/footprint_oracle.py).
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import _lib
from oracle import c_oracle as co
from oracle import raster_oracle as ro
from tests import size_cases as sc
from tests.helpers import (assert_grads_close, assert_image_close, assert_iteration_agrees, gaussians_near_pixels, grad_stats,
                           image_stats, iteration_case, record_stats, rotation_grad_scale)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import footprint_oracle as fo                                                 # noqa: E402

KEYS = sc.KEYS
NAMES = [c.name for c in sc.CASES]
PLANES = ('img', 'depthmap', 'mask', 'radius', 'is_vis')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    _lib.load()          # fail loudly if the HIP library is missing
    exa.config.mode = 'exact'
    exa.config.fixed_capacity = None
    torch.set_num_threads(min(16, torch.get_num_threads()))      # hundreds of OpenMP threads slow the oracle down
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _config():
    saved = (exa.config.mode, exa.config.fixed_capacity)
    exa.config.mode, exa.config.fixed_capacity = 'exact', None
    yield
    exa.config.mode, exa.config.fixed_capacity = saved
    _lib.timing_enable(False)


def _step(dev, assets, shape, camd, bg, G, mode):
    """One forward + backward in ``mode`` ('exact': the two-stage protocol; 'capacity': the fused call, sized by the exact call
    of the same shape before it).  Returns (outputs, leaves, the timing slots that ran)."""
    exa.config.mode = mode
    _lib.timing_enable(True)
    try:
        a = {k: v.to(dev).requires_grad_(True) for k, v in assets.items()}
        out = exa.GaussianRenderer()(a, shape, camd, bg)
        (out['img'] * G).sum().backward()
        torch.cuda.synchronize()
        ran = set(_lib.timing_read())
    finally:
        _lib.timing_enable(False)
        exa.config.mode = 'exact'
    return out, a, ran


def _results(out, a):
    return [out[k].detach() for k in PLANES] + [a[k].grad for k in KEYS] + [out['mean_2d'].grad]


def _scan_launches_ran(case, fused):
    return sc.M not in _lib.launch_paths(case.W, case.H, case.P, fused=fused)[0]


# ---- (a) every case against the C oracle ----

@pytest.mark.parametrize('name', NAMES)
def test_the_case_agrees_with_the_c_oracle_forward_and_backward(dev, name):
    """Dense random dL/dimg.  Image, depth and alpha within 1e-4 off the oracle's ambiguous pixels, their count within the
    case's budget, radii and is_vis bit-equal, every gradient and mean_2d.grad within 1e-3 relative globally and per Gaussian
    (tests/helpers.py) -- for the two-stage protocol; the fused call of the same inputs then has to give the same bits, and
    the cell-scan slot of the timing table has to have run exactly when the path query says the scans are not merged."""
    c = sc.BY_NAME[name]
    shape = (c.H, c.W)
    assets, cam = c.make()
    g = torch.Generator().manual_seed(1)
    G, bg = torch.randn(3, c.H, c.W, generator=g), torch.rand(3, generator=g)
    camd, Gd, bgd = {k: v.to(dev) for k, v in cam.items()}, G.to(dev), bg.to(dev)
    t0 = time.perf_counter()
    out, a, ran = _step(dev, assets, shape, camd, bgd, Gd, 'exact')
    assert ('cell_scan' in ran) == _scan_launches_ran(c, False) and 'cell_scan' in ran, (name, sorted(ran))
    assert {'preprocess_fwd', 'cell_scatter', 'subtile_bin', 'sort_subtiles', 'render_fwd', 'render_bwd', 'preprocess_bwd'} <= ran
    out_f, a_f, ran_f = _step(dev, assets, shape, camd, bgd, Gd, 'capacity')
    t_gpu = time.perf_counter() - t0
    assert ('cell_scan' in ran_f) == _scan_launches_ran(c, True), (name, sorted(ran_f))
    assert ('cell_scan' in ran_f) == (sc.M not in c.paths), name
    for i, (x, y) in enumerate(zip(_results(out_f, a_f), _results(out, a))):
        assert torch.equal(x, y), '%s: fused and two-stage differ in result %d' % (name, i)
    del out_f, a_f

    ref = co.render(assets, shape, cam, bg, dL_dimg=G)
    amb = ref['pixel_margin'] < 1e-4
    stats = {'P': c.P, 'H': c.H, 'W': c.W, 'cells': sc.cells(c), 'budget': sc.budget(c), 'gpu_seconds_both_modes': round(t_gpu, 3)}
    for key, got, want in (('img', out['img'], ref['img']), ('depth', out['depthmap'], ref['depthmap']),
                           ('alpha', out['mask'], ref['mask'])):
        stats[key] = image_stats(got, want, amb)
    stats['radii_equal'] = bool(torch.equal(out['radius'].cpu(), ref['radius']))
    with torch.no_grad():
        so = ro.settings_from_camera(cam, shape, bg)
        pre = ro.preprocess(assets['mean_3d'], None, assets['opacity'], assets['scale'], assets['rotation'], None, so,
                            torch.float32)
    near = gaussians_near_pixels(pre, amb)
    grads = {k: (a[k].grad if k != 'mean_2d' else out['mean_2d'].grad) for k in KEYS + ('mean_2d',)}
    scale_abs = rotation_grad_scale(assets['scale'], ref['grads']['scale'])
    for k, got in grads.items():
        stats['grad_' + k] = grad_stats(got, ref['grads'][k], near, scale_abs if k == 'rotation' else 0.0)
    print(name, stats)                                              # measure first, record, then assert
    record_stats('size_paths_' + name, stats)
    for key in ('img', 'depth', 'alpha'):
        assert_image_close(None, None, amb, key, sc.budget(c), stats=stats[key])
    assert stats['radii_equal'], 'radii differ'
    assert torch.equal(out['is_vis'].cpu(), ref['is_vis'])
    for k, got in grads.items():
        assert_grads_close(got, ref['grads'][k], k, near, abs_scale=scale_abs if k == 'rotation' else 0.0)


# ---- (b) the fused call against the two-stage protocol ----

@pytest.mark.parametrize('name', sc.FUSED_VS_TWO_STAGE)
def test_fused_call_equals_two_stage_call_bitwise_at_257_to_1023_cells(dev, name):
    """The merged column walk of cell_scatter_kernel (fused call) against col_scan + cell_scan as launches of their own (the
    two-stage protocol never merges) on the same input: every image plane, radii and every gradient with torch.equal, as
    test_gpu_parity.py::test_fused_call_equals_two_stage_call_bitwise does at 16 cells.  Dense gradients into all three planes."""
    c = sc.BY_NAME[name]
    assert sc.M in c.paths
    assets, cam = c.make()
    camd = {k: v.to(dev) for k, v in cam.items()}
    gen = torch.Generator(device=dev).manual_seed(5)
    G = torch.randn(3, c.H, c.W, device=dev, generator=gen)
    Gd = torch.randn(2, c.H, c.W, device=dev, generator=gen)
    res = {}
    try:
        for mode in ('exact', 'capacity'):
            exa.config.mode = mode                 # capacity: sized from the exact call of the same shape just before
            a = {k: v.to(dev).requires_grad_(True) for k, v in assets.items()}
            out = exa.GaussianRenderer()(a, (c.H, c.W), camd, torch.tensor([0.3, 0.2, 0.1], device=dev))
            ((out['img'] * G).sum() + (out['depthmap'] * Gd[:1]).sum() + (out['mask'] * Gd[1:]).sum()).backward()
            res[mode] = _results(out, a)
    finally:
        exa.config.mode = 'exact'
    for i, (x, y) in enumerate(zip(res['exact'], res['capacity'])):
        assert torch.equal(x, y), (name, i)


# ---- (c) the five renders of an iteration ----

def _sets(c):
    scene, cam = c.make()
    human = sc.human(c)
    g = torch.Generator().manual_seed(53)
    refined = {k: (v + 0.01 * torch.randn(v.shape, generator=g) if k == 'mean_3d' else v.clone()) for k, v in human.items()}
    return scene, human, refined, cam


@pytest.mark.parametrize('name', sc.ITERATION)
def test_the_five_renders_of_an_iteration_agree_three_ways(dev, name):
    """render_iteration(merge=True), merge=False and five renders of torch.cat((scene.detach(), human)): images and radii
    bit-equal, gradients to 1e-5 of their maximum (tests/helpers.py assert_iteration_agrees, as at 12 cells in
    test_gpu_edge_cases.py).  The human covers well under half of the image and part of every compose trip (checked on the
    CPU), so compose_kernel's carry crosses trips that hold merged and copied sub-tiles alike."""
    c = sc.BY_NAME[name]
    scene, human, refined, cam = _sets(c)
    res = iteration_case(dev, scene, human, refined, c.H, c.W, None, torch.tensor([0.1, 0.2, 0.3], device=dev), 54, cam=cam)
    assert_iteration_agrees(res)
    assert _lib.launch_paths(c.W, c.H, c.P)[1] == c.trips > 1


def test_the_composite_of_a_510_cell_frame_agrees_with_the_c_oracle(dev):
    """`scene_human` of render_iteration at 1080 x 1920 against the C oracle on the concatenation, as
    test_gpu_edge_cases.py::test_composite_render_agrees_with_the_oracle does at 96 x 128."""
    c = sc.BY_NAME[sc.COMPOSITE_CASE]
    scene, human, _, cam = _sets(c)
    H, W = c.H, c.W
    camd = {k: t.to(dev) for k, t in cam.items()}
    G = torch.randn(3, H, W, generator=torch.Generator().manual_seed(83))
    to = lambda d: {k: v.to(dev).requires_grad_(True) for k, v in d.items()}                     # noqa: E731
    s, h, r = to(scene), to(human), to(human)
    o = exa.render_iteration(exa.GaussianRenderer(), s, h, r, (H, W), camd, torch.ones(3, device=dev))['scene_human']
    (o['img'] * G.to(dev)).sum().backward()
    cat = {k: torch.cat((scene[k], human[k])) for k in KEYS}
    ref = co.render(cat, (H, W), cam, torch.ones(3), dL_dimg=G)
    amb = ref['pixel_margin'] < 1e-4
    budget = int(-(-1.3 * sc.COMPOSITE_AMBIGUOUS // 1))
    stats = {n: image_stats(o[k], ref[k], amb) for n, k in (('img', 'img'), ('depth', 'depthmap'), ('alpha', 'mask'))}
    print('composite', stats)
    record_stats('size_paths_composite_' + c.name, stats)
    for n in stats:
        assert_image_close(None, None, amb, n, budget, stats=stats[n])
    assert torch.equal(o['radius'].cpu(), ref['radius'])
    nS = c.P
    with torch.no_grad():
        so = ro.settings_from_camera(cam, (H, W), torch.ones(3))
        pre = ro.preprocess(cat['mean_3d'], None, cat['opacity'], cat['scale'], cat['rotation'], None, so, torch.float32)
    near = gaussians_near_pixels(pre, amb)[nS:]
    for k in KEYS:
        assert_grads_close(h[k].grad, ref['grads'][k][nS:], k, near,
                           abs_scale=rotation_grad_scale(human['scale'], ref['grads']['scale'][nS:]) if k == 'rotation' else 0.0)
    assert_grads_close(o['mean_2d'].grad, ref['grads']['mean_2d'][nS:], 'mean_2d', near)
    assert all(s[k].grad is None for k in KEYS)          # only the composite was differentiated: the scene is a constant of it


def test_a_graphed_iteration_replay_equals_the_eager_iteration_at_510_cells(dev):
    """One GraphedIteration at 1080 x 1920: the capture and two replays with new values equal the eager iteration bit for bit."""
    c = sc.BY_NAME['portrait20k']
    H, W = c.H, c.W
    scene, human, refined, cam = _sets(c)
    sets = [{k: v.to(dev) for k, v in d.items()} for d in (scene, human, refined)]
    camd = {k: t.to(dev) for k, t in cam.items()}
    gen = torch.Generator().manual_seed(9)
    G = [torch.randn(3, H, W, generator=gen).to(dev) for _ in range(5)]
    rend = exa.GaussianRenderer()

    def run(fn):
        s, h, r = [{k: v.detach().clone().requires_grad_(True) for k, v in d.items()} for d in sets]
        out = fn(s, h, r, camd, bg, None)
        planes = [out[n][k].detach().clone() for n in exa.ITERATION_RENDERS for k in PLANES]
        sum((out[n]['img'] * G[i]).sum() * (0.5 + 0.25 * i) for i, n in enumerate(exa.ITERATION_RENDERS)).backward()
        torch.cuda.synchronize()
        return planes + [t[k].grad.clone() for t in (s, h, r) for k in KEYS] + \
            [out[n]['mean_2d'].grad.clone() for n in exa.ITERATION_RENDERS]

    eager = lambda s, h, r, cam_, bg_, dens=None: exa.render_iteration(rend, s, h, r, (H, W), cam_, bg_, dens)   # noqa: E731
    with exa.GraphedIteration((H, W), dev) as it:
        for i in range(3):
            bg = torch.rand(3, generator=gen).to(dev)
            if i:       # new values every iteration, as an optimizer step leaves them
                sets = [{k: (v + 0.003 * torch.randn(v.shape, generator=gen).to(dev) if k in ('mean_3d', 'rgb') else v)
                         for k, v in d.items()} for d in sets]
            for j, (x, y) in enumerate(zip(run(it), run(eager))):
                assert torch.equal(x, y), 'iteration %d: result %d differs' % (i, j)
        assert it.captures >= 1 and it.overflow_retries == 0


# ---- (d) the lists themselves ----

# Gaussians whose pairs are judged: all of cells1003; a fixed seeded sample elsewhere, because the oracle evaluates 64 pixels in
# float64 for every (Gaussian, sub-tile) pair of the tile rects -- 2.9 M pairs for cells1024 and for portrait150k, which is
# tens of seconds on the CPU.  The well-formedness check always covers every list.
JUDGED = {'cells1003': None, 'cells1024': 2000, 'portrait150k': 8000}


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    """The arrays of tests/_size_paths_dump.py: ONE fresh child process under its own time limit, shared by the tests below."""
    path = str(tmp_path_factory.mktemp('size_paths') / 'lists.npz')
    base = {k: v for k, v in os.environ.items() if k not in ('EXA_BIN_SINGLE_CELLS', 'EXA_FOOTPRINT', 'EXA_SORT_SPLIT_SUBTILES')}
    r = subprocess.run(['timeout', '-k', '10', '150', sys.executable, os.path.join(ROOT, 'tests', '_size_paths_dump.py'), path],
                       cwd=ROOT, env=base, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return dict(np.load(path))


@pytest.mark.parametrize('name', sc.LISTS)
def test_the_lists_are_well_formed_miss_nothing_reached_and_list_nothing_unreachable(dump, name):
    """cells1003: masks by subtile_count_kernel on the default path; cells1024: one workgroup per cell and the split sort;
    portrait150k: the production size.  Two-stage and fused call list the same pairs."""
    c = sc.BY_NAME[name]
    H, W = c.H, c.W
    rec = dump[name + '__exact__records']
    n = JUDGED[name]
    idx = np.arange(len(rec)) if n is None else np.sort(np.random.RandomState(1).permutation(len(rec))[:n])
    cl = fo.classify(rec[idx], H, W)
    cl['g'] = idx[cl['g']]
    cl['key'] = fo.pair_key(cl['g'], cl['sx'], cl['sy'], H, W)
    cnt = fo.counts(cl)
    print(name, 'judged Gaussians', len(idx), cnt)
    assert cnt['MUST'] > 1000 and cnt['MUST_NOT'] > 0, (name, cnt)
    for mode in ('exact', 'capacity'):
        tag = '%s__%s__' % (name, mode)
        assert np.array_equal(dump[tag + 'records'][:, :15], rec[:, :15]), mode
        key = fo.assert_well_formed(rec, dump[tag + 'ranges'], dump[tag + 'ids'], int(dump[tag + 'capacity']), H, W)
        fo.assert_nothing_reached_is_missing(cl, key)
        fo.assert_no_unreachable_pair_is_listed(cl, key)
    e, f = (fo.pair_key(*fo.listed_pairs(dump['%s__%s__ranges' % (name, m)], dump['%s__%s__ids' % (name, m)], H, W), H, W)
            for m in ('exact', 'capacity'))
    assert np.array_equal(np.sort(e), np.sort(f)), 'two-stage and fused call list different pairs'
