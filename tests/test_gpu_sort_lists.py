"""The per-sub-tile sort of the sort launch (csrc/render_fwd.hip), list by list, at the smallest sizes that reach every path:
the one-wave sorts of the quad workgroups (rank sort up to 64 keys, wave_bucket_sort<2 | 4 | 8> up to WAVE_KEYS, its rank-sort
escape for depths that pile up), the tail workgroups that find the long lists through the batch owners (distribution sort,
merge sort, the register rank sort beyond 2048 keys), and the rule by which they find them.

A scene is a set of LISTS of chosen lengths: n tiny isotropic Gaussians (sigma ~ 1 px, opacity 1) centred in one 8 x 8 sub-tile
each, so that the exact footprint (alpha >= 1/255 within 3.4 px of the centre, the nearest pixel of a neighbour is 4.5 px
away) reaches that sub-tile only, at chosen depths.  The result of a sort is unique -- ascending (depth bits << 32 | id) --
so the check is exact: the sorted ids of every sub-tile are the low words of its keys sorted as unsigned 64-bit integers."""
import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import rasterizer as rz, stats
from exavatar_release_amd.camera import make_raster_matrices

pytestmark = pytest.mark.gpu

# brackets both values of WAVE_KEYS (256, 512), one wave (64), SORT_TILE (2048)
LENGTHS = (1, 63, 64, 65, 128, 255, 256, 257, 511, 512, 513, 1024, 2048, 2049)
PILED = (65, 256, 300, 512, 600)          # all keys of a list at ONE depth: ties by id, BUCKET_MAX exceeded on both paths
FOCAL = 2000.0                            # x / z <= 0.032: the projected covariance stays isotropic to 0.1 %


def _lists(size, pattern):
    """[(sub-tile index, length)] of the scene: one cell (64 x 64) or four cells (128 x 128), long lists in every cell."""
    lengths = PILED if pattern == 'one' else LENGTHS
    out = []
    for i, n in enumerate(lengths):
        if size == 64:
            cx = cy = 0
            lx, ly = (2 * i) % 8, 2 * ((2 * i) // 8)
        else:
            cx, cy = i & 1, (i >> 1) & 1
            lx, ly = 1 + 2 * (i // 4), 3
        out.append(((cy * (size // 64) + cx) * 64 + ly * 8 + lx, n))
    return out


def _scene(size, pattern, seed=0):
    rng = np.random.RandomState(seed)
    px, py, z = [], [], []
    for st, n in _lists(size, pattern):
        cell, local = st // 64, st % 64
        cx, cy = cell % (size // 64), cell // (size // 64)
        px.append(np.full(n, (cx * 8 + local % 8) * 8 + 3.5))
        py.append(np.full(n, (cy * 8 + local // 8) * 8 + 3.5))
        if pattern == 'random':                                   # distinct depths
            d = 2.0 + 4.0 * rng.permutation(n) / max(n, 1)
        elif pattern == 'one':
            d = np.full(n, 3.25)
        elif pattern == 'two':
            d = np.where(rng.rand(n) < 0.5, 3.0, 4.5)
        else:                                                     # 'pairs': every depth twice
            d = 2.0 + 4.0 * (rng.permutation(n) // 2) / max(n, 1)
        z.append(d)
    px, py, z = (np.concatenate(v) for v in (px, py, z))
    perm = rng.permutation(len(z))                                # ids do not follow the lists or the depths
    px, py, z = px[perm], py[perm], z[perm].astype(np.float32).astype(np.float64)
    P = len(z)
    x = (px - (size - 1) / 2) * z / FOCAL
    y = (py - (size - 1) / 2) * z / FOCAL
    f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)         # noqa: E731
    return dict(means3D=f32(np.stack([x, y, z], 1)), scales=f32(np.repeat((0.85 * z / FOCAL)[:, None], 3, 1)),
                rotations=f32(np.tile([1.0, 0.0, 0.0, 0.0], (P, 1))), opacities=torch.ones(P, 1),
                colors_precomp=f32(rng.rand(P, 3)))


def _settings(size, dev):
    cam = {'R': torch.eye(3), 't': torch.zeros(3), 'focal': torch.tensor([FOCAL, FOCAL]),
           'princpt': torch.tensor([size / 2.0, size / 2.0])}
    tanx, tany, vm, pm, cp = make_raster_matrices(cam, (size, size))
    return exa.GaussianRasterizationSettings(size, size, tanx, tany, torch.zeros(3, device=dev), 1.0, vm.to(dev), pm.to(dev), 0,
                                             cp.to(dev), False, False)


def _job(size, pattern, dev):
    sc = {k: v.to(dev) for k, v in _scene(size, pattern).items()}
    P = sc['means3D'].shape[0]
    return dict(raster_settings=_settings(size, dev), means3D=sc['means3D'], means2D=torch.zeros(P, 3, device=dev), shs=None,
                colors_precomp=sc['colors_precomp'], opacities=sc['opacities'], scales=sc['scales'], rotations=sc['rotations'],
                cov3D_precomp=None), P


class _Config:
    """exa.config for the duration of a test."""
    NAMES = ('mode', 'keep_debug', 'fixed_capacity', 'on_overflow')

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {n: getattr(exa.config, n) for n in self.NAMES}
        for n, v in self.kw.items():
            setattr(exa.config, n, v)

    def __exit__(self, *exc):
        for n, v in self.old.items():
            setattr(exa.config, n, v)


def _render(jobs, keep_keys=False, **cfg):
    """Images of the batch (with no_grad: plain forwards) and the workspaces of its LAST job."""
    with _Config(keep_debug=True, **cfg), torch.no_grad():
        outs = rz.rasterize_gaussians_batch(jobs, keep_keys=keep_keys)
        if keep_keys:
            outs = outs[0]
        torch.cuda.synchronize()
        dbg = rz._debug_last
        ws = dbg['tile'].cpu().numpy().copy(), dbg['bin'].cpu().numpy().copy(), int(dbg['capacity'])
    return [tuple(t.clone() for t in o) for o in outs], ws


def _sections(ws, P, size):
    tile, binws, cap = ws
    lay, bins = stats.tile_offsets(P, size, size), stats.bin_offsets(cap)
    nsub = lay['cells'] * 64
    rg = tile[lay['ranges'][0]:lay['ranges'][0] + nsub * 8].view(np.uint32).reshape(-1, 2).astype(np.int64)
    keys = binws[bins['keys'][0]:bins['keys'][0] + cap * 8].view(np.uint64)
    order = binws[bins['sorted'][0]:bins['sorted'][0] + cap * 4].view(np.uint32)
    owner = binws[bins['owner'][0]:bins['owner'][0] + (cap // 64 + 1) * 16].view(np.uint32).reshape(-1, 4).astype(np.int64)
    return rg, keys, order, owner, cap


def _check_lists(ws, P, size, pattern, sorted_keys_in_place=False, unsorted=None):
    """Every list has the length it was built with and is sorted; every long list has exactly one tail workgroup.  Returns
    the keys."""
    rg, keys, order, owner, cap = _sections(ws, P, size)
    n = rg[:, 1] - rg[:, 0]
    expect = np.zeros(len(n), dtype=np.int64)
    for st, length in _lists(size, pattern):
        expect[st] = length
    assert np.array_equal(n, expect), 'list lengths: %s' % {int(s): (int(n[s]), int(expect[s])) for s in np.flatnonzero(n != expect)}
    for st in np.flatnonzero(n > 0):
        b, e = rg[st]
        src = keys[b:e] if unsorted is None else unsorted[st]
        want = np.sort(src)                                       # unsigned 64-bit: depth bits, then id
        got = order[b:e]
        assert np.array_equal(got, (want & np.uint64(0xffffffff)).astype(np.uint32)), \
            'sub-tile %d (n = %d): first wrong position %d' % (st, n[st], int(np.flatnonzero(got != (want & np.uint64(0xffffffff)))[0]))
        if sorted_keys_in_place:
            assert np.array_equal(keys[b:e], want), 'sub-tile %d (n = %d): keys in place' % (st, n[st])
    # the rule of the tail workgroups (sort_subtiles_quads_kernel), for both values of WAVE_KEYS, on the owner records this
    # render left: workgroup t looks at batch slot t * (WAVE_KEYS / 64 + 1) and takes the list that owns it when the list is
    # longer than WAVE_KEYS and no earlier look fell into its slots -- exactly the long lists, each once
    for wk in (256, 512):
        stride = wk // 64 + 1
        took = [int(o[0]) - 1 for slot, o in zip(range(0, cap // 64, stride), owner[0:cap // 64:stride])
                if o[0] != 0 and o[2] > wk and slot - o[1] // 64 < stride]
        assert sorted(took) == np.flatnonzero(n > wk).tolist(), (wk, sorted(took), np.flatnonzero(n > wk).tolist())
    for st in np.flatnonzero(n > 0):                              # (the records the rule reads are the lists' own)
        b, e = rg[st]
        assert np.array_equal(owner[b // 64:b // 64 + (n[st] + 63) // 64], np.tile([st + 1, b, n[st], 0], ((n[st] + 63) // 64, 1)))
    return {int(st): keys[rg[st, 0]:rg[st, 1]].copy() for st in np.flatnonzero(n > 0)}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from exavatar_release_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


_exact = {}


def _exact_render(size, pattern, dev):
    """The exact-mode render of a scene, computed once: (job, P, images, workspaces)."""
    if (size, pattern) not in _exact:
        job, P = _job(size, pattern, dev)
        outs, ws = _render([job], mode='exact', fixed_capacity=None)
        _exact[(size, pattern)] = (job, P, outs[0], ws)
    return _exact[(size, pattern)]


@pytest.mark.parametrize('pattern', ['random', 'one', 'two', 'pairs'])
@pytest.mark.parametrize('size', [64, 128])
def test_every_list_is_sorted_and_the_long_ones_are_listed(dev, size, pattern):
    job, P, _, ws = _exact_render(size, pattern, dev)
    _check_lists(ws, P, size, pattern)


@pytest.mark.parametrize('order', ['small_last', 'large_last'])
def test_batch_of_two_unequal_jobs(dev, order):
    """Two images of different size in one launch: the quads and the tail of the smaller job lie inside the larger grid."""
    small, large = _exact_render(64, 'random', dev), _exact_render(128, 'two', dev)
    pair = [large, small] if order == 'small_last' else [small, large]
    outs, ws = _render([p[0] for p in pair], mode='exact', fixed_capacity=None)
    for got, p in zip(outs, pair):
        assert all(torch.equal(g, w) for g, w in zip(got, p[2]))
    _check_lists(ws, pair[1][1], 64 if order == 'small_last' else 128, 'random' if order == 'small_last' else 'two')


@pytest.mark.parametrize('fits', [True, False])
def test_capacity_mode_equals_exact_mode(dev, fits):
    """A buffer that fits (with unused batch slots behind the lists): the same lists in one fused call.  One that does not:
    the overflowed render is repaired, and what it returns and leaves behind equals exact mode again."""
    job, P, want, ws = _exact_render(128, 'random', dev)
    need = ws[2]
    rz.overflow_events.clear()
    outs, ws2 = _render([job], mode='capacity', fixed_capacity=need + 4096 if fits else 640, on_overflow='retry')
    assert all(torch.equal(g, w) for g, w in zip(outs[0], want))
    assert bool(rz.overflow_events) == (not fits)
    _check_lists(ws2, P, 128, 'random')


def test_kept_keys_are_the_sorted_keys(dev):
    """A merge source of a composite render (keep_sorted_keys): the sorted keys replace the unsorted ones in place."""
    job, P, want, ws = _exact_render(128, 'pairs', dev)
    unsorted = _check_lists(ws, P, 128, 'pairs')
    outs, ws2 = _render([job], keep_keys=True, mode='exact', fixed_capacity=None)
    assert all(torch.equal(g, w) for g, w in zip(outs[0], want))
    _check_lists(ws2, P, 128, 'pairs', sorted_keys_in_place=True, unsorted=unsorted)
