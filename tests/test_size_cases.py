"""CPU tests of the size-case table (tests/size_cases.py): every case takes exactly the launch paths it is there for -- asked of
``exa_raster_launch_paths``, which answers from the predicates the launchers call -- and the C oracle alone keeps each case
inside its ambiguity budget and its time.  Conditions on the INPUTS of tests/test_gpu_size_paths.py, not measurements of the
kernels: when a constant moves a threshold, the case that lost its path fails here by name, and the fix is to move the case."""
import time

import pytest
import torch

from exavatar_release_amd import _lib
from oracle import c_oracle as co
from tests import size_cases as sc

NAMES = [c.name for c in sc.CASES]
ORACLE_SECONDS_MAX = 10.0


@pytest.fixture(scope='module', autouse=True)
def _threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    before = co.num_threads()
    co.set_num_threads(min(16, before))
    yield
    co.set_num_threads(before)


def test_the_table_is_consistent():
    assert len(set(NAMES)) == len(NAMES)
    for group in (sc.FUSED_VS_TWO_STAGE, sc.ITERATION, sc.LISTS, (sc.COMPOSITE_CASE,)):
        assert set(group) <= set(NAMES)
    assert all(sc.BY_NAME[n].human is not None for n in sc.ITERATION)
    for c in sc.CASES:
        assert c.paths <= set(_lib.PATH_NAMES.values()), c.name
        assert c.trips == (sc.cells(c) + 255) // 256, c.name
    # the neighbours across every threshold are both in the table
    got = {sc.cells(c) for c in sc.CASES}
    assert {257, 510, 1002, 1003, 1023, 1024, 1025, 4096} <= got


@pytest.mark.parametrize('name', NAMES)
def test_the_case_takes_the_paths_it_is_there_for(name):
    c = sc.BY_NAME[name]
    paths, trips = _lib.launch_paths(c.W, c.H, c.P, fused=True)
    assert paths == set(c.paths), '%s lost its path (%s): the library now takes %s, the table says %s' % (
        name, c.there_for, sorted(paths), sorted(c.paths))
    assert trips == c.trips, '%s: %d compose-scan trips, the table says %d' % (name, trips, c.trips)
    # the two-stage protocol never merges the scans; everything else is a matter of the size alone
    two, trips2 = _lib.launch_paths(c.W, c.H, c.P, fused=False)
    assert two == set(c.paths) - {sc.M, sc.W2} and trips2 == c.trips, name


def test_the_query_refuses_what_the_render_calls_refuse():
    import ctypes
    lib = _lib.load()
    bits = ctypes.c_uint32()
    assert lib.exa_raster_launch_paths(64, 64, 1, 1, None) == -2
    assert lib.exa_raster_launch_paths(-1, 64, 1, 1, ctypes.byref(bits)) == -1
    assert lib.exa_raster_launch_paths(4096, 4097, 1, 1, ctypes.byref(bits)) == -1 and b'4096 cells' in lib.exa_raster_last_error()
    assert _lib.launch_paths(0, 0, 0) == (set(), 0)
    assert _lib.launch_paths(64, 64, 0) == ({sc.M, sc.MR, sc.MP}, 1)           # one cell: the odd walk


@pytest.mark.parametrize('name', NAMES)
def test_the_oracle_alone_keeps_the_case_within_its_budget_and_time(name):
    """The recorded count is this oracle's own on the machine the table was written on; another build of it may differ by a
    few pixels, which is what the factor 1.3 of the budget is for."""
    c = sc.BY_NAME[name]
    assets, cam = c.make()
    assert assets['mean_3d'].shape[0] == c.P
    g = torch.Generator().manual_seed(1)
    G, bg = torch.randn(3, c.H, c.W, generator=g), torch.rand(3, generator=g)
    t0 = time.perf_counter()
    ref = co.render(assets, (c.H, c.W), cam, bg, dL_dimg=G)
    dt = time.perf_counter() - t0
    n = int((ref['pixel_margin'] < 1e-4).sum())
    print('%s: oracle %.2f s (table %.2f), %d ambiguous pixels (table %d, budget %d), %d visible, %d tile instances' % (
        name, dt, c.oracle_s, n, c.ambiguous, sc.budget(c), int((ref['radius'] > 0).sum()), ref['num_rendered']))
    assert n <= sc.budget(c), '%s: the oracle alone counts %d ambiguous pixels, budget %d' % (name, n, sc.budget(c))
    assert dt < ORACLE_SECONDS_MAX, '%s: the oracle needs %.1f s: shrink the set, not the image' % (name, dt)
    assert int((ref['radius'] > 0).sum()) >= 2000, 'the case must put work on the screen'
    if name == 'chunks1025':
        assert int((ref['radius'] > 0).sum()) <= 5000 and ref['num_rendered'] <= 50_000     # the lists stay small
        vis = torch.nonzero(ref['radius'] > 0).flatten()
        assert int(vis.min()) < 1024 and int(vis.max()) >= 1024 * 1024                      # first and last chunk


def _subtile_any(mask, H, W):
    """[cells, 64] bool: any pixel of ``mask`` [H, W] per sub-tile, cells row-major as the kernels number them."""
    Hc, Wc = (H + 63) // 64, (W + 63) // 64
    pad = torch.zeros(Hc * 64, Wc * 64, dtype=torch.bool)
    pad[:H, :W] = mask
    return pad.view(Hc, 8, 8, Wc, 8, 8).permute(0, 3, 1, 4, 2, 5).reshape(Hc * Wc, 64, 64).any(2)


@pytest.mark.parametrize('name', sc.ITERATION)
def test_the_human_is_in_front_covers_under_half_and_splits_every_compose_trip(name):
    c = sc.BY_NAME[name]
    assets, cam = c.make()
    h = sc.human(c)
    depth = lambda a: (a['mean_3d'] @ cam['R'].T + cam['t'])[:, 2]                                # noqa: E731
    assert float(depth(h).max()) <= 1.8 + 1e-4 and float(depth(assets)[depth(assets) > 0.2].min()) >= 1.9
    r = co.render(h, (c.H, c.W), cam, torch.ones(3))
    covered = r['mask'][0] > 0
    assert float(covered.float().mean()) < 0.45, name
    with_h = _subtile_any(covered, c.H, c.W)
    inside = _subtile_any(torch.ones(c.H, c.W, dtype=torch.bool), c.H, c.W)
    for trip in range(c.trips):
        sl = slice(256 * trip, 256 * (trip + 1))
        assert int(with_h[sl].sum()) > 0 and int((inside[sl] & ~with_h[sl]).sum()) > 0, (name, trip)
    if name == sc.COMPOSITE_CASE:
        cat = {k: torch.cat((assets[k], h[k])) for k in sc.KEYS}
        n = int((co.render(cat, (c.H, c.W), cam, torch.ones(3))['pixel_margin'] < 1e-4).sum())
        print('%s + human: %d ambiguous pixels (table %d)' % (name, n, sc.COMPOSITE_AMBIGUOUS))
        assert n <= int(-(-1.3 * sc.COMPOSITE_AMBIGUOUS // 1))
