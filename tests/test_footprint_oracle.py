"""tests/footprint_oracle.py against the designed arithmetic, on the CPU, before any of it judges the device.

Records are built with oracle/raster_oracle.preprocess in float32 (bit-identical to the kernel's preprocess but for the
hardware log) and the sub-tile rect formula of csrc/preprocess_fwd.hip, for every case of tests/_footprint_dump.py.  Required:
MUST lies inside the rect; the float32 model of make_footprint / footprint_band / rows_mask (``model_mask``) contains MUST and is
disjoint from MUST_NOT, i.e. the oracle's two bounds really bracket the designed arithmetic; the cases have the teeth the GPU test
relies on; and the assertions of the GPU test, fed a deliberately broken model in place of the device's lists, fail.

One mistake they cannot see: dropping the `- 1e-3 - 1e-5 mag` from make_footprint's threshold.  That relaxation covers the float32
rounding of the per-pixel evaluation, i.e. exactly the pairs the oracle calls BAND; MUST keeps d = 1e-6 (1 + mag) away from the
threshold, several times that rounding, so a model without the relaxation still keeps every MUST pair (tried on these cases and
on 8 000 random needles whose tips end inside the image: none missed)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import footprint_oracle as fo                                                 # noqa: E402
import _footprint_dump as fd                                                  # noqa: E402
from oracle import raster_oracle as ro                                        # noqa: E402

f32 = np.float32
CASE_NAMES = ('avatar', 'scene', 'needles', 'tangent_sweep', 'threshold_opacity', 'far_centres', 'one_huge')


def cpu_records(sc, H, W, shrink=1.0):
    """The Splat records of scene ``sc`` as preprocess_fwd.hip writes them: raster_oracle.preprocess in float32, then the
    sub-tile rect and the pre-scaled conic of the kernel, operation by operation in float32.  (``shrink`` scales the half
    extents of the rect: 1 is the kernel's formula.)"""
    job = fd._job(sc, H, W, 'cpu', False)
    s = ro.OracleSettings(*job['raster_settings'])
    with torch.no_grad():
        pre = ro.preprocess(job['means3D'], None, job['opacities'], job['scales'], job['rotations'], None, s, torch.float32)
    n = lambda t: t.numpy()                                                                # noqa: E731
    px, py, op = n(pre['px']), n(pre['py']), n(job['opacities'])[:, 0]
    ca2, cc2 = n(pre['cov2'][0]), n(pre['cov2'][2])
    conic, vis, radius = n(pre['conic']), n(pre['visible']), n(pre['radius'])
    tx0, ty0, tx1, ty1 = (n(v) for v in pre['rect'])
    g = fo.grid(H, W)
    with np.errstate(all='ignore'):
        o255 = f32(255.0) * op
        tau2 = f32(2.0) * np.log(o255) + f32(1e-3)
        ex = np.sqrt(tau2 * ca2) * f32(1.001) * f32(shrink) + f32(0.01)
        ey = np.sqrt(tau2 * cc2) * f32(1.001) * f32(shrink) + f32(0.01)
        lim = f32(1.0e6)
        cl = lambda v: np.nan_to_num(np.minimum(np.maximum(v, -lim), lim), nan=-1.0e6)     # noqa: E731  (fminf(fmaxf(NaN, -lim), lim) = -lim)
        bx0, bx1 = np.floor(cl(px - ex)).astype(np.int64), np.ceil(cl(px + ex)).astype(np.int64)
        by0, by1 = np.floor(cl(py - ey)).astype(np.int64), np.ceil(cl(py + ey)).astype(np.int64)
    sx0, sx1 = np.maximum(2 * tx0, bx0 // 8), np.minimum(np.minimum(2 * tx1, g['sx']), bx1 // 8 + 1)
    sy0, sy1 = np.maximum(2 * ty0, by0 // 8), np.minimum(np.minimum(2 * ty1, g['sy']), by1 // 8 + 1)
    live = vis & (o255 >= 1.0) & (sx1 > sx0) & (sy1 > sy0)
    sx0, sx1, sy0, sy1 = (np.where(live, v, 0) for v in (sx0, sx1, sy0, sy1))
    LOG2E = f32(1.4426950408889634)
    rec = fo.pack(px, py, radius, (f32(-0.5) * LOG2E) * conic[:, 0], -LOG2E * conic[:, 1], (f32(-0.5) * LOG2E) * conic[:, 2], op,
                  sx0, sx1, sy0, sy1, depth=n(pre['depth']))
    rec[~vis] = 0
    return rec


@pytest.fixture(scope='module')
def judged():
    """name -> (records, classes, model mask over the rect pairs): computed once, shared, never modified."""
    out = {}
    for name, ((H, W), sc, _) in fd.CASES.items():
        rec = cpu_records(sc, H, W)
        out[name] = (rec, fo.classify(rec, H, W), fo.model_mask(rec, H, W), (H, W))
    return out


def test_the_cases_are_the_ones_judged():
    assert tuple(fd.CASES) == CASE_NAMES
    for name, ((H, W), sc, _) in fd.CASES.items():
        assert len(sc['z']) <= 2500, name


@pytest.mark.parametrize('case', CASE_NAMES)
def test_must_lies_inside_the_rect(judged, case):
    rec, cl, _, _ = judged[case]
    out = ~cl['in_rect'] & (cl['cls'] == fo.MUST)
    assert not out.any(), [(int(cl['g'][i]), int(cl['sx'][i]), int(cl['sy'][i])) for i in np.flatnonzero(out)[:5]]


def _kept(rec, H, W, mask):
    g, sx, sy = fo.rect_pairs(rec, H, W)
    return fo.pair_key(g, sx, sy, H, W)[mask]


@pytest.mark.parametrize('case', CASE_NAMES)
def test_the_model_lies_between_must_and_must_not(judged, case):
    """The assertions the GPU test applies to the device's lists, applied to the model's."""
    rec, cl, model, (H, W) = judged[case]
    assert cl['in_rect'].sum() == len(model) == fo.unpack(rec)['n_inst'].sum()
    kept = _kept(rec, H, W, model)
    fo.assert_nothing_reached_is_missing(cl, kept)
    fo.assert_no_unreachable_pair_is_listed(cl, kept)


# Deliberately broken models: each has to trip the assertion named with it in at least one case, or the GPU test could not see
# the same mistake in the kernel.  (text of model_cell_masks -> replacement)
MUTANTS = {
    'lo_subtracts_SUB_instead_of_SUB_minus_1': ('unreachable', [('(xa - m - f32(SUB - 1) - e(xl0))', '(xa - m - f32(SUB) - e(xl0))')]),
    'ceil_and_floor_swapped': ('unreachable', [('np.ceil(np.where(ordered, lo, 0))', 'np.floor(np.where(ordered, lo, 0))'),
                                               ('np.floor(np.where(ordered, hi, 0))', 'np.ceil(np.where(ordered, hi, 0))')]),
    'ysr_with_the_wrong_sign': ('missing', [('yR, yL = _clampf(e(ysr), yl, yh), _clampf(-e(ysr), yl, yh)',
                                             'yR, yL = _clampf(-e(ysr), yl, yh), _clampf(e(ysr), yl, yh)')]),
}


def _mutant(edits):
    src = open(fo.__file__).read()
    for old, new in edits:
        assert src.count(old) == 1, old
        src = src.replace(old, new)
    ns = {'__name__': 'footprint_oracle_mutant'}
    exec(compile(src, fo.__file__, 'exec'), ns)
    return ns['model_mask']


def _trips(check, cl, kept):
    try:
        check(cl, kept)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize('name', sorted(MUTANTS))
def test_a_broken_model_is_caught(judged, name):
    which, edits = MUTANTS[name]
    check = {'missing': fo.assert_nothing_reached_is_missing, 'unreachable': fo.assert_no_unreachable_pair_is_listed}[which]
    mask = _mutant(edits)
    caught = [case for case, (rec, cl, _, (H, W)) in judged.items() if _trips(check, cl, _kept(rec, H, W, mask(rec, H, W)))]
    assert caught, name


def test_the_whole_rect_is_caught(judged):
    """rows_mask returning the whole rect: every case lists unreachable pairs."""
    for case, (rec, cl, model, (H, W)) in judged.items():
        assert _trips(fo.assert_no_unreachable_pair_is_listed, cl, _kept(rec, H, W, np.ones_like(model))), case


def test_a_rect_shrunk_by_two_percent_is_caught():
    """ex, ey of the sub-tile rect times 0.98: with the footprint test off (the lists are the rects) a reached pair is missing."""
    (H, W), sc, _ = fd.CASES['scene']
    rec = cpu_records(sc, H, W, shrink=0.98)
    cl = fo.classify(rec, H, W)
    assert (~cl['in_rect'] & (cl['cls'] == fo.MUST)).any()
    assert _trips(fo.assert_nothing_reached_is_missing, cl, _kept(rec, H, W, fo.model_mask(rec, H, W, footprint=False)))


@pytest.mark.parametrize('case', CASE_NAMES)
def test_the_case_has_teeth(judged, case):
    rec, cl, _, _ = judged[case]
    fd.assert_case_has_teeth(case, cl, rec)


def test_without_the_footprint_test_the_model_keeps_the_rect(judged):
    rec, _, _, (H, W) = judged['scene']
    assert fo.model_mask(rec, H, W, footprint=False).all()


def test_known_pairs_of_one_round_splat():
    """One isotropic splat, sigma^2 = 4 (conic 1/4), opacity 1, centred in sub-tile (2, 2) of a 64 x 64 image with a rect of
    5 x 5 sub-tiles: alpha >= 1/255 out to r = 2 sqrt(2 ln 255) = 6.66 px.  By hand: the centre sub-tile and its four edge
    neighbours are reached (pixel distance 4.5 along an axis); the diagonal neighbours' nearest pixel centre is 4.5 sqrt 2 =
    6.36 px away: reached; every sub-tile of the outer ring is at least 8 + 4.5 px away: never."""
    A = f32(-0.5 * 1.4426950408889634 / 4.0)
    rec = fo.pack([f32(19.5)], [f32(19.5)], [40], [A], [f32(0)], [A], [f32(1)], [0], [5], [0], [5])
    cl = fo.classify(rec, 64, 64)
    near = (np.abs(cl['sx'] - 2) <= 1) & (np.abs(cl['sy'] - 2) <= 1)
    assert cl['in_rect'].sum() == 25 and (cl['cls'][near] == fo.MUST).all() and near.sum() == 9
    assert (cl['cls'][cl['in_rect'] & ~near] == fo.MUST_NOT).all()
    assert fo.model_mask(rec, 64, 64).sum() == 9
