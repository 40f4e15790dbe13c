"""The sub-tile lists against the per-pixel alpha rule (tests/footprint_oracle.py, float64).

Every other binning test compares two paths of the same library that share one rows_mask body and one rect, so an error in the
footprint arithmetic (csrc/common.h make_footprint / footprint_band, csrc/binning.hip rows_mask), in a relaxation or in the
sub-tile rect of csrc/preprocess_fwd.hip is identical on both sides.  Here the rule the design assumes -- a sub-tile is dropped
only if none of its 64 pixel centres passes alpha >= 1/255 -- judges the lists themselves, on the records the kernels read:

  * every pair the rule reaches (MUST) is listed -- multi-part path, one-workgroup-per-cell path, and with the footprint test
    off (which tests the rect alone);
  * with the footprint test off the lists are exactly the rects;
  * with it on, no pair that twice the documented relaxations cannot reach (MUST_NOT) is listed;
  * the lists are well-formed, and the two footprint-on paths leave identical ranges and ids.

tests/_footprint_dump.py renders the cases in three fresh child processes (default, EXA_BIN_SINGLE_CELLS=1, EXA_FOOTPRINT=0),
exact and capacity mode each.  Per-case counts are appended to profiles/footprint_lists.md."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import footprint_oracle as fo                                                 # noqa: E402

CASE_NAMES = ('avatar', 'scene', 'needles', 'tangent_sweep', 'threshold_opacity', 'far_centres', 'one_huge')
VARIANTS = (('parts', {}), ('single', {'EXA_BIN_SINGLE_CELLS': '1'}), ('rect', {'EXA_FOOTPRINT': '0'}))
MODES = ('exact', 'capacity')
REPORT = {}                 # case -> counts; written once, when the module's tests are over


# ---- the device's lists ----

@pytest.fixture(scope='module')
def dumps(tmp_path_factory):
    """variant -> arrays of tests/_footprint_dump.py: three fresh child processes, one after the other, each under its own time
    limit; shared by all tests, never modified."""
    d = tmp_path_factory.mktemp('footprint_lists')
    out = {}
    base = {k: v for k, v in os.environ.items() if k not in ('EXA_BIN_SINGLE_CELLS', 'EXA_FOOTPRINT')}
    for name, env in VARIANTS:
        path = str(d / (name + '.npz'))
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_footprint_dump.py'), path], cwd=ROOT,
                           env=dict(base, **env), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        out[name] = dict(np.load(path))
    return out


@pytest.fixture(scope='module')
def judged(dumps):
    """case -> (records, classes, (H, W)): the oracle's classes of the records the DEVICE left (default path, exact mode)."""
    import _footprint_dump as fd
    out = {}
    for case, ((H, W), _, _) in fd.CASES.items():
        rec = dumps['parts'][case + '__exact__records']
        out[case] = (rec, fo.classify(rec, H, W), (H, W))
    return out


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    if not REPORT:
        return
    cols = ('rect', 'MUST', 'BAND', 'MAY', 'MUST_NOT') + tuple('listed ' + v for v, _ in VARIANTS) + ('device != model',)
    lines = ['', '## %s' % time.strftime('%Y-%m-%d %H:%M:%S'), '',
             '| case | ' + ' | '.join(cols) + ' |', '|---|' + '---:|' * len(cols)]
    for case in CASE_NAMES:
        if case in REPORT:
            lines.append('| %s | ' % case + ' | '.join(str(REPORT[case].get(c, '')) for c in cols) + ' |')
    with open(os.path.join(ROOT, 'profiles', 'footprint_lists.md'), 'a') as f:
        f.write('\n'.join(lines) + '\n')


def _key(dumps, variant, case, mode, H, W):
    tag = '%s__%s__' % (case, mode)
    return fo.pair_key(*fo.listed_pairs(dumps[variant][tag + 'ranges'], dumps[variant][tag + 'ids'], H, W), H, W)


def test_the_cases_are_the_ones_rendered():
    import _footprint_dump as fd
    assert tuple(fd.CASES) == CASE_NAMES and fd.MODES == MODES


@pytest.mark.parametrize('case', CASE_NAMES)
def test_every_run_judges_the_same_records(dumps, judged, case):
    """The classes are built once per case; every variant and mode left the same records (all but the instance offset)."""
    rec = judged[case][0]
    for variant, _ in VARIANTS:
        for mode in MODES:
            assert np.array_equal(dumps[variant]['%s__%s__records' % (case, mode)][:, :15], rec[:, :15]), (variant, mode)


@pytest.mark.parametrize('case', CASE_NAMES)
def test_the_case_has_teeth(judged, case):
    import _footprint_dump as fd
    rec, cl, _ = judged[case]
    fd.assert_case_has_teeth(case, cl, rec)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('variant', [v for v, _ in VARIANTS])
@pytest.mark.parametrize('case', CASE_NAMES)
def test_lists_are_well_formed_and_miss_nothing_reached(dumps, judged, case, variant, mode):
    rec, cl, (H, W) = judged[case]
    tag = '%s__%s__' % (case, mode)
    d = dumps[variant]
    key = fo.assert_well_formed(rec, d[tag + 'ranges'], d[tag + 'ids'], int(d[tag + 'capacity']), H, W)
    fo.assert_nothing_reached_is_missing(cl, key)
    if variant == 'rect':
        fo.assert_lists_are_the_rects(rec, key, H, W)
    else:
        fo.assert_no_unreachable_pair_is_listed(cl, key)
    if mode == 'exact':
        REPORT.setdefault(case, dict(fo.counts(cl)))['listed ' + variant] = len(key)
        if variant == 'parts':
            g, sx, sy = fo.rect_pairs(rec, H, W)
            model = fo.pair_key(g, sx, sy, H, W)[fo.model_mask(rec, H, W)]
            REPORT[case]['device != model'] = len(np.setxor1d(model, key))            # reported, not asserted (MAY pairs)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', CASE_NAMES)
def test_the_two_footprint_paths_leave_the_same_lists(dumps, case, mode):
    tag = '%s__%s__' % (case, mode)
    for k in ('ranges', 'ids', 'capacity'):
        assert np.array_equal(dumps['parts'][tag + k], dumps['single'][tag + k]), k


@pytest.mark.parametrize('case', CASE_NAMES)
def test_both_modes_list_the_same_pairs(dumps, judged, case):
    _, _, (H, W) = judged[case]
    for variant, _ in VARIANTS:
        assert np.array_equal(np.sort(_key(dumps, variant, case, 'exact', H, W)), np.sort(_key(dumps, variant, case, 'capacity', H, W))), variant
