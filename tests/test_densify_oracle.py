"""CPU tests of the densification oracle (tests/densify_oracle.py) and of the cases the GPU tests run
(tests/densify_cases.py): the numpy three passes reproduce the topology and every copied row of what the reference itself
returned (tests/golden/ref_densify.npz), the generator reproduces the fixture where the reference is at hand, every row of
the fixture and of every generated case is admissible (no decision within 1e-5 relative of its threshold in float64), and
the class letters mean what tests/densify_cases.py says."""
import importlib.util
import os

import numpy as np
import pytest

from tests import densify_cases as dc
from tests import densify_oracle as do

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'ref_densify.npz')
PARAMS = ('mean', 'feature_dc', 'feature_rest', 'opacity', 'scale', 'rotation')
MOMENTS = ('exp_avg_', 'exp_avg_sq_')
VARIANTS = (('none', None), ('s20', 20))
MARGIN = 1e-5


@pytest.fixture(scope='module')
def fixture():
    return dict(np.load(GOLDEN))


def _oracle(fixture, ssm, child_dtype=np.float32):
    P = {k: fixture['in_' + k] for k in PARAMS}
    S = {m + k: fixture['in_' + m + k] for k in PARAMS for m in MOMENTS}
    return do.three_passes(P, S, fixture['in_xyz_grad_accum'], fixture['in_track_cnt'], float(fixture['in_cam_dist_radius'][0]),
                           fixture['in_noise'], grad_thr=0.0002, dense_percent=0.01, opacity_min=0.005, screen_size_max=ssm,
                           child_dtype=child_dtype)


def test_the_fixture_is_what_the_issue_asks_for(fixture):
    P0 = fixture['in_mean'].shape[0]
    assert 650 <= P0 <= 750
    assert all(fixture['in_' + m + k].all() for k in PARAMS for m in MOMENTS), 'non-zero moments'
    _, _, info = _oracle(fixture, 20)
    assert info['n_keep'] > 0 and info['n_clone'] > 0 and info['n_split'] > 0 and info['n_pruned'] > 0
    assert info['n_cand'] > info['n_split'] and fixture['in_noise'].shape == (2 * info['n_cand'], 3)
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize('tag,ssm', VARIANTS)
def test_every_row_of_the_fixture_is_admissible(fixture, tag, ssm):
    m = do.margins(fixture['in_scale'], fixture['in_opacity'], float(fixture['in_cam_dist_radius'][0]), prune_big=bool(ssm))
    assert m.min() > MARGIN, (int(m.argmin()), float(m.min()))
    g = fixture['in_xyz_grad_accum'] / np.maximum(fixture['in_track_cnt'], 1)
    assert np.abs(g[fixture['in_track_cnt'] > 0] / np.float32(0.0002) - 1).min() > MARGIN


@pytest.mark.parametrize('tag,ssm', VARIANTS)
def test_the_oracle_reproduces_the_fixtures_topology_and_copied_rows(fixture, tag, ssm):
    new, states, info = _oracle(fixture, ssm)
    ref = lambda k: fixture['%s_%s' % (tag, k)]      # noqa: E731
    assert info['n_out'] == int(ref('point_num')[0])
    for k in ('feature_dc', 'feature_rest', 'opacity', 'rotation'):
        assert np.array_equal(new[k].view(np.uint32), ref(k).view(np.uint32)), k
    for k, v in states.items():
        assert np.array_equal(v.view(np.uint32), ref(k).view(np.uint32)), k
    old = info['kind'] < 2
    assert old.sum() == info['n_keep'] + info['n_clone'] and not old[old.sum():].any()
    for k in ('mean', 'scale'):
        assert np.array_equal(new[k][old].view(np.uint32), ref(k)[old].view(np.uint32)), k
        # the children: two float32 evaluations of the same lines, a few ulps apart
        assert np.abs(new[k][~old] - ref(k)[~old]).max() <= 8 * np.finfo(np.float32).eps * np.abs(ref(k)[~old]).max()
    new_states = [states[m + k][info['kind'] > 0] for k in PARAMS for m in MOMENTS]
    assert all(not s.any() and not np.signbit(s).any() for s in new_states), 'new rows start at +0.0'
    for k in ('radius_max', 'xyz_grad_accum', 'track_cnt'):
        assert ref(k).shape[0] == info['n_out'] and not ref(k).any()
    # the row order the single pass writes: originals, clones, copy 0 of every surviving split row, copy 1 ...
    assert np.all(np.diff(info['kind']) >= 0)
    for kd in range(4):
        assert np.all(np.diff(info['source'][info['kind'] == kd]) > 0)
    assert np.array_equal(info['source'][info['kind'] == 2], info['source'][info['kind'] == 3])


@pytest.mark.parametrize('tag,ssm', VARIANTS)
def test_the_float64_children_stay_near_the_references(fixture, tag, ssm):
    new, _, info = _oracle(fixture, ssm, np.float64)
    kids = info['kind'] >= 2
    for k in ('mean', 'scale'):
        assert new[k].dtype == np.float64
        assert np.abs(new[k][kids] - fixture['%s_%s' % (tag, k)][kids]).max() < 1e-5


@pytest.mark.skipif(not os.path.exists('/root/reference/avatar/common/nets/module.py'), reason='the reference checkout is not here')
def test_the_generator_reproduces_the_fixture(fixture):
    spec = importlib.util.spec_from_file_location('make_golden_densify', os.path.join(HERE, 'golden', 'make_golden_densify.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    case = gen.build_case()
    n = fixture['in_noise'].shape[0]
    for k, v in case.items():
        want = fixture['in_' + k]
        assert np.array_equal(v[:n] if k == 'noise' else v, want), k
    for tag, ssm in VARIANTS:
        out = gen.run_reference(case, ssm)
        assert int(out.pop('n_noise')) == n
        for k, v in out.items():
            assert np.array_equal(v, fixture['%s_%s' % (tag, k)]), (tag, k)


@pytest.mark.parametrize('letter', sorted(dc.CLASSES))
def test_a_class_letter_means_what_it_says(letter):
    pattern = letter * 40
    c = dc.build(pattern, seed=ord(letter))
    P = {k: c[k] for k in ('mean', 'scale', 'rotation', 'opacity')}
    _, _, info = do.three_passes(P, {}, c['xyz_grad_accum'], c['track_cnt'], dc.EXTENT, c['noise'], screen_size_max=20, **dc.HYPER)
    assert (info['n_keep'], info['n_clone'], info['n_split'], info['n_cand']) == dc.expected_counts(pattern)
    assert dc.expected_counts(pattern) == tuple(40 * x for x in dc.EXPECT[letter])


@pytest.mark.parametrize('P0,seed', [(n, n) for n in (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 773)] + [(65793, 9)])
def test_every_generated_row_is_admissible(P0, seed):
    c = dc.build(dc.random_pattern(P0, seed), seed)
    m = do.margins(c['scale'], c['opacity'], dc.EXTENT, prune_big=True, **{k: dc.HYPER[k] for k in ('dense_percent', 'opacity_min')})
    assert m.min() > 1e3 * MARGIN
    g = c['xyz_grad_accum'] / c['track_cnt']
    assert np.abs(g / np.float32(dc.HYPER['grad_thr']) - 1).min() > 1e3 * MARGIN


def test_nan_to_num_and_the_divisions_by_zero():
    g = do._grad(np.float32([0, 1, -1, 2]), np.float32([0, 0, 0, 4]))
    assert list(g) == [0.0, np.finfo(np.float32).max, np.finfo(np.float32).min, 0.5]


@pytest.mark.parametrize('P0,seed,screen,keep_radius', [(1025, 1, 20, False), (773, 2, None, False), (700, 3, 20, True)])
def test_the_single_pass_decision_table_gives_the_three_passes_rows(P0, seed, screen, keep_radius):
    """The table csrc/densify.hip classifies by, restated in numpy, orders the rows as the three passes do."""
    c = dc.build(dc.random_pattern(P0, seed), seed)
    P = {k: c[k] for k in ('mean', 'scale', 'rotation', 'opacity')}
    _, _, info = do.three_passes(P, {}, c['xyz_grad_accum'], c['track_cnt'], dc.EXTENT, c['noise'], screen_size_max=screen,
                                 radius_max=c['radius_max'], reference_radius_reset=not keep_radius, **dc.HYPER)
    code = do.codes(c['xyz_grad_accum'], c['track_cnt'], c['scale'], c['opacity'], dc.EXTENT, prune_big=bool(screen),
                    radius_max=c['radius_max'] if keep_radius else None, screen_size_max=screen, **dc.HYPER)
    source, kind, rank = do.single_pass(code)
    assert np.array_equal(source, info['source']) and np.array_equal(kind, info['kind'])
    assert int(((code & do.CAND) != 0).sum()) == info['n_cand']
    pos = {r: k for k, r in enumerate(info['cand_rows'])}
    assert all(rank[i] == pos[source[i]] for i in np.nonzero(kind >= 2)[0])


def test_the_fixtures_rows_follow_from_the_decision_table(fixture):
    for tag, ssm in VARIANTS:
        _, _, info = _oracle(fixture, ssm)
        code = do.codes(fixture['in_xyz_grad_accum'], fixture['in_track_cnt'], fixture['in_scale'], fixture['in_opacity'],
                        float(fixture['in_cam_dist_radius'][0]), grad_thr=0.0002, prune_big=bool(ssm))
        source, kind, _ = do.single_pass(code)
        assert np.array_equal(source, info['source']) and np.array_equal(kind, info['kind']), tag
