"""The small case of the composed loss-block tests (``tests/loss_case.py``) and its fixtures
(``tests/golden/ref_lossblock_w0.npz`` / ``_w1.npz``, written by ``tests/golden/make_golden_lossblock.py`` from the
reference's own training branch of ``Model.forward``): the inputs rebuilt here are the ones the fixtures were generated
from, they keep the distances from every decision that the GPU comparison rests on, and -- where a checkout of the
reference is at hand (at ``REFERENCE``, or where ``EXAVATAR_REFERENCE`` points) -- the generator's float64 run
reproduces the fixtures."""
import importlib.util
import os

import numpy as np
import pytest

from tests import loss_case as lc

REFERENCE = '/root/reference'      # where the other generators of tests/golden read it; EXAVATAR_REFERENCE overrides


@pytest.fixture(scope='module')
def golden(golden_dir):
    return {w: np.load(os.path.join(golden_dir, 'ref_lossblock_w%d.npz' % w)) for w in (0, 1)}


@pytest.fixture(scope='module')
def measured():
    return lc.margins(lc.build_case())


def test_the_case_rebuilds_the_inputs_the_fixtures_were_generated_from(golden):
    got = lc.digests(lc.build_case())
    for g in golden.values():
        want = {k[len('sha256/'):]: str(g[k]) for k in g.files if k.startswith('sha256/')}
        assert sorted(got) == sorted(want)
        assert [k for k in got if got[k] != want[k]] == []


def test_each_fixture_file_is_under_one_mebibyte(golden_dir):
    for w in (0, 1):
        assert os.path.getsize(os.path.join(golden_dir, 'ref_lossblock_w%d.npz' % w)) < (1 << 20)


def test_the_case_has_the_sizes_and_paths_the_modules_need():
    c = lc.build_case()
    assert c['mesh_neutral_pose'].shape == (3202, 3) and c['face_upsampled'].shape == (6400, 3)
    assert c['face_upsampled'].min() == 0 and c['face_upsampled'].max() == lc.V - 1
    assert all(not a.flags.writeable for a in c.values())
    degree = np.bincount(np.unique(np.sort(np.concatenate([c['face_upsampled'][:, [0, 1]], c['face_upsampled'][:, [1, 2]],
                                                           c['face_upsampled'][:, [2, 0]]]), 1), axis=0).reshape(-1))
    assert degree[lc.POLE_R] == degree[lc.POLE_L] == 20 and degree[:lc.POLE_R].max() == 6      # the poles are truncated at 10
    assert int(c['is_rhand'].sum()) == int(c['is_lhand'].sum()) == 301 > 256                  # more than one chunk of rows
    assert c['is_rhand'][lc.POLE_R] and c['is_lhand'][lc.POLE_L] and not (c['is_rhand'] & c['is_lhand']).any()
    assert int(c['is_face'].sum()) == 400 and int(c['is_face_expr'].sum()) == 180 and int(c['is_cavity'].sum()) == 30
    assert not (c['is_face_expr'] & ~c['is_face']).any() and not (c['is_cavity'] & ~c['is_face_expr']).any()
    assert (c['mesh_neutral_pose'][c['is_face_expr'], 2] > 0).all()
    Wt = c['skinning_weight']
    assert Wt.shape == (lc.V, 55) and ((Wt != 0).sum(1) <= 4).all() and np.allclose(Wt.sum(1), 1, atol=1e-6)
    label, ring = Wt.argmax(1), lc.ring_of()
    top2 = np.sort(Wt, 1)[:, -2:]
    assert (top2[:, 1] > top2[:, 0]).all()                                                    # a strict argmax
    on_arm = np.zeros(lc.V, dtype=bool)
    for name, (r0, r1) in lc.ARM_RINGS.items():
        rows = (ring >= r0) & (ring < r1)
        assert (label[rows] == lc.JOINTS_NAME.index(name)).all(), name
        on_arm |= rows
    assert not np.isin(label[~on_arm], [lc.JOINTS_NAME.index(n) for n in lc.ARM_JOINTS]).any()
    assert len(lc.JOINTS_NAME) == 55 == len(set(lc.JOINTS_NAME))
    rights = [n for n in lc.JOINTS_NAME if n[:2] == 'R_']
    assert len(rights) == 24 and all('L_' + n[2:] in lc.JOINTS_NAME for n in rights)
    assert [lc.JOINTS_NAME[j] for j in (lc.JOINT_PART['lhand'][0], lc.JOINT_PART['rhand'][-1])] == ['L_Index_1', 'R_Thumb_3']
    for k in lc.RENDERS + ('img',):
        assert c[k].shape == (lc.B, 3, lc.H, lc.W) and 0 < c[k].min() and c[k].max() < 1, k
    m = c['mask']
    assert m.shape == (lc.B, 1, lc.H, lc.W) and (m == 0).any() and (m == 1).any() and ((m > 0) & (m < 1)).any()
    for k in ('face', 'face_refined'):
        rgb, a = c[k], c[k + '_alpha']
        inside = rgb != -1
        assert ((rgb == -1) | ((rgb > 0) & (rgb < 1))).all() and set(np.unique(a)) == {0.0, 0.5, 1.0}
        assert (inside & (a == 0.5)).any() and (~inside & (a == 1)).any() and (inside & (a == 1)).any()   # both factors decide
        assert (inside.any(1) & ~inside.all(1)).any()                                           # and per channel
    # the reference's clamp of the bbox: both clamps fire and the right edge is inside the image
    xmin, ymin, w, h = (int(v) for v in c['bbox'][0])
    x0, y0 = max(xmin, 0), max(ymin, 0)
    assert (x0, y0, min(x0 + w, lc.W) - x0, min(y0 + h, lc.H) - y0) == lc.CROP
    assert xmin < 0 and y0 + h > lc.H and x0 + w < lc.W and y0 > 0


def test_the_case_keeps_its_distance_from_every_decision(golden, measured):
    lc.check_margins(measured)
    assert measured['arm/normal_margin'] > 0.03 and measured['arm/dx_margin'] > 1e-3 and measured['arm/kth_gap'] > 1e-5
    for g in golden.values():
        for k, v in measured.items():
            assert abs(float(g['margin/' + k]) - v) <= 1e-9 * max(abs(v), 1e-30) + 1e-15, k


def test_k_and_the_arm_sizes_are_as_recorded(golden, measured):
    for g in golden.values():
        up, lo = g['arm/is_upper'], g['arm/is_lower']
        assert (int(up.sum()), int(lo.sum()), int(g['arm/k'])) == (lc.U_ARM, lc.L_ARM, lc.K_ARM) == (420, 780, 21)
        assert (int(g['arm/n_valid'].min()), int(g['arm/n_valid'].max())) == lc.N_VALID == (21, 35)
        assert g['arm/n_valid'].shape == (lc.L_ARM,)
        got = lc.arm_masks(lc.build_case(), lc.normals64(lc.build_case()))
        assert np.array_equal(got[0], up) and np.array_equal(got[1], lo)
    assert (measured['arm/U'], measured['arm/L'], measured['arm/k']) == (420, 780, 21)


def test_the_fixture_stores_every_leaf_and_every_term(golden):
    for g in golden.values():
        assert [str(s) for s in g['unreached']] == ['rgb_offset']
        for k in lc.LEAVES:
            if k == 'rgb_offset':
                continue
            idx = lc.sample_index(k, lc.build_case()[k].shape)
            n = lc.build_case()[k].size if idx is None else len(idx)
            assert g['grad/' + k].shape == (n,) or idx is None, k
            assert all('grad/%s#%s' % (k, s) in g.files for s in ('norm', 'rel_l2', 'rel_max')), k
        for k in lc.DROPIN_TERMS:
            assert all(('term/' + k + s) in g.files for s in ('', '#f32', '#elem')), k
            assert abs(float(g['term/%s#f32' % k]) - float(g['term/' + k])) <= lc.FACTOR * lc.term_scale(g, 'dropin', k)
        assert abs(sum(float(g['term/' + k]) for k in lc.DROPIN_TERMS) - float(g['total'])) <= 1e-12 * float(g['total'])
    # the band: every pixel within six of the crop's inner edges is stored
    idx = set(lc.sample_index('human', (lc.B, 3, lc.H, lc.W)).tolist())
    flat = lambda b, c, y, x: ((b * 3 + c) * lc.H + y) * lc.W + x      # noqa: E731
    assert all(flat(1, 2, y, x) in idx for y in (1, 7, 12) for x in range(lc.W))
    assert all(flat(0, 1, y, x) in idx for x in (54, 60, 65) for y in range(lc.H))
    assert len(idx) < 0.5 * lc.B * 3 * lc.H * lc.W


def test_the_generator_reproduces_the_fixtures_from_the_reference(golden, golden_dir):
    ref = os.environ.get('EXAVATAR_REFERENCE', REFERENCE)
    if not os.path.exists(os.path.join(ref, 'avatar', 'main', 'model.py')):
        pytest.skip('no checkout of the reference at %s' % ref)
    spec = importlib.util.spec_from_file_location('make_golden_lossblock', os.path.join(golden_dir, 'make_golden_lossblock.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for w, g in golden.items():
        out = gen.record(ref, bool(w), with_float32=False)
        assert sorted(out) == sorted(k for k in g.files if not k.endswith(('#rel_l2', '#rel_max', '#f32')))
        for k, a in out.items():
            b = g[k]
            if a.dtype.kind in 'USbiu':
                assert np.array_equal(a, b), k
                continue
            scale = float(g[k + '#norm']) if k + '#norm' in g.files else float(np.abs(b).max())
            assert a.shape == b.shape and np.abs(a.astype(np.float64) - b).max() <= 1e-12 * max(scale, 1e-300), k
