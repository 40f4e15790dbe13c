"""The small avatar of the composed-forward tests (``tests/human_case.py``) and its fixture
(``tests/golden/ref_human.npz``, written by ``tests/golden/make_golden_human.py`` from the reference's own
``HumanGaussian.forward``): the inputs rebuilt here are the ones the fixture was generated from, they meet the conditions
the GPU comparison rests on, and -- where a checkout of the reference is at hand (at ``REFERENCE``, or where
``EXAVATAR_REFERENCE`` points) -- the generator's float64 run reproduces the fixture."""
import importlib.util
import os

import numpy as np
import pytest

from tests import human_case as hc

REFERENCE = '/root/reference'      # where the other generators of tests/golden read it; EXAVATAR_REFERENCE overrides


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'ref_human.npz'))


def test_the_case_rebuilds_the_inputs_the_fixture_was_generated_from(golden):
    case = hc.build_case()
    want = {k[len('sha256/'):]: str(golden[k]) for k in golden.files if k.startswith('sha256/')}
    got = hc.digests(case)
    assert sorted(got) == sorted(want)
    assert [k for k in got if got[k] != want[k]] == []


def test_the_case_has_the_sizes_and_paths_the_modules_need():
    c = hc.build_case()
    assert c['mesh_lr'].shape == (162, 3) and c['mesh_neutral_pose'].shape == (2562, 3)
    assert c['face_upsampled'].shape == (5120, 3) and c['face_upsampled'].min() == 0 and c['face_upsampled'].max() == 2561
    assert hc.V % 512 == 2 and hc.V % 256 == 2                     # a two-row last MLP chunk, a two-vertex skinning chunk
    pose_mask = c['is_rhand'] | c['is_lhand'] | c['is_face_expr']
    assert 3 * int(pose_mask.sum()) > 1024                          # more than one blend chunk of compact columns
    for k in ('is_rhand', 'is_lhand', 'is_face', 'is_face_expr', 'is_cavity'):
        assert c[k].dtype == np.bool_ and 0 < int(c[k].sum()) < hc.V, k
    assert not (c['is_face_expr'] & ~c['is_face']).any()
    expr_rows = (c['expr_dirs'] != 0).reshape(hc.V, -1).any(1)
    assert np.array_equal(expr_rows, c['is_face_expr'])              # non-zero only, and everywhere, on is_face_expr
    assert not c['leye_pose'].any() and not c['reye_pose'].any()
    assert all(np.abs(c[k]).min() > 0 for k in hc.POSE_LEAVES)
    W = c['skinning_weight']
    assert ((W != 0).sum(1) <= 4).all() and ((W != 0).sum(1) >= 1).all() and np.allclose(W.sum(1), 1, atol=1e-6)
    T = c['transform_mat_neutral_pose'].astype(np.float64)
    R = T[:, :3, :3]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6 and np.allclose(np.linalg.det(R), 1, atol=1e-6)
    assert np.array_equal(T[:, 3], np.tile([0, 0, 0, 1.0], (hc.J, 1)))
    assert np.abs(R - np.eye(3)).reshape(hc.J, -1).max(1).min() > 1e-3 and np.abs(T[:, :3, 3]).max(1).min() > 1e-4
    Rc = c['cam_R'].astype(np.float64)
    assert np.abs(Rc @ Rc.T - np.eye(3)).max() < 1e-6 and np.abs(Rc - np.eye(3)).max() > 0.05
    for name, (dims, _, _) in hc.NETS.items():                       # module.py:279-287
        first = c['%s.0.weight' % name]
        assert first.shape == (dims[1], dims[0])
    assert all(a.dtype in (np.float32, np.bool_, np.int64) for a in c.values())


def test_some_face_rows_sample_the_zero_padding():
    c = hc.build_case()
    g = hc.face_coords(c)
    outside = (np.abs(g) > 1).any(1)
    assert 0 < int(outside.sum()) < len(g)
    body = c['pos_enc_mesh'].astype(np.float64)
    body = (body - body.mean(0)) / (np.asarray(hc.TRIPLANE_SHAPE_3D) / 2)
    assert np.abs(body).max() < 1


def test_the_nearest_vertex_is_a_discrete_fact(golden):
    """For every vertex outside the hand / face mask the float64 gap between the nearest and the second-nearest
    low-resolution vertex is at least 1e-4 relative, so float32 evaluations in any order pick the same one."""
    c = hc.build_case()
    gaps, idx = hc.knn_gaps(c, golden['knn/mean_offset_f32'])
    assert gaps.min() >= hc.KNN_GAP
    assert abs(gaps.min() - float(golden['knn/min_gap'])) < 1e-6
    assert np.array_equal(idx, golden['nn_vertex_idxs'])
    mask = hc.hand_face_mask(c)
    assert (idx[~mask] < hc.V_LR).all() and len(np.unique(idx[~mask])) > 50


def test_the_sample_the_fixture_keeps_depends_on_name_and_shape_alone(golden):
    a = np.arange(hc.V * 3, dtype=np.float64).reshape(hc.V, 3)
    s = hc.take_sample('wc0/out/assets/mean_3d', a)
    assert s.shape == (hc.ROW_SAMPLE, 3) == golden['wc0/out/assets/mean_3d'].shape
    assert np.array_equal(s, hc.take_sample('wc0/out/assets/mean_3d', a.copy()))
    assert not np.array_equal(s, hc.take_sample('wc1/out/assets/mean_3d', a))
    assert hc.take_sample('x', np.zeros((128, 96))).shape == (hc.ENTRY_SAMPLE,)
    assert hc.take_sample('x', np.zeros((55, 4, 4))).shape == (55, 4, 4)
    for tag in ('wc0', 'wc1', 'wc0_single'):                      # every leaf is stored or named as unreached
        unreached = set(str(s) for s in golden[tag + '/unreached']) - {''}
        assert {k for k in hc.leaf_names() if '%s/grad/%s' % (tag, k) in golden.files} | unreached == set(hc.leaf_names())
        assert unreached == (set() if tag != 'wc0_single' else {
            k for k in hc.leaf_names() if k.split('.')[0] in ('scale_net', 'scale_offset_net', 'rgb_net', 'rgb_offset_net')})


def test_the_generator_reproduces_the_fixture_from_the_reference(golden, golden_dir):
    ref = os.environ.get('EXAVATAR_REFERENCE', REFERENCE)
    if not os.path.exists(os.path.join(ref, 'avatar', 'common', 'nets', 'module.py')):
        pytest.skip('no checkout of the reference at %s' % ref)
    spec = importlib.util.spec_from_file_location('make_golden_human', os.path.join(golden_dir, 'make_golden_human.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    out = gen.record(ref, with_float32=False)
    values = [k for k in golden.files if '#' not in k]
    assert sorted(out) == sorted(k for k in golden.files if not k.endswith(('#rel_l2', '#rel_max')))
    for k in values:
        a, b = out[k], golden[k]
        if a.dtype.kind in 'US' or a.dtype.kind in 'iu':
            assert np.array_equal(a, b), k
            continue
        assert a.shape == b.shape, k
        scale = float(golden[k + '#norm']) if k + '#norm' in golden.files else float(np.abs(b).max())
        assert np.abs(a.astype(np.float64) - b).max() <= 1e-12 * scale, k
        if k + '#norm' in golden.files:
            assert abs(float(out[k + '#norm']) - scale) <= 1e-12 * scale, k
