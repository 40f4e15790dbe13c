"""CPU tests of the posed SMPL-X stage's restatement (tests/posed_oracle.py) against the reference's own run
(tests/golden/ref_posed.npz, written by tests/golden/make_golden_posed.py): the float64 run agrees with it to rounding,
the float32 run stays within what the reference's own float32 arithmetic loses, and the hand-written backward of
Rodrigues' formula is the derivative of its forward."""
import os
import types

import numpy as np
import pytest

import posed_oracle as po

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_posed.npz')
NAMES = po.OUTPUTS + ('rot',) + tuple('grad_' + k for k in po.INPUTS)


@pytest.fixture(scope='module')
def golden():
    case, inputs, cot = po.golden_inputs()
    return types.SimpleNamespace(case=case, inputs=inputs, cot=cot, ref=dict(np.load(GOLDEN)))


def _oracle(g, dtype):
    i = g.inputs
    Rinv = np.linalg.inv(i['R'].astype(np.float64)).astype(dtype)
    fwd = po.forward(g.case, i['pose'], i['betas'], i['expression'], i['transl'], i['joint_offset'], Rinv, i['t'], dtype)
    grads = po.backward(g.case, i['pose'], fwd, g.cot, Rinv, dtype, n_betas=po.GOLDEN_BETAS)
    res = {k: fwd[k] for k in po.OUTPUTS + ('rot',)}
    res.update({'grad_' + k: v for k, v in grads.items()})
    return res


def test_the_fixture_was_made_from_these_inputs(golden):
    want = dict(zip(golden.ref['digest_names'].tolist(), golden.ref['digest_values'].tolist()))
    assert po.golden_digests(golden.case, golden.inputs, golden.cot) == want
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert sorted(k for k in golden.ref if k.startswith('ref_f32_err/')) == sorted('ref_f32_err/' + k for k in NAMES)
    # the pose holds what the GPU tests name: exact zero rows for both eyes, one angle within 1e-3 of pi
    full = golden.inputs['pose'].astype(np.float64) + golden.case['pose_mean']
    assert not full[23].any() and not full[24].any()
    assert abs(np.linalg.norm(full[22]) - np.pi) < 1e-3


def test_float64_oracle_agrees_with_the_reference_to_rounding(golden):
    """Both sides evaluate the same expression in float64 in different orders.  ``ref_f32_err`` is what the reference's
    order loses at u = 2^-24; rounding errors are linear in u, so at u = 2^-53 it loses 2^-29 of that, and the oracle's
    order as much within the project's factor 4 for a different but fixed order: 8 * 2^-29 * ref_f32_err in all."""
    got = _oracle(golden, np.float64)
    for k in NAMES:
        assert got[k].shape == golden.ref[k].shape and got[k].dtype == np.float64, k
        err = np.abs(got[k] - golden.ref[k]).max()
        bound = 8 * 2.0 ** -29 * float(golden.ref['ref_f32_err/' + k])
        print(k, 'max |oracle64 - reference|', err, 'bound', bound)
        assert err <= bound, k


def test_float32_oracle_is_within_the_references_own_float32_error(golden):
    """The bit-exactness oracle against the golden: 4 * ref_f32_err, the bound the GPU test applies to the device."""
    got = _oracle(golden, np.float32)
    for k in NAMES:
        assert got[k].dtype == np.float32, k
        err = np.abs(got[k].astype(np.float64) - golden.ref[k]).max()
        bound = 4 * float(golden.ref['ref_f32_err/' + k])
        print(k, 'max |oracle32 - reference|', err, 'bound', bound, 'ratio', err / bound * 4)
        assert np.isfinite(got[k]).all() and err <= bound, k


def test_rodrigues_backward_is_the_derivative_of_its_forward():
    """Central differences in float64 over a zero row, a row near pi and random rows, with and without a pose_mean:
    the step's truncation is h^2 |f'''| / 6 ~ 1e-10 at h = 1e-5 and its rounding u64 / h ~ 1e-11; 1e-8 holds both."""
    rng = np.random.RandomState(5)
    pose = 0.7 * rng.standard_normal((6, 3))
    pose[0] = 0
    pose[1] *= (np.pi - 5e-4) / np.linalg.norm(pose[1])
    G = rng.standard_normal((6, 3, 3))
    for mean in (None, np.concatenate([np.zeros((2, 3)), 0.1 * rng.standard_normal((4, 3))])):
        rot, sc = po.rodrigues(pose, mean, np.float64)
        got = po.rodrigues_backward(pose, mean, G, sc, np.float64)
        assert np.isfinite(got).all()
        h = 1e-5
        for j in range(6):
            for k in range(3):
                d = np.zeros_like(pose)
                d[j, k] = h
                num = ((po.rodrigues(pose + d, mean, np.float64)[0] - po.rodrigues(pose - d, mean, np.float64)[0]) * G).sum() / (2 * h)
                assert abs(num - got[j, k]) <= 1e-8 * max(1.0, abs(num)), (j, k, num, got[j, k])
        # orthonormal to rounding away from the epsilon's own effect (f / |f + 1e-8| is a unit vector to 1e-8)
        assert np.abs(rot @ np.swapaxes(rot, 1, 2) - np.eye(3)).max() < 1e-7


def test_missing_cotangents_and_options_change_what_they_should(golden):
    """No camera: no world output; a missing cotangent contributes nothing (the gradients add up over the patterns in
    float64); J == 1 has no pose correctives."""
    i, case = golden.inputs, golden.case
    Rinv = np.linalg.inv(i['R'].astype(np.float64))
    fwd = po.forward(case, i['pose'], i['betas'], i['expression'], i['transl'], i['joint_offset'], Rinv, i['t'], np.float64)
    assert po.forward(case, i['pose'], i['betas'], i['expression'], i['transl'], None, None, None, np.float64)['vertices_world'] is None
    full = po.backward(case, i['pose'], fwd, golden.cot, Rinv, np.float64, n_betas=po.GOLDEN_BETAS)
    parts = [po.backward(case, i['pose'], fwd, {k: golden.cot[k] if k == only else None for k in po.OUTPUTS}, Rinv,
                         np.float64, n_betas=po.GOLDEN_BETAS) for only in po.OUTPUTS]
    for k in po.INPUTS:
        total = sum(p[k] for p in parts if p[k] is not None)
        assert np.abs(total - full[k]).max() <= 1e-12 * max(1.0, np.abs(full[k]).max()), k
    assert np.abs(parts[1]['transl'] - golden.cot['joints'].astype(np.float64).sum(0)).max() <= 1e-12      # 55 terms
    import body_oracle as bo
    verts, faces = bo.grid(3, 4)
    one = po.random_case(verts, faces, 3, [-1], 3)
    x = po.random_inputs(one, 2, 4, camera=False)
    f1 = po.forward(one, x['pose'], x['betas'], x['expression'], x['transl'], x['joint_offset'])
    assert f1['v_posed'] is f1['v_shaped'] and one['posedirs'].shape == (0, 36)
