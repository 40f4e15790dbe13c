"""CPU tests of tests/scene_oracle.py, the restatement that pins the scene-Gaussian stage: its float64 form equals the
reference's own run (tests/golden/ref_scene.npz) and the autograd of the reference's expression, its float32 form stays
within its own first-order bound of the float64 one, and the rows every implementation has to get right have their known
answers."""
import os

import numpy as np
import pytest
import torch

from tests import scene_oracle as so

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_scene.npz')
OUT = ('opacity', 'scale', 'rotation', 'rgb')


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(GOLDEN))


def _close(a, b, tol):
    """|a - b| <= tol max(1, |b|), elementwise."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.all(np.isfinite(a))
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    assert err.max(initial=0.0) <= tol, err.max()


def test_golden_file_is_small_and_holds_the_special_rows(golden):
    assert os.path.getsize(GOLDEN) < 64 * 1024
    assert golden['rotation'].shape == (12, 6)
    np.testing.assert_array_equal(golden['rotation'][:8], np.asarray(so.SPECIAL_ROWS, np.float64))
    assert (golden['deg3_rgb'] == 0).any() and (golden['deg3_rgb'] > 0).any()


@pytest.mark.parametrize('deg', range(4))
def test_float64_oracle_equals_the_references_run(golden, deg):
    z = golden
    case = {k: z[k] for k in so.PARAMS + so.COTANGENTS + ('R', 't')}
    fwd, bwd = so.run(case, deg, np.float64)
    for name, a in zip(OUT, fwd):
        _close(a, z['deg%d_%s' % (deg, name)], 1e-12)
    for name, a in zip(so.PARAMS, bwd):
        _close(a, z['deg%d_grad_%s' % (deg, name)], 1e-12)


def _autograd(case, deg, dtype=torch.float64):
    """(outputs, gradients) of reference_expression as float64 numpy arrays."""
    t = {k: torch.tensor(np.asarray(v, np.float64), dtype=dtype) for k, v in case.items()}
    params = [t[k].clone().requires_grad_(True) for k in so.PARAMS]
    assets = so.reference_expression(*params, deg, t['R'], t['t'])
    grads = torch.autograd.grad([assets[k] for k in OUT], params, [t[k] for k in so.COTANGENTS], allow_unused=True)
    grads = [torch.zeros_like(p) if g is None else g for g, p in zip(grads, params)]
    return [assets[k].detach().double().numpy() for k in OUT], [g.double().numpy() for g in grads]


@pytest.mark.parametrize('deg,Mr', [(0, 15), (1, 3), (2, 8), (3, 15), (0, 0)])
def test_float64_backward_equals_the_autograd_of_the_reference_expression(deg, Mr):
    case = so.make_case(37, Mr, 100 + deg)
    fwd, bwd = so.run(case, deg, np.float64)
    outs, grads = _autograd(case, deg)
    for a, b in zip(fwd, outs):
        _close(a, b, 1e-12)
    for a, b in zip(bwd, grads):
        _close(a, b, 1e-11)


@pytest.mark.parametrize('deg', range(4))
def test_float32_oracle_is_within_half_its_bound_of_float64(deg):
    case = so.make_case(1500, 15, 200 + deg)
    # rows whose second axis is nearly parallel to the first: the Gram-Schmidt step cancels, the bound carries kappa
    for j, e in enumerate((1e-1, 1e-2, 1e-3, 1e-4)):
        case['rotation'][20 + j, 3:] = (np.float32(1.5) * case['rotation'][20 + j, :3]
                                        + np.float32(e) * case['rotation'][40 + j, :3])
    f64, b64 = so.run(case, deg, np.float64)
    f32, b32 = so.run(case, deg, np.float32, outputs=(f64[0], f64[1]))
    assert all(a.dtype == np.float32 for a in f32[:4] + b32)
    kappa = so.conditioning(case['mean'], case['rotation'], case['R'], case['t'])[0]
    assert kappa[20:24].max() > 1e3
    np.testing.assert_array_equal(f32[3] == 0, f64[3] == 0)      # no channel changes its clamp decision
    bound = so.case_bounds(case, deg)
    pairs = [(f32[2], f64[2]), (f32[3], f64[3]), (b32[0], b64[0]), (b32[3], b64[3]), (b32[4], b64[4]), (b32[5], b64[5])]
    for name, (a, b), bd in zip(('rotation', 'rgb', 'grad mean', 'grad rotation', 'grad dc', 'grad rest'), pairs, bound):
        err = np.abs(a.astype(np.float64) - b)
        assert np.all(np.isfinite(a)), name
        assert np.all(err <= 0.5 * bd), (name, np.nanmax(np.where(err > 0, err / bd, 0.0)))


def test_the_bound_of_the_rotation_gradient_carries_the_conditioning():
    """The same cotangent on a well and on a badly conditioned row: the bound grows with kappa (no flat tolerance)."""
    case = so.make_case(2, 0, 5, special=False)
    a1 = case['rotation'][0, :3]
    case['rotation'][1, :3] = a1
    case['rotation'][0, 3:] = np.float32(2.0) * a1 + np.float32(1e-3) * case['rotation'][1, 3:]
    for k in so.COTANGENTS:
        case[k][1] = case[k][0]
    kappa = so.conditioning(case['mean'], case['rotation'], case['R'], case['t'])[0]
    b = so.case_bounds(case, 0)
    assert kappa[0] > 100 * kappa[1]
    assert b[0][0].max() > 100 * b[0][1].max()
    f64, b64 = so.run(case, 0, np.float64)
    rel = b[3] / np.abs(b64[3]).max(1, keepdims=True)
    assert rel[0].max() > 100 * rel[1].max()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_known_rotations(dtype):
    rows = np.asarray(so.SPECIAL_ROWS, dtype=dtype)
    case = so.make_case(len(rows), 0, 1)
    case['rotation'] = rows
    fwd, bwd = so.run(case, 0, dtype)
    h = np.sqrt(dtype(0.5))
    want = [(1, 0, 0, 0), (0.5, 0, 0, 0), (0.5, -0.5, -0.5, -0.5), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1),
            (h, 0, 0, 0), (h, 0, 0, 0)]
    np.testing.assert_array_equal(fwd[2][:6], np.asarray(want[:6], dtype=dtype))
    # the tiny row's b1 is (1e-8, 0, 0): its matrix is a rotation to 1e-8 only
    np.testing.assert_allclose(fwd[2][6:], np.asarray(want[6:], dtype=dtype), rtol=0, atol=1e-7)
    g = bwd[3]
    assert g.dtype == dtype and np.all(np.isfinite(g))
    # the zero, parallel and tiny rows: F.normalize's eps is the divisor, the gradient is of order 1 / eps
    for r in (1, 6, 7):
        assert 1e10 < np.abs(g[r]).max() < 1e13, (r, g[r])
    for r in (0, 2, 3, 4, 5):
        assert np.abs(g[r]).max() < 10
    # and they are torch's: the stand-ins' autograd on the same rows
    _, grads = _autograd({k: np.asarray(v, np.float64) for k, v in case.items()}, 0)
    if dtype is np.float64:
        _close(g, grads[3], 1e-12)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_the_clamp_passes_the_gradient_at_equality(dtype):
    """Degree 0: u = C0 dc + 0.5.  A dc whose product with C0 rounds to exactly -0.5 gives u == 0: colour 0, gradient
    C0 g; one step further down u < 0 and the gradient is 0."""
    dt = np.dtype(dtype).type
    c0 = dt(so.C0)
    dc = dt(-0.5) / c0
    cand = [dc]
    for _ in range(64):
        cand = [np.nextafter(cand[0], dt(-10))] + cand + [np.nextafter(cand[-1], dt(0))]
    hits = [v for v in cand if c0 * v + dt(0.5) == 0]
    assert hits, 'no dc gives an unclamped colour of exactly 0'
    at, below = max(hits), min(hits)
    below = np.nextafter(below, dt(-10))
    while c0 * below + dt(0.5) == 0:
        below = np.nextafter(below, dt(-10))
    case = so.make_case(2, 0, 3)
    case = {k: np.asarray(v, dtype) for k, v in case.items()}
    case['feature_dc'][0, 0, :], case['feature_dc'][1, 0, :] = at, below
    fwd, bwd = so.run(case, 0, dtype)
    assert np.all(fwd[4][0] == 0) and np.all(fwd[4][1] < 0) and np.all(fwd[3] == 0)
    np.testing.assert_array_equal(bwd[4][0, 0], c0 * case['G_rgb'][0])
    assert np.all(bwd[4][0, 0] != 0) and np.all(bwd[4][1] == 0)
    if dtype is np.float64:       # torch's clamp_min does the same
        _, grads = _autograd(case, 0)
        np.testing.assert_array_equal(bwd[4], grads[4])


@pytest.mark.parametrize('deg,Mr', [(0, 15), (1, 15), (2, 15), (1, 3), (0, 3), (2, 8)])
def test_rows_above_the_active_degree_get_plus_zero(deg, Mr):
    case = so.make_case(9, Mr, 7)
    _, bwd = so.run(case, deg, np.float32)
    rest = bwd[5]
    active = so.n_coef(deg) - 1
    assert rest.shape == (9, Mr, 3) and rest.dtype == np.float32
    assert np.all(rest[:, active:, :].view(np.uint32) == 0)          # +0, not -0
    if active:
        assert np.all(np.abs(rest[:, :active, :]).sum((1, 2)) > 0)


def test_camera_centre_by_cofactors_is_the_inverse():
    case = so.make_case(1, 0, 11)
    R, t = case['R'].astype(np.float64), case['t'].astype(np.float64)
    np.testing.assert_allclose(so.camera_centre(R, t, np.float64), np.linalg.inv(R) @ -t, rtol=0, atol=1e-14)
    R = R @ np.diag([2.0, 0.5, 3.0]) + 0.1      # no rotation: the inverse is not the transpose
    np.testing.assert_allclose(so.camera_centre(R, t, np.float64), np.linalg.inv(R) @ -t, rtol=1e-12, atol=1e-13)
    err = np.abs(so.camera_centre(R, t, np.float32).astype(np.float64) - np.linalg.inv(R) @ -t)
    assert np.all(err <= so.camera_centre_error(R, t))
