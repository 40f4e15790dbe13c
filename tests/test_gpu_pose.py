"""The HIP pose-parameter stage (exavatar_release_amd.pose_params / pose_features / SMPLXParamDict) on the GPU.

The quaternion -- no transcendental precedes it -- equals the float32 oracle tests/pose_oracle.py BIT FOR BIT.  The
axis-angle and the gradients pass the device's ``atan2f`` / ``sinf`` / ``cosf``, which preclude bit equality with a CPU:
they are held against the float64 oracle with the allowance of tests/test_gpu_kinematics.py -- at most 4x the maximum
error of the CPU float32 evaluation of the same formula (the float32 oracle), floored at 2^-24 of the tensor's largest
magnitude.  The rows whose quaternion has no vector part (identity, zero, the degenerate frames) pass no transcendental
at a non-trivial argument and equal the float32 oracle bit for bit, gradients included.  Against the fixture recorded
from the reference's own class every output and gradient stays within ``FACTOR`` = 4 times the reference's own
float32-versus-float64 error, floored at ``FLOOR`` = 2^-24 (tests/test_gpu_human_chain.py's).  Cotangents that are missing,
packed or both, frozen parameters, more tensors than one call takes, repeated calls, the pose features and a captured
forward + backward of the chain into the kinematics are covered below."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import _lib
from exavatar_release_amd._device import _ptr, _ptrs, launch
from tests import helpers
from tests import pose_oracle as po

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 4.0
FLOOR = 2.0 ** -24
POSES = ('root_pose', 'body_pose', 'jaw_pose', 'leye_pose', 'reye_pose', 'lhand_pose', 'rhand_pose')
module = sys.modules['exavatar_release_amd.pose_params']


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = int((_bits(a) != _bits(b)).sum())
    assert bad == 0, '%s differs in %d of %d elements' % (what, bad, a.size)


def _dev(parts, grad=True):
    return [torch.from_numpy(p).to(DEV).requires_grad_(grad) for p in parts]


def _quat(parts):
    """The C call with `quat` alone: [R, 4]."""
    t = _dev(parts, False)
    rows = (ctypes.c_int32 * len(t))(*[x.shape[0] for x in t])
    q = torch.empty((sum(x.shape[0] for x in t), 4), dtype=torch.float32, device=DEV)
    launch(_lib.MESH, 'exa_mesh_pose_params_forward', DEV, len(t), rows, _ptrs(t), None, None, _ptr(q))
    return q.cpu().numpy()


def _run(parts, cots=None, packed_cot=None, packed=False, need=None):
    """pose_params on the device: (outputs, packed or None, gradients (None where not asked for or not reached))."""
    need = [True] * len(parts) if need is None else need
    t = [torch.from_numpy(p).to(DEV).requires_grad_(w) for p, w in zip(parts, need)]
    res = exa.pose_params(t, packed=packed)
    outs, pk = (res[:-1], res[-1]) if packed else (res, None)
    grads = [None] * len(parts)
    pairs = [(o, torch.from_numpy(g).to(DEV)) for o, g in zip(outs, cots or []) if g is not None]
    if packed_cot is not None:
        pairs.append((pk, torch.from_numpy(packed_cot).to(DEV)))
    wanted = [i for i, w in enumerate(need) if w]
    if pairs and wanted:
        got = torch.autograd.grad([o for o, _ in pairs], [t[i] for i in wanted], [g for _, g in pairs], allow_unused=True)
        for i, g in zip(wanted, got):
            grads[i] = None if g is None else g.cpu().numpy()
    return [o.detach().cpu().numpy() for o in outs], None if pk is None else pk.detach().cpu().numpy(), grads


@pytest.fixture(scope='module')
def rows():
    """The 4096 random rows with their cotangents and the oracle's three runs, computed once."""
    d6, g = po.random_rows(4096, seed=3)
    aa32, q32 = po.forward(d6)
    aa64, _ = po.forward(d6, np.float64)
    return dict(d6=d6, g=g, aa32=aa32, q32=q32, aa64=aa64, g32=po.backward(d6, g), g64=po.backward(d6, g, np.float64))


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'ref_pose.npz'))


# ---- 1. the quaternion, bit for bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize('sizes', [po.SEGMENT_ROWS, (4096,), (5, 0, 9), (0, 70, 0)], ids=['frame', '4096', 'empty-between',
                                                                                           'empty-ends'])
def test_quaternion_is_bit_exact(rows, sizes):
    R = sum(sizes)
    d6 = rows['d6'][:R].copy()
    sp = po.special_rows()
    n = min(len(sp), R)
    d6[R - n:] = sp[:n]                                   # the special rows at the end: in the last segments
    parts = po.split(d6, sizes)
    _same(_quat(parts), po.forward(d6)[1], 'quat')
    outs, pk, _ = _run(parts, packed=True)
    assert [o.shape for o in outs] == [(r, 3) for r in sizes] and pk.shape == (R, 3)
    _same(np.concatenate(outs), pk, 'packed against the separate outputs')


# ---- 2. axis-angle and gradients against float64 ---------------------------------------------------------------------
def _allowance(tag, dev, cpu32, exact):
    err_dev = float(np.abs(dev.astype(np.float64) - exact).max())
    err_cpu = float(np.abs(cpu32.astype(np.float64) - exact).max())
    floor = FLOOR * float(np.abs(exact).max())
    print('%s: device max error %.3e, CPU float32 max error %.3e, ratio %.2f, floor %.3e' % (
        tag, err_dev, err_cpu, err_dev / max(err_cpu, 1e-300), floor))
    helpers.record_stats('pose/' + tag, {'err_dev': err_dev, 'err_cpu': err_cpu, 'floor': floor,
                                         'ratio': err_dev / max(err_cpu, floor)})
    assert np.isfinite(dev).all()
    assert err_dev <= max(4 * err_cpu, floor), (tag, err_dev, err_cpu, floor)


def test_axis_angle_and_gradient_against_float64(rows):
    outs, _, grads = _run([rows['d6']], [rows['g']])
    _allowance('axis_angle', outs[0], rows['aa32'], rows['aa64'])
    _allowance('grad_d6', grads[0], rows['g32'], rows['g64'])


def test_special_rows_on_both_sides_of_each_branch():
    d6 = po.special_rows()
    g = np.ones((len(d6), 3), dtype=np.float32)
    g[1::2] = np.random.default_rng(9).standard_normal((len(d6[1::2]), 3)).astype(np.float32)
    outs, _, grads = _run([d6], [g])
    aa, gd = outs[0], grads[0]
    aa32, q32 = po.forward(d6)
    g32 = po.backward(d6, g)
    aa64, g64 = po.forward(d6, np.float64)[0], po.backward(d6, g, np.float64)
    _same(_quat([d6]), q32, 'quat')
    i, neg, small = po.decisions(d6)
    assert set(i.tolist()) == {0, 1, 2, 3} and small.any() and not small.all()
    assert np.isfinite(aa).all() and np.isfinite(gd).all()
    # no vector part: atan2f(0, w) = 0, the series at angle 0, nothing else transcendental -- the oracle's bits
    flat = ~q32[:, 1:].any(1)
    assert flat.sum() >= 4 and flat[0] and flat[1]
    _same(aa[flat], aa32[flat], 'axis-angle of the rows without a vector part')
    _same(gd[flat], g32[flat], 'gradient of the rows without a vector part')
    assert np.array_equal(gd[0], np.float32([0, -1, 1, 0, 0, -1]))      # the identity row, all-ones cotangent (a -0 is 0)
    # the others (the tie, the half turns, the series row, both sides of 1e-6) against float64
    rest = ~flat
    assert small[rest].any() and not small[rest].all()
    _allowance('special/axis_angle', aa[rest], aa32[rest], aa64[rest])
    _allowance('special/grad_d6', gd[rest], g32[rest], g64[rest])


# ---- 3. against the fixture ------------------------------------------------------------------------------------------
def _ratio(golden, key, got):
    ref = golden[key]
    got = got.detach().cpu().double().numpy().reshape(ref.shape)
    e = got - ref
    norm = float(np.linalg.norm(ref))
    if norm == 0.0:
        return 0.0 if not e.any() else float('inf')
    rel_l2, rel_max = max(float(golden[key + '#rel_l2']), FLOOR), max(float(golden[key + '#rel_max']), FLOOR)
    return max(float(np.linalg.norm(e)) / (rel_l2 * norm), float(np.abs(e).max()) / (rel_max * norm / np.sqrt(ref.size)))


def _module(golden):
    m = exa.SMPLXParamDict()
    m.init({int(f): {n: torch.from_numpy(golden['raw/%d/%s' % (f, n)]).float() for n in module.PARAM_NAMES}
            for f in golden['frames']})
    return m.to(DEV)


def test_against_the_fixture(golden):
    m = _module(golden)
    frames = [int(f) for f in golden['frames']]
    res = m(torch.tensor(frames), packed=True)
    assert len(res) == 2
    ratios = {}
    for f, frame in zip(frames, res):
        assert list(frame.keys()) == list(module.PARAM_NAMES) + ['pose']
        assert frame['expr'] is m.smplx_params[str(f)]['expr'] and frame['trans'] is m.smplx_params[str(f)]['trans']
        assert tuple(frame['pose'].shape) == (55, 3)
        _same(frame['pose'].detach().cpu().numpy(),
              np.concatenate([frame[n].detach().cpu().numpy().reshape(-1, 3) for n in POSES]), 'pose of frame %d' % f)
        for n in POSES:
            assert frame[n].shape == m.smplx_params[str(f)][n].shape[:-1] + (3,)
            ratios['out/%d/%s' % (f, n)] = _ratio(golden, 'out/%d/%s' % (f, n), frame[n])
    outs = [frame[n] for frame in res for n in POSES]
    cots = [torch.from_numpy(golden['G/%d/%s' % (f, n)]).float().to(DEV) for f in frames for n in POSES]
    params = [m.smplx_params[str(f)][n] for f in frames for n in POSES]
    grads = torch.autograd.grad(outs, params, cots)
    for (f, n), g in zip([(f, n) for f in frames for n in POSES], grads):
        ratios['grad/%d/%s' % (f, n)] = _ratio(golden, 'grad/%d/%s' % (f, n), g)
    worst = sorted(ratios.items(), key=lambda kv: -kv[1])
    for k, r in worst:
        print('%-24s ratio %.3f' % (k, r))
    helpers.record_stats('pose/fixture', {'max_ratio': worst[0][1], 'at': worst[0][0], 'ratios': ratios})
    bad = [(k, round(r, 2)) for k, r in worst if not r <= FACTOR]
    assert not bad, 'HIP error above %g x the reference\'s own float32 error: %s' % (FACTOR, bad)
    # the packed output alone carries the same gradients as the separate ones
    res2 = m(frames, packed=True)
    packed_cots = [torch.cat([c.reshape(-1, 3) for c in cots[7 * k:7 * k + 7]]) for k in range(2)]
    grads2 = torch.autograd.grad([fr['pose'] for fr in res2], params, packed_cots)
    for a, b, p in zip(grads, grads2, params):
        _same(a.cpu().numpy(), b.cpu().numpy(), 'gradient through the packed pose')


# ---- 4. partial work -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def partial(rows):
    sizes = (7, 40, 1, 30)
    d6, g = rows['d6'][100:178].copy(), rows['g'][100:178].copy()
    d6[:3] = po.special_rows()[[0, 2, 11]]
    parts, cots = po.split(d6, sizes), po.split(g, sizes)
    outs, pk, grads = _run(parts, cots, packed=True)
    return dict(sizes=sizes, d6=d6, g=g, parts=parts, cots=cots, outs=outs, pk=pk, grads=grads)


def test_a_segment_without_a_cotangent(partial):
    c = partial
    cots = [c['cots'][0], None, c['cots'][2], None]
    _, _, grads = _run(c['parts'], cots)
    for k in (0, 2):
        _same(grads[k], c['grads'][k], 'gradient of segment %d' % k)
    for k in (1, 3):                                     # requested, reached by +0 alone
        assert grads[k].shape == c['parts'][k].shape and not grads[k].any()


def test_a_packed_cotangent_alone(partial):
    c = partial
    _, _, grads = _run(c['parts'], None, packed_cot=c['g'], packed=True)
    for k in range(4):
        _same(grads[k], c['grads'][k], 'gradient of segment %d' % k)


def test_both_cotangents_are_one_rounded_add(partial):
    c = partial
    extra = np.random.default_rng(4).standard_normal(c['g'].shape).astype(np.float32)
    cots = [c['cots'][0], None, c['cots'][2], c['cots'][3]]
    _, _, grads = _run(c['parts'], cots, packed_cot=extra, packed=True)
    summed = [e if g is None else g + e for g, e in zip(cots, po.split(extra, c['sizes']))]      # float32: one rounding
    _, _, want = _run(c['parts'], summed)
    for k in range(4):
        _same(grads[k], want[k], 'gradient of segment %d' % k)


def test_a_frozen_parameter_gets_no_gradient(partial, monkeypatch):
    c = partial
    seen = []
    real = module.launch

    def spy(abi, name, dev, *args):
        seen.append((name, [args[5][k] for k in range(args[0])] if name.endswith('backward') else None))
        return real(abi, name, dev, *args)
    monkeypatch.setattr(module, 'launch', spy)
    outs, pk, grads = _run(c['parts'], c['cots'], packed=True, need=[True, False, True, True])
    assert grads[1] is None
    for k in (0, 2, 3):
        _same(grads[k], c['grads'][k], 'gradient of segment %d' % k)
    _same(pk, c['pk'], 'packed')
    assert [n for n, _ in seen] == ['exa_mesh_pose_params_forward', 'exa_mesh_pose_params_backward']
    ptrs = seen[1][1]
    assert ptrs[1] is None and all(ptrs[k] for k in (0, 2, 3))      # NULL: nothing is computed for the frozen segment


class _Drop(torch.autograd.Function):
    """Passes its input on and hands no gradient back."""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return None


def test_no_cotangent_at_all_is_no_launch(partial, monkeypatch):
    t = _dev(partial['parts'])
    other = torch.ones(3, device=DEV, requires_grad=True)
    outs = exa.pose_params(t)
    calls = []
    real = module.launch
    monkeypatch.setattr(module, 'launch', lambda *a: (calls.append(a[1]), real(*a))[1])
    loss = sum(_Drop.apply(o).sum() for o in outs) + other.sum()
    loss.backward()
    assert calls == [] and all(x.grad is None for x in t) and other.grad is not None


def test_more_tensors_than_one_call_takes(rows, monkeypatch):
    sizes = [1 + (k % 3) for k in range(70)]                     # 139 rows in 70 tensors: two C calls each way
    R = sum(sizes)
    d6, g = rows['d6'][200:200 + R], rows['g'][200:200 + R]
    calls = []
    real = module.launch
    monkeypatch.setattr(module, 'launch', lambda *a: (calls.append((a[1], a[3])), real(*a))[1])
    outs, pk, grads = _run(po.split(d6, sizes), po.split(g, sizes), packed=True)
    assert calls == [('exa_mesh_pose_params_forward', 64), ('exa_mesh_pose_params_forward', 6),
                     ('exa_mesh_pose_params_backward', 64), ('exa_mesh_pose_params_backward', 6)]
    one_out, _, one_grad = _run([d6], [g])
    _same(pk, one_out[0], 'packed')
    _same(np.concatenate(outs), one_out[0], 'outputs')
    _same(np.concatenate(grads), one_grad[0], 'gradients')


# ---- 5. bit-reproducible ---------------------------------------------------------------------------------------------
def test_repeated_calls_give_identical_bits(partial):
    c = partial
    for _ in range(2):
        outs, pk, grads = _run(c['parts'], c['cots'], packed=True)
        _same(pk, c['pk'], 'packed')
        for k in range(4):
            _same(outs[k], c['outs'][k], 'output %d' % k)
            _same(grads[k], c['grads'][k], 'gradient %d' % k)


def test_leading_dimensions_and_views(rows):
    d6 = rows['d6'][:24]
    a = torch.from_numpy(d6).to(DEV)
    flat = exa.pose_params([a])[0]
    shaped, single, strided = exa.pose_params([a.view(2, 3, 4, 6), a[5], a[::2]])
    assert tuple(shaped.shape) == (2, 3, 4, 3) and tuple(single.shape) == (3,) and tuple(strided.shape) == (12, 3)
    assert torch.equal(shaped.view(24, 3), flat) and torch.equal(single, flat[5]) and torch.equal(strided, flat[::2])


# ---- 6. pose_features ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('J,n_body', [(55, 21), (64, 63), (2, 1), (1, 0), (55, 0)])
def test_pose_features_are_a_slice_and_a_subtraction(J, n_body):
    from exavatar_release_amd import p3d_standins as p3d
    rot = torch.randn(J, 3, 3, generator=torch.Generator().manual_seed(J)).to(DEV)
    pose6d, pose_feat = exa.pose_features(rot, n_body)
    assert not pose6d.requires_grad and not pose_feat.requires_grad
    assert tuple(pose6d.shape) == (6 * n_body,) and tuple(pose_feat.shape) == (1, 9 * (J - 1))
    assert torch.equal(pose6d, p3d.matrix_to_rotation_6d(rot[1:1 + n_body]).reshape(n_body * 6))
    assert torch.equal(pose_feat, (rot[1:] - torch.eye(3, device=DEV)[None, :, :]).view(1, (J - 1) * 9))


# ---- 7. the chain into the kinematics, captured ----------------------------------------------------------------------
def test_chain_replays_from_one_captured_graph_and_agrees_with_the_standin_chain():
    """tests/_pose_capture.py in a child process under a time limit: a capture that hangs must not take the session with
    it."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_pose_capture.py')], capture_output=True, text=True,
                       timeout=240, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and 'RESULT ok' in r.stdout, 'child: rc %d\n%s\n%s' % (r.returncode, r.stdout[-800:],
                                                                                   r.stderr[-1500:])
