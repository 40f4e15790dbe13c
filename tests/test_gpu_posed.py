"""GPU tests of the posed SMPL-X stage (exavatar_release_amd/posed_body.py, csrc/posed_body.hip, include/exa_mesh.h
exa_mesh_posed_*).

The three outputs and the five gradients are held to tests/posed_oracle.py bit for bit once the oracle is fed the
device's ``rot`` (and, backward, its sin / cos): the Rodrigues step is the one place where the device's sinf / cosf
preclude bit equality with a CPU, and it is held on its own against float64 with the rule of
tests/test_gpu_kinematics.py (at most 4x the CPU float32 evaluation's own maximum error, floored at one ulp of 1.0).
The shapes are the smallest at which every path is left: 642 vertices (two full 256-vertex chunks and a partial one)
and 35 (less than one), the SMPL-X tree and three joints as a chain and as a star, both coefficient arrays, one, the
other; with and without joint_offset, face_offset, pose_mean and the camera; exact zero pose rows for both eyes and one
angle within 1e-3 of pi.  Then the reference's own run (tests/golden/ref_posed.npz) within 4x its own float32 error,
every pattern of missing cotangents, unneeded gradients, reproducibility under poisoned workspaces, a captured graph,
the chain from ``SMPLXParamDict`` and the agreement with ``BodyTemplate`` at a constant pose."""
import itertools
import os
import types

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import lbs, posed_body
from tests import body_oracle as bo
from tests import human_case
from tests import kin_oracle
from tests import posed_oracle as po

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_posed.npz')
ULP1 = 2.0 ** -23
GRADS = tuple('grad_' + k for k in po.INPUTS)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b, what):
    assert a.shape == b.shape, what
    bad = int((_bits(a) != _bits(b)).sum())
    assert bad == 0, '%s differs in %d of %d elements' % (what, bad, a.size)


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _icosphere(level):
    verts, faces = human_case._icosphere(level)
    return verts * np.asarray(human_case.RADII), faces


def _module(case):
    return exa.PosedBody(_t(case['v_template']), _t(case['shape_dirs']), _t(case['posedirs']), _t(case['J_regressor']),
                         _t(case['weights']), list(case['parents']), pose_mean=_t(case['pose_mean']),
                         face_offset=_t(case['face_offset']))


def _run(body, inp, cot, need=(True,) * 5):
    """The module's outputs and gradients as numpy arrays, with the device's own rot, (sin, cos) and inverse(R)."""
    exa.config.keep_debug = True
    x = {k: None if inp[k] is None else _t(inp[k]).requires_grad_(w) for k, w in zip(po.INPUTS, need)}
    out = body(x['pose'], x['betas'], x['expression'], x['transl'], x['joint_offset'], _t(inp['R']), _t(inp['t']))
    assert isinstance(out, exa.PosedBodyOutput) and not out.rot.requires_grad
    J = body.num_joints
    res = {k: None if o is None else o.detach().cpu().numpy() for k, o in zip(out._fields, out)}
    res['sincos'] = body.debug_workspace[:8 * J].view(torch.float32).view(J, 2).cpu().numpy()
    res['Rinv'] = None if inp['R'] is None else torch.inverse(_t(inp['R'])).cpu().numpy()
    present = [(getattr(out, k), _t(cot[k])) for k in po.OUTPUTS if cot.get(k) is not None]
    wanted = [k for k, w in zip(po.INPUTS, need) if w and x[k] is not None]
    if present and wanted:
        grads = torch.autograd.grad([o for o, _ in present], [x[k] for k in wanted], [g for _, g in present])
        res.update({'grad_' + k: g.cpu().numpy() for k, g in zip(wanted, grads)})
    return res


def _oracle(case, inp, cot, got, dtype=np.float32):
    """The oracle over the device's rot / sincos / inverse(R) (float32), or on its own (float64)."""
    f32 = dtype == np.float32
    Rinv = got['Rinv'] if f32 else (None if inp['R'] is None else np.linalg.inv(inp['R'].astype(np.float64)))
    fwd = po.forward(case, inp['pose'], inp['betas'], inp['expression'], inp['transl'], inp['joint_offset'], Rinv, inp['t'],
                     dtype, rot=got['rot'] if f32 else None)
    res = {k: fwd[k] for k in po.OUTPUTS + ('rot',)}
    if any(cot.get(k) is not None for k in po.OUTPUTS):
        grads = po.backward(case, inp['pose'], fwd, cot, Rinv, dtype, sincos=got['sincos'] if f32 else None,
                            n_betas=inp['betas'].shape[0])
        res.update({'grad_' + k: v for k, v in grads.items()})
    return res


def _check(name, case, inp, cot, got=None):
    got = _run(_module(case), inp, cot) if got is None else got
    want = _oracle(case, inp, cot, got)
    for k in po.OUTPUTS:
        if inp['R'] is None and k == 'vertices_world':
            assert got[k] is None
            continue
        _same(got[k], want[k], '%s: %s' % (name, k))
    for k in po.INPUTS:
        if inp[k] is None:
            continue
        assert np.isfinite(got['grad_' + k]).all(), k
        _same(got['grad_' + k], want['grad_' + k], '%s: dL/d%s' % (name, k))
    return got


# name: (mesh, parents, (Lb, Le), pose_mean, face_offset, joint_offset, camera, regressor)
CASES = {
    'icosphere642-smplx-7+5-all': (lambda: _icosphere(3), lbs.SMPLX_PARENTS, (7, 5), True, True, True, True, 'sparse'),
    'icosphere642-smplx-10+0-plain': (lambda: _icosphere(3), lbs.SMPLX_PARENTS, (10, 0), False, False, False, False, 'sparse'),
    'grid35-smplx-0+3-rows': (lambda: bo.grid(5, 7), lbs.SMPLX_PARENTS, (0, 3), True, False, True, True, 'rows'),
    'grid35-chain3-7+5': (lambda: bo.grid(5, 7), bo.chain_tree(3), (7, 5), True, True, False, True, 'sparse'),
    'grid35-star3-10+0': (lambda: bo.grid(5, 7), bo.star_tree(3), (10, 0), False, True, True, False, 'rows'),
    'grid35-star3-0+3': (lambda: bo.grid(5, 7), bo.star_tree(3), (0, 3), True, False, False, True, 'sparse'),
}


def _build(name, seed=301):
    mesh, parents, (Lb, Le), mean, face, jo, cam, regressor = CASES[name]
    verts, faces = mesh()
    case = po.random_case(verts, faces, Lb + Le, parents, seed, mean, face, regressor)
    J = len(parents)
    zero, near_pi = ((23, 24), 22) if J == 55 else ((1,), 2)
    if mean:
        case['pose_mean'][list(zero)] = 0
    inp = po.random_inputs(case, Lb, seed + 1, jo, cam, zero_rows=zero, pi_row=near_pi)
    full = inp['pose'].astype(np.float64) + (0 if case['pose_mean'] is None else case['pose_mean'])
    assert not full[list(zero)].any() and abs(np.linalg.norm(full[near_pi]) - np.pi) < 1e-3
    return case, inp, po.random_cotangents(case, seed + 2, cam), zero


# ---- 1. bit for bit against the float32 oracle; 6. the zero pose rows -------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_bit_exact_against_the_oracle(name):
    case, inp, cot, zero = _build(name)
    got = _check(name, case, inp, cot)
    rows = got['grad_pose'][list(zero)]
    assert np.isfinite(rows).all() and rows.any(), 'the zero pose rows get a finite, non-zero gradient'
    _same(got['rot'][list(zero)], np.broadcast_to(np.eye(3, dtype=np.float32), (len(zero), 3, 3)), 'rot of a zero row')


def test_leading_axes_of_one_and_refusals():
    case, inp, cot, _ = _build('grid35-chain3-7+5')
    body = _module(case)
    plain = _run(body, inp, cot)
    lead = dict(inp, **{k: inp[k][None] for k in ('pose', 'betas', 'expression', 'transl')})
    got = _run(body, lead, cot)
    for k in po.OUTPUTS:
        _same(got[k], plain[k], k)
    assert got['grad_pose'].shape == (1, 3, 3) and got['grad_betas'].shape == (1, 7) and got['grad_transl'].shape == (1, 3)
    _same(got['grad_pose'][0], plain['grad_pose'], 'dL/dpose of [1, J, 3]')
    a = {k: _t(inp[k]) for k in po.INPUTS if inp[k] is not None}
    R, t = _t(inp['R']), _t(inp['t'])
    with pytest.raises(ValueError, match='pose holds a batch of 2; the stage takes one sample per call'):
        body(torch.stack([a['pose']] * 2), a['betas'], a['expression'], a['transl'])
    with pytest.raises(ValueError, match='betas holds a batch of 2'):
        body(a['pose'], torch.stack([a['betas']] * 2), a['expression'], a['transl'])
    with pytest.raises(ValueError, match=r'pose must be \[J, 3\] or \[1, J, 3\] with J = 3'):
        body(a['pose'][:2], a['betas'], a['expression'], a['transl'])
    with pytest.raises(ValueError, match=r'betas and expression hold 7 \+ 4 coefficients, shape_dirs 12'):
        body(a['pose'], a['betas'], a['expression'][:4], a['transl'])
    with pytest.raises(ValueError, match=r'transl must be \[3\] or \[1, 3\]'):
        body(a['pose'], a['betas'], a['expression'], a['transl'][:2])
    with pytest.raises(ValueError, match='joint_offset must be'):
        body(a['pose'], a['betas'], a['expression'], a['transl'], torch.zeros(4, 3, device=DEV))
    with pytest.raises(ValueError, match='R and t must be given together'):
        body(a['pose'], a['betas'], a['expression'], a['transl'], None, R)
    with pytest.raises(ValueError, match='PosedBody: R is camera data in the reference and gets no gradient'):
        body(a['pose'], a['betas'], a['expression'], a['transl'], None, R.clone().requires_grad_(True), t)
    with pytest.raises(ValueError, match='must be float32'):
        body(a['pose'].double(), a['betas'], a['expression'], a['transl'])
    with pytest.raises(RuntimeError, match='PosedBody runs on a ROCm device only'):
        body(a['pose'], a['betas'], a['expression'].cpu(), a['transl'])
    with pytest.raises(ValueError, match='move the module with .to'):
        _module(case).to('cpu')(a['pose'], a['betas'], a['expression'], a['transl'])
    moved = _module(case).to('cpu').to(DEV)                # .to() moves the tables; state_dict stays empty
    assert moved.state_dict() == {}
    _same(_run(moved, inp, cot)['vertices'], plain['vertices'], 'after .to()')


# ---- 2. the Rodrigues step on its own ---------------------------------------------------------------------------------
def _trig_poses(J, mean):
    """Axis-angle rows whose full pose (+ pose_mean) has the angles at which sin / cos are hard: tiny, around pi / 2, pi,
    2 pi and beyond."""
    rng = np.random.RandomState(7)
    angles = np.concatenate([[0.0, 1e-7, 1e-4, 1e-2, np.pi / 2, np.pi - 1e-3, np.pi - 1e-6, np.pi, np.pi + 1e-3, 2 * np.pi,
                              2 * np.pi + 0.5, 9.0], rng.uniform(0, np.pi, J)])[:J]
    axes = rng.standard_normal((J, 3))
    return (axes / np.linalg.norm(axes, axis=1, keepdims=True) * angles[:, None] - mean).astype(np.float32)


def _rodrigues_errors(got_rot, pose, mean):
    exact = po.rodrigues(pose, mean, np.float64)[0]
    cpu32 = po.rodrigues(pose, mean, np.float32)[0]
    err_dev = float(np.abs(got_rot.astype(np.float64) - exact).max())
    err_cpu = float(np.abs(cpu32.astype(np.float64) - exact).max())
    return err_dev, err_cpu


def test_rodrigues_step_against_float64():
    case, inp, cot, _ = _build('icosphere642-smplx-7+5-all')
    body = _module(case)
    worst = 0.0
    for tag, pose in (('the case\'s pose', inp['pose']), ('the hard angles', _trig_poses(55, case['pose_mean']))):
        got = _run(body, dict(inp, pose=pose), {})
        err_dev, err_cpu = _rodrigues_errors(got['rot'], pose, case['pose_mean'])
        print('rot, %s: device max error %.3e, CPU float32 max error %.3e, ratio %.2f' % (tag, err_dev, err_cpu,
                                                                                         err_dev / err_cpu))
        worst = max(worst, err_dev / err_cpu)
        assert err_dev <= max(4 * err_cpu, ULP1), (tag, err_dev, err_cpu)
    print('rot: worst ratio %.2f' % worst)


# ---- 3. the reference's own run ---------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def golden():
    case, inp, cot = po.golden_inputs()
    return types.SimpleNamespace(case=case, inp=inp, cot=cot, ref=dict(np.load(GOLDEN)))


def test_against_the_references_own_run(golden):
    """Every output and gradient within 4 * ref_f32_err/<name> of the float64 run of the reference's own code: the
    reference's float32 run loses ref_f32_err, the factor 4 covers a different but fixed summation order."""
    got = _run(_module(golden.case), golden.inp, golden.cot)
    for k in po.OUTPUTS + ('rot',) + GRADS:
        err = float(np.abs(got[k].astype(np.float64) - golden.ref[k]).max())
        own = float(golden.ref['ref_f32_err/' + k])
        print('%-18s max |hip - reference| %.3e, ref_f32_err %.3e, ratio %.2f' % (k, err, own, err / own))
        assert np.isfinite(got[k]).all() and err <= 4 * own, k
    _check('golden', golden.case, golden.inp, golden.cot, got)      # and the float32 oracle, bit for bit


# ---- 4. missing cotangents --------------------------------------------------------------------------------------------
def test_every_pattern_of_missing_cotangents_bit_exact():
    case, inp, full, _ = _build('grid35-smplx-0+3-rows')
    body = _module(case)
    n = 0
    for mask in itertools.product((False, True), repeat=3):
        if not any(mask):
            continue
        cot = {k: full[k] if m else None for k, m in zip(po.OUTPUTS, mask)}
        _check('cotangents %s' % (mask,), case, inp, cot, _run(body, inp, cot))
        n += 1
    assert n == 7


# ---- 5. unneeded gradients --------------------------------------------------------------------------------------------
def test_unneeded_gradients_are_none_and_never_allocated(monkeypatch):
    case, inp, cot, _ = _build('grid35-chain3-7+5')
    inp['joint_offset'] = (0.02 * np.random.RandomState(3).standard_normal((3, 3))).astype(np.float32)
    body = _module(case)
    both = _run(body, inp, cot)
    seen = []
    real = posed_body.launch

    def spy(abi, name, dev, *args):
        if name == 'exa_mesh_posed_backward':
            seen.append([a.value for a in args[11:16]])      # dL_dpose, dL_dbetas, dL_dexpression, dL_dtransl, dL_djoint_offset
        return real(abi, name, dev, *args)
    monkeypatch.setattr(posed_body, 'launch', spy)
    for i, only in enumerate(po.INPUTS):
        for need in (tuple(j == i for j in range(5)), tuple(j != i for j in range(5))):
            del seen[:]
            got = _run(body, inp, cot, need)
            assert len(seen) == 1
            for k, w, ptr in zip(po.INPUTS, need, seen[0]):
                assert ('grad_' + k in got) == w and (ptr is not None) == w, (only, k)
                if w:
                    _same(got['grad_' + k], both['grad_' + k], 'dL/d%s with %s' % (k, need))
    del seen[:]
    x = [_t(inp[k]) for k in po.INPUTS]
    out = body(*x, _t(inp['R']), _t(inp['t']))
    assert not any(o.requires_grad for o in out) and not seen      # nothing needs a gradient: no backward at all
    # a joint_offset of None: no gradient slot, the same values as zeros
    none = _run(body, dict(inp, joint_offset=None), cot)
    zeros = _run(body, dict(inp, joint_offset=np.zeros((3, 3), np.float32)), cot)
    assert 'grad_joint_offset' not in none
    for k in po.OUTPUTS + ('grad_pose', 'grad_betas', 'grad_transl'):
        _same(none[k], zeros[k], k)


# ---- 7. reproducibility -----------------------------------------------------------------------------------------------
def test_repeated_calls_and_poisoned_workspaces_give_identical_bits(golden):
    body = _module(golden.case)
    first = _run(body, golden.inp, golden.cot)
    second = _run(body, golden.inp, golden.cot)
    exa.config.poison = True
    poisoned = _run(body, golden.inp, golden.cot)
    only = {k: golden.cot[k] if k == 'joints' else None for k in po.OUTPUTS}
    poisoned_joints = _run(body, golden.inp, only)
    exa.config.poison = False
    plain_joints = _run(body, golden.inp, only)
    for k in po.OUTPUTS + ('rot',) + GRADS:
        _same(first[k], second[k], k + ' on the second call')
        _same(first[k], poisoned[k], k + ' with poisoned workspaces')
    for k in GRADS:
        _same(plain_joints[k], poisoned_joints[k], k + ' from joints alone, poisoned')


# ---- 8. graph capture -------------------------------------------------------------------------------------------------
def test_graph_capture_replays_with_new_inputs():
    # no camera step: its torch.inverse(R) (taken in the wrapper, as the reference does) synchronises on ROCm and cannot be
    # captured; the kernels can
    case, inp, cot, _ = _build('icosphere642-smplx-10+0-plain')
    inp['joint_offset'] = (0.02 * np.random.RandomState(4).standard_normal((55, 3))).astype(np.float32)
    body = _module(case)
    x = [_t(inp[k]).clone().requires_grad_(True) for k in po.INPUTS]
    G = [_t(cot[k]) for k in ('vertices', 'joints')]

    def step():
        out = body(*x)
        return out, torch.autograd.grad([out.vertices, out.joints], x, G)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, grads = step()
    new = po.random_inputs(case, 10, 99, True, False, zero_rows=(23,))
    with torch.no_grad():
        for t, k in zip(x, po.INPUTS):
            t.copy_(_t(new[k]))
    graph.replay()
    torch.cuda.synchronize()
    eager = _run(body, new, cot)
    for k, a in zip(('vertices', 'joints') + GRADS, [out.vertices, out.joints] + list(grads)):
        _same(a.detach().cpu().numpy(), eager[k], k + ' after the replay')
    assert (_bits(eager['vertices']) != _bits(_run(body, inp, cot)['vertices'])).any()      # the inputs did change


# ---- 9. the chain from the pose parameters ----------------------------------------------------------------------------
def test_pose_parameters_chain_into_the_posed_body(golden):
    """``SMPLXParamDict(packed=True)['pose']`` is the layer's [55, 3] pose as it is; the cotangent of the
    vertices reaches the 6D parameters, bit-equal to the two stages run one after the other by hand."""
    body = _module(golden.case)
    pose = torch.from_numpy(golden.inp['pose'])
    spans = dict(root_pose=(0, 1), body_pose=(1, 22), jaw_pose=(22, 23), leye_pose=(23, 24), reye_pose=(24, 25),
                 lhand_pose=(25, 40), rhand_pose=(40, 55))
    frame = {k: pose[a:b].reshape(-1) if k in ('root_pose', 'jaw_pose', 'leye_pose', 'reye_pose') else pose[a:b]
             for k, (a, b) in spans.items()}
    frame.update(expr=torch.from_numpy(golden.inp['expression']), trans=torch.from_numpy(golden.inp['transl']))
    params = exa.SMPLXParamDict()
    params.init({0: frame}, device=DEV)
    betas, jo = _t(golden.inp['betas']).requires_grad_(True), _t(golden.inp['joint_offset']).requires_grad_(True)
    R, t, G = _t(golden.inp['R']), _t(golden.inp['t']), _t(golden.cot['vertices_world'])

    def run():
        (p,) = params([0], packed=True)
        assert p['pose'].shape == (55, 3)
        out = body(p['pose'], betas, p['expr'], p['trans'], jo, R, t)
        leaves = [params.smplx_params['0'][k] for k in spans] + [params.smplx_params['0']['expr'],
                                                                 params.smplx_params['0']['trans'], betas, jo]
        (g_pose,) = torch.autograd.grad(out.vertices_world, p['pose'], G, retain_graph=True)
        return out, p['pose'], g_pose, torch.autograd.grad(out.vertices_world, leaves, G)

    out, packed, g_pose, grads = run()
    _, _, _, again = run()
    for k, g, g2 in zip(list(spans) + ['expr', 'trans', 'betas', 'joint_offset'], grads, again):
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, k
        assert torch.equal(g, g2), k
    # by hand: the posed body on the detached packed pose, then its pose gradient into the packed cotangent
    by_hand = _run(body, dict(golden.inp, pose=packed.detach().cpu().numpy()), dict(vertices_world=golden.cot['vertices_world']))
    _same(out.vertices_world.detach().cpu().numpy(), by_hand['vertices_world'], 'vertices_world')
    _same(g_pose.cpu().numpy(), by_hand['grad_pose'], 'dL/dpose')
    (p,) = params([0], packed=True)
    want = torch.autograd.grad(p['pose'], [params.smplx_params['0'][k] for k in spans], _t(by_hand['grad_pose']))
    for k, g, w in zip(spans, grads, want):
        _same(g.cpu().numpy(), w.cpu().numpy(), 'dL/d' + k)
    # the pose is the reference's axis-angle to the pose stage's own accuracy, so the mesh is the golden's closely
    err = float(np.abs(out.vertices_world.detach().cpu().numpy() - golden.ref['vertices_world']).max())
    print('vertices_world through the 6D parameters: max |hip - reference| %.3e' % err)


# ---- 10. consistency with the template stage --------------------------------------------------------------------------
def test_agrees_with_the_template_stage_at_a_constant_pose():
    """The same constant pose and coefficients through ``BodyTemplate`` (rotations and pose offsets computed once in
    float64 and rounded) and through ``PosedBody`` (Rodrigues and the correctives on the device), the root row of
    joint_offset zero.  Both evaluate one polynomial of the tables, the coefficients and the rotations in float32, each
    within its first-order bound E = K u * (the sum of the monomials' magnitudes) of the exact value at its own
    rotations (tests/body_oracle.py's count K, with the P + 3 roundings of the device's corrective sum on the posed
    side and the constants' own on the template's); and the rotations differ per entry by at most B = the bound of the
    Rodrigues test + the half ulp of the template's rounding.  The mesh is at most quadratic in any one rotation entry,
    so central differences of the float64 oracle give d mesh / d rot exactly: |difference| <= E_posed + E_template +
    B * sum_entries |d mesh / d rot|."""
    verts, faces = bo.grid(5, 7)
    parents = bo.chain_tree(3)
    L, J, V = 7, 3, verts.shape[0]
    P = 9 * (J - 1)
    tcase, coef, jo = bo.random_case(verts, faces, L, parents, 1, 401)
    jo[0] = 0
    rng = np.random.RandomState(402)
    pose = (0.5 * rng.standard_normal((J, 3))).astype(np.float32)
    posedirs = (0.01 * rng.standard_normal((P, 3 * V))).astype(np.float32)
    rot64 = po.rodrigues(pose, None, np.float64)[0]
    feat64 = (rot64[1:] - np.eye(3)).reshape(-1)
    offsets64 = (feat64 @ posedirs.astype(np.float64)).reshape(V, 3)
    tcase.update(rot_pose=rot64.astype(np.float32), rot_inverse=np.ascontiguousarray(np.swapaxes(rot64, 1, 2)).astype(np.float32),
                 pose_offsets=offsets64.astype(np.float32))
    up = exa.MeshUpsampler(tcase['faces'], 1, num_verts=V).to(DEV)
    tpl = exa.BodyTemplate(_t(tcase['v_template']), _t(tcase['shape_dirs']), _t(tcase['J_regressor']), _t(tcase['weights']),
                           parents, up, rot_pose=_t(tcase['rot_pose']), rot_inverse=_t(tcase['rot_inverse']),
                           pose_offsets=_t(tcase['pose_offsets']), face_offset=_t(tcase['face_offset']), root_joint_idx=0)
    mesh = tpl(_t(coef), _t(jo)).mesh.cpu().numpy()
    pcase = dict({k: tcase[k] for k in ('v_template', 'face_offset', 'shape_dirs', 'J_regressor', 'weights', 'parents')},
                 posedirs=posedirs, pose_mean=None)
    inp = dict(pose=pose, betas=coef, expression=np.zeros(0, np.float32), transl=np.zeros(3, np.float32), joint_offset=jo,
               R=None, t=None)
    got = _run(_module(pcase), inp, {})
    # B: the Rodrigues test's bound at this pose, and the template's rounding of its constants
    err_dev, err_cpu = _rodrigues_errors(got['rot'], pose, None)
    assert err_dev <= max(4 * err_cpu, ULP1)
    B = max(4 * err_cpu, ULP1) + 2.0 ** -24
    # d mesh / d rot by central differences of the float64 oracle (exact for a quadratic)
    args = (pcase, pose, coef, inp['expression'], inp['transl'], jo, None, None, np.float64)
    sens = np.zeros((V, 3))
    h = 2.0 ** -10
    for e in range(9 * J):
        d = np.zeros(9 * J)
        d[e] = h
        d = d.reshape(J, 3, 3)
        sens += np.abs(po.forward(*args, rot=rot64 + d)['vertices'] - po.forward(*args, rot=rot64 - d)['vertices']) / (2 * h)
    # E: the template stage's count over the monomials' magnitudes, the corrective sum expanded term by term
    D = max(kin_oracle.depths(list(parents)))
    c64 = dict(tcase, rot_pose=rot64, pose_offsets=offsets64, rot_inverse=np.swapaxes(rot64, 1, 2))
    cmag = dict(c64, pose_offsets=(np.abs(feat64) @ np.abs(posedirs.astype(np.float64))).reshape(V, 3))
    mag = bo.forward(cmag, coef, jo, np.float64, True)['mesh']
    E_tpl = bo.roundings(c64, 2 * (D + 1) + 1)['mesh'] * bo.U * mag
    E_posed = bo.roundings(c64, P + 3)['mesh'] * bo.U * mag
    bound = E_tpl + E_posed + B * sens
    err = np.abs(got['vertices'].astype(np.float64) - mesh.astype(np.float64))
    print('max |PosedBody.vertices - BodyTemplate.mesh| %.3e, max bound %.3e (rotations %.3e), max err / bound %.3f'
          % (err.max(), bound.max(), (B * sens).max(), (err / bound).max()))
    assert (err <= bound).all()
    # and the float64 oracle at the exact rotations is the template oracle's mesh: one polynomial
    exact_p = po.forward(*args, rot=rot64)['vertices']
    exact_t = bo.forward(c64, coef, jo, np.float64)['mesh']
    assert np.abs(exact_p - exact_t).max() <= 1e-12
