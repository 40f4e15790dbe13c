"""GPU tests of the SMPL-X template stage (exavatar_release_amd/body.py, csrc/body.hip, include/exa_mesh.h
exa_mesh_body_* / exa_mesh_upsample_*).

The five outputs and both gradients are held to tests/body_oracle.py bit for bit -- nothing in the stage runs a
transcendental on the device -- over the sizes at which the kernels take another path: one vertex block and two (256,
257), one chunk of dL/dcoef and several, L below and above the eight rows a thread keeps in flight and above a
workgroup's staging pass (150 < 256 < 512), one joint, the SMPL-X tree and the 64-joint chain and star, one round and
two, open and closed meshes, regressor rows that are empty, single and dense (more than 64 non-zeros: the lanes loop),
with and without the two offset tables, and every pattern of missing cotangents.  Then ``MeshUpsampler.up`` alone, the
reference's own float64 run (tests/golden/ref_body.npz) within the derived bounds, reproducibility, poisoned workspaces,
a captured graph, and the outputs chained into the stages that consume them."""
import itertools
import os
import types

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import lbs, p3d_standins as p3d
from tests import body_oracle as bo
from tests import human_case

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_body.npz')
TREE7 = (-1, 0, 1, 1, 0, 4, 2)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b, what):
    assert a.shape == b.shape, what
    bad = int((_bits(a) != _bits(b)).sum())
    assert bad == 0, '%s differs in %d of %d elements' % (what, bad, a.size)


def _icosphere(level):
    verts, faces = human_case._icosphere(level)
    return verts * np.asarray(human_case.RADII), faces


def _template(case):
    """The module over a case's arrays, on the device."""
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    up = exa.MeshUpsampler(case['faces'], case['levels'], num_verts=case['v_template'].shape[0]).to(DEV)
    return exa.BodyTemplate(t(case['v_template']), t(case['shape_dirs']), t(case['J_regressor']), t(case['weights']),
                            list(case['parents']), up, rot_pose=t(case['rot_pose']), rot_inverse=t(case['rot_inverse']),
                            pose_offsets=t(case['pose_offsets']), face_offset=t(case['face_offset']),
                            root_joint_idx=case['root'])


def _run(tpl, coef, jo, cot, need=(True, True)):
    """The module's outputs and gradients as numpy arrays: {output: array, 'coef': .., 'joint_offset': ..}."""
    c = torch.from_numpy(coef).to(DEV).requires_grad_(need[0])
    j = torch.from_numpy(jo).to(DEV).requires_grad_(need[1])
    out = tpl(c, j)
    assert isinstance(out, exa.BodyOutput)
    res = {k: o.detach().cpu().numpy() for k, o in zip(bo.OUTPUTS, out)}
    present = [(o, torch.from_numpy(cot[k]).to(DEV)) for k, o in zip(bo.OUTPUTS, out) if cot.get(k) is not None]
    inputs = [(n, x) for n, x, w in (('coef', c, need[0]), ('joint_offset', j, need[1])) if w]
    if present and inputs:
        grads = torch.autograd.grad([o for o, _ in present], [x for _, x in inputs], [g for _, g in present])
        res.update({n: g.cpu().numpy() for (n, _), g in zip(inputs, grads)})
    return res


def _oracle(case, coef, jo, cot, want_coef=True):
    fwd = bo.forward(case, coef, jo)
    dcoef, djo = bo.backward(case, fwd, cot, want_coef=want_coef)
    res = {k: fwd[k] for k in bo.OUTPUTS}
    res.update(coef=dcoef, joint_offset=djo)
    return res


# name: (mesh, L, parents, rounds, regressor, offset tables, root)
CASES = {
    'triangle-L1-J1': (bo.triangle, 1, (-1,), 2, 'sparse', True, 0),
    'grid256-L7-smplx-1round': (lambda: bo.grid(16, 16), 7, lbs.SMPLX_PARENTS, 1, 'sparse', False, 0),
    'strip257-L150-chain64': (lambda: bo.strip(257), 150, bo.chain_tree(64), 2, 'rows', True, 2),
    'icosphere642-L100-smplx': (lambda: _icosphere(3), 100, lbs.SMPLX_PARENTS, 2, 'sparse', True, 0),
    'grid35-L7-star64': (lambda: bo.grid(5, 7), 7, bo.star_tree(64), 2, 'rows', False, 3),
    'icosphere162-L100-smplx-1round': (lambda: _icosphere(2), 100, lbs.SMPLX_PARENTS, 1, 'rows', True, 0),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_bit_exact_against_the_oracle(name):
    mesh, L, parents, levels, regressor, offsets, root = CASES[name]
    verts, faces = mesh()
    case, coef, jo = bo.random_case(verts, faces, L, parents, levels, 31, regressor, offsets, root)
    cot = bo.random_cotangents(case, 32)
    got, want = _run(_template(case), coef, jo, cot), _oracle(case, coef, jo, cot)
    for k in bo.OUTPUTS + ('coef', 'joint_offset'):
        _same(got[k], want[k], '%s: %s' % (name, k))
    assert (_bits(got['joint_offset'][root]) == 0).all()      # +0.0, not -0.0


def test_every_pattern_of_missing_cotangents_bit_exact():
    verts, faces = bo.grid(5, 7)
    case, coef, jo = bo.random_case(verts, faces, 7, TREE7, 2, 41, 'rows')
    tpl = _template(case)
    full = bo.random_cotangents(case, 42)
    for mask in itertools.product((False, True), repeat=5):
        if not any(mask):
            continue
        cot = {k: full[k] if m else None for k, m in zip(bo.OUTPUTS, mask)}
        got, want = _run(tpl, coef, jo, cot), _oracle(case, coef, jo, cot)
        for k in ('coef', 'joint_offset'):
            _same(got[k], want[k], '%s with cotangents %s' % (k, mask))


def test_unneeded_gradients_are_skipped():
    verts, faces = bo.strip(257)
    case, coef, jo = bo.random_case(verts, faces, 20, TREE7, 2, 51)
    tpl, cot = _template(case), bo.random_cotangents(case, 52)
    both = _run(tpl, coef, jo, cot)
    only_coef, only_jo, neither = (_run(tpl, coef, jo, cot, need) for need in ((True, False), (False, True), (False, False)))
    assert 'joint_offset' not in only_coef and 'coef' not in only_jo and not {'coef', 'joint_offset'} & set(neither)
    _same(only_coef['coef'], both['coef'], 'dL/dcoef alone')
    _same(only_jo['joint_offset'], both['joint_offset'], 'dL/djoint_offset alone')
    _same(only_jo['joint_offset'], _oracle(case, coef, jo, cot, want_coef=False)['joint_offset'], 'against the oracle')
    # the batch axes of the reference's Parameters ([1, L], [1, J, 3]) are accepted and come back in the gradients
    c = torch.from_numpy(coef).to(DEV)[None].requires_grad_(True)
    j = torch.from_numpy(jo).to(DEV)[None].requires_grad_(True)
    out = tpl(c, j)
    gc, gj = torch.autograd.grad(list(out), [c, j], [torch.from_numpy(cot[k]).to(DEV) for k in bo.OUTPUTS])
    assert gc.shape == c.shape and gj.shape == j.shape
    _same(gc[0].cpu().numpy(), both['coef'], 'dL/dcoef of [1, L]')
    _same(gj[0].cpu().numpy(), both['joint_offset'], 'dL/djoint_offset of [1, J, 3]')


@pytest.mark.parametrize('C', [1, 3, 8])
@pytest.mark.parametrize('mesh,levels', [('grid5x7', 2), ('icosphere2', 2), ('strip257', 1)])
def test_upsampler_alone(mesh, levels, C):
    verts, faces = {'grid5x7': lambda: bo.grid(5, 7), 'icosphere2': lambda: _icosphere(2),
                    'strip257': lambda: bo.strip(257)}[mesh]()
    rng = np.random.RandomState(61)
    V0 = verts.shape[0]
    x = rng.standard_normal((V0, C)).astype(np.float32)
    up = exa.MeshUpsampler(torch.from_numpy(faces).to(DEV), levels, num_verts=V0)      # a device tensor of faces
    assert up.faces.device.type == 'cuda'
    xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
    out = up.up(xd)
    # the two-pass stand-in on the CPU, through its feature path (any channel count)
    m, feats = p3d.Meshes(torch.from_numpy(verts)[None].float(), torch.from_numpy(faces)[None]), torch.from_numpy(x)
    for _ in range(levels):
        sub = p3d.SubdivideMeshes(m)
        m, feats = sub(m, feats)
        feats = feats[0]
    _same(out.detach().cpu().numpy(), feats.numpy(), 'up(vert), C = %d' % C)
    pl = bo.plan(faces, V0, levels)
    _same(out.detach().cpu().numpy(), bo.up_forward(x, pl), 'up(vert) against the oracle')
    g = rng.standard_normal(tuple(out.shape)).astype(np.float32)
    (dx,) = torch.autograd.grad(out, xd, torch.from_numpy(g).to(DEV))
    _same(dx.cpu().numpy(), bo.up_backward(g, pl), 'dL/dvert, C = %d' % C)
    (dx2,) = torch.autograd.grad(up(xd), xd, torch.from_numpy(g).to(DEV))
    assert torch.equal(dx, dx2)


@pytest.fixture(scope='module')
def golden():
    case, coef, jo, cot = bo.golden_inputs()
    ref = dict(np.load(GOLDEN))
    c32 = dict(case, **{k: ref[k].astype(np.float32) for k in ('rot_pose', 'rot_inverse', 'pose_offsets')})
    c64 = dict(case, **{k: ref[k] for k in ('rot_pose', 'rot_inverse', 'pose_offsets')})
    return types.SimpleNamespace(case=c32, case64=c64, coef=coef, jo=jo, cot=cot, ref=ref)


def test_against_the_references_own_run(golden):
    """Every element within the first-order bound of the fp32 evaluation (tests/body_oracle.exact; the constants are the
    reference's rounded to float32: 2 (D + 1) + 1 roundings more per monomial), no element excluded; the gradients
    within that plus the float64 side's own bound (the same count at u = 2^-53)."""
    D = max(bo.kin_oracle.depths(list(golden.case['parents'])))
    ex = bo.exact(golden.case64, golden.coef, golden.jo, golden.cot, 2 * (D + 1) + 1)
    got = _run(_template(golden.case), golden.coef, golden.jo, golden.cot)
    ref = {k: golden.ref[k] for k in bo.OUTPUTS}
    ref.update(coef=golden.ref['grad_coef'], joint_offset=golden.ref['grad_joint_offset'])
    for k in bo.OUTPUTS + ('coef', 'joint_offset'):
        err = np.abs(got[k].astype(np.float64) - ref[k])
        bound = ex[k][1] * (1 + 2.0 ** -53 / bo.U)
        print(k, 'max |hip - reference|', err.max(), 'max bound', bound.max(), 'max err / bound', (err / np.maximum(bound, 1e-300)).max())
        assert np.isfinite(got[k]).all() and (err <= bound).all(), k
    # and the fp32 oracle over the same constants, bit for bit
    want = _oracle(golden.case, golden.coef, golden.jo, golden.cot)
    for k in bo.OUTPUTS + ('coef', 'joint_offset'):
        _same(got[k], want[k], k)


def test_repeated_calls_and_poisoned_workspaces_give_identical_bits(golden):
    tpl = _template(golden.case)
    first = _run(tpl, golden.coef, golden.jo, golden.cot)
    second = _run(tpl, golden.coef, golden.jo, golden.cot)
    exa.config.poison = True
    poisoned = _run(tpl, golden.coef, golden.jo, golden.cot)
    only_up = {k: golden.cot[k] if k == 'mesh_upsampled' else None for k in bo.OUTPUTS}
    poisoned_up = _run(tpl, golden.coef, golden.jo, only_up)
    exa.config.poison = False
    for k in first:
        _same(first[k], second[k], k + ' on the second call')
        _same(first[k], poisoned[k], k + ' with poisoned workspaces')
    plain_up = _run(tpl, golden.coef, golden.jo, only_up)
    for k in ('coef', 'joint_offset'):
        _same(plain_up[k], poisoned_up[k], k + ' from mesh_upsampled alone, poisoned')


def test_graph_capture_replays_with_new_inputs():
    verts, faces = _icosphere(2)
    case, coef, jo = bo.random_case(verts, faces, 100, lbs.SMPLX_PARENTS, 2, 71)
    cot = bo.random_cotangents(case, 72)
    tpl = _template(case)
    c = torch.from_numpy(coef).to(DEV).clone().requires_grad_(True)
    j = torch.from_numpy(jo).to(DEV).clone().requires_grad_(True)
    G = [torch.from_numpy(cot[k]).to(DEV) for k in bo.OUTPUTS]

    def step():
        out = tpl(c, j)
        return out, torch.autograd.grad(list(out), [c, j], G)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, grads = step()
    _, coef2, jo2 = bo.random_case(verts, faces, 100, lbs.SMPLX_PARENTS, 2, 73)
    with torch.no_grad():
        c.copy_(torch.from_numpy(coef2).to(DEV))
        j.copy_(torch.from_numpy(jo2).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    eager = _run(tpl, coef2, jo2, cot)
    for k, a in zip(bo.OUTPUTS + ('coef', 'joint_offset'), list(out) + list(grads)):
        _same(a.detach().cpu().numpy(), eager[k], k + ' after the replay')
    assert (_bits(eager['mesh']) != _bits(_run(tpl, coef, jo, cot)['mesh'])).any()      # the inputs did change


def test_outputs_chain_into_the_stages_that_consume_them(golden):
    """``joint_zero_pose`` and ``transform_mat_neutral_pose`` feed ``joint_transforms``,
    ``mesh_upsampled`` the nearest-vertex search and the points that ``skin_points`` poses.  A scalar loss then reaches
    ``coef`` and ``joint_offset``: finite, the same bits on two runs, and within the two sides' bounds of the reference's
    torch expression of the stage on the device, fed the cotangents that the same downstream stages hand back (both
    sides evaluate the same polynomials of the inputs and those cotangents in fp32, in different orders; each is within
    tests/body_oracle.exact's first-order bound of the exact value; the module is built by ``from_layer``, whose
    constants are the expression's rounded once)."""
    c = golden.case
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    layer = types.SimpleNamespace(v_template=t(c['v_template']), shapedirs=t(c['shape_dirs']), expr_dirs=None,
                                  posedirs=t(c['posedirs']), J_regressor=t(c['J_regressor']), lbs_weights=t(c['weights']),
                                  parents=torch.tensor(list(c['parents'])))
    tpl = exa.BodyTemplate.from_layer(layer, c['faces'], t(c['pose']), face_offset=t(c['face_offset']))
    parents = list(c['parents'])
    V = c['v_template'].shape[0]
    weights_up = t(bo.up_forward(c['weights'], bo.plan(c['faces'], V, 2)))            # what init() upsamples once
    rng = np.random.RandomState(81)
    pose = t((0.3 * rng.standard_normal((55, 3))).astype(np.float32))
    offset = t((0.002 * rng.standard_normal((tpl.upsampler.num_verts, 3))).astype(np.float32))
    G = t(rng.standard_normal((tpl.upsampler.num_verts, 3)).astype(np.float32))

    def downstream(out):
        T, _, _ = exa.joint_transforms(pose, out[4], parents, out[3])
        mean_3d = out[0] + offset
        idx = exa.knn_points(mean_3d[None].detach(), out[0][None].detach(), K=1).idx[0, :, 0]
        (posed,) = exa.skin_points(mean_3d, T, weights_up, idx)
        return (posed * G).sum() + out[1].sum() * 0.5 + out[2].sum() * 0.25

    def run():
        coef = t(golden.coef).requires_grad_(True)
        jo = t(golden.jo).requires_grad_(True)
        out = tpl(coef, jo)
        loss = downstream(out)
        cots = torch.autograd.grad(loss, list(out), retain_graph=True)
        return out, cots, torch.autograd.grad(loss, [coef, jo])

    out, cots, (gc, gj) = run()
    _, _, (gc2, gj2) = run()
    assert torch.isfinite(gc).all() and torch.isfinite(gj).all() and float(gc.abs().max()) > 0 and float(gj.abs().max()) > 0
    assert torch.equal(gc, gc2) and torch.equal(gj, gj2)
    # the torch expression of the stage on the device, over the same cotangents
    ct = {k: t(c[k]) for k in ('v_template', 'face_offset', 'shape_dirs', 'J_regressor', 'weights', 'pose', 'posedirs')}
    ct.update(parents=parents, root=c['root'], rot_inverse=tpl.rot_inverse)
    subs = [s.to(DEV) for s in bo.stand_in_subdividers(c['v_template'], c['faces'], 2)]
    coef, jo = t(golden.coef).requires_grad_(True), t(golden.jo).requires_grad_(True)
    ref_out = bo.reference_expression(ct, coef, jo, subs)
    rc, rj = torch.autograd.grad(list(ref_out), [coef, jo], [g.detach() for g in cots])
    cot = {k: g.detach().cpu().numpy() for k, g in zip(bo.OUTPUTS, cots)}
    # the constants' own roundings per monomial (at most D + 1 rotations of chain A, as many of chain B, one pose offset):
    # one each on the module's side; on torch's side Rodrigues' formula in fp32 (at most 12 roundings per entry) and the
    # 486-term corrective product
    D = max(bo.kin_oracle.depths(parents))
    hip = bo.exact(golden.case64, golden.coef, golden.jo, cot, 2 * (D + 1) + 1)
    ref = bo.exact(golden.case64, golden.coef, golden.jo, cot, 13 * (D + 1) + 9 * 54 + 12)
    for k, a, b in zip(bo.OUTPUTS + ('coef', 'joint_offset'), list(out) + [gc, gj], list(ref_out) + [rc, rj]):
        err = (a.detach().double() - b.detach().double()).abs().cpu().numpy()
        bound = hip[k][1] + ref[k][1]
        print(k, 'max |hip - torch|', err.max(), 'max bound', bound.max())
        assert (err <= bound).all(), k
