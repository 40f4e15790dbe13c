"""CPU tests of the SMPL-X template stage's restatement (tests/body_oracle.py) against the reference's own run
(tests/golden/ref_body.npz, written by tests/golden/make_golden_body.py), of the pose constants ``BodyTemplate.from_layer``
computes, and of the host planner of ``MeshUpsampler`` against the chained ``SubdivideMeshes`` stand-in."""
import os
import types

import numpy as np
import pytest
import torch

import body_oracle as bo
import human_case
import exavatar_release_amd as exa
from exavatar_release_amd import body, p3d_standins as p3d

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_body.npz')
U64 = 2.0 ** -53


@pytest.fixture(scope='module')
def golden():
    case, coef, jo, cot = bo.golden_inputs()
    ref = dict(np.load(GOLDEN))
    return types.SimpleNamespace(case=case, coef=coef, jo=jo, cot=cot, ref=ref)


def _with_constants(g, dtype):
    """The fixture's case with the reference's three pose constants, as float64 or rounded to float32."""
    return dict(g.case, **{k: g.ref[k].astype(dtype) for k in ('rot_pose', 'rot_inverse', 'pose_offsets')})


def _reference(g):
    ref = {k: g.ref[k] for k in bo.OUTPUTS}
    ref.update(coef=g.ref['grad_coef'], joint_offset=g.ref['grad_joint_offset'])
    return ref


def test_the_fixture_was_made_from_these_inputs(golden):
    want = dict(zip(golden.ref['digest_names'].tolist(), golden.ref['digest_values'].tolist()))
    assert bo.golden_digests(golden.case, golden.coef, golden.jo, golden.cot) == want
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_float64_oracle_agrees_with_the_reference(golden):
    """Both sides evaluate the same polynomials in float64 in different orders: each is within K u64 of the exact value
    times the monomials' magnitudes, K the fp32 analysis' count (the orders differ, the depths do not grow)."""
    case = _with_constants(golden, np.float64)
    ex = bo.exact(case, golden.coef, golden.jo, golden.cot)
    for name, ref in _reference(golden).items():
        val, E32 = ex[name]
        assert val.shape == ref.shape, name
        bound = 2 * E32 * (U64 / bo.U)
        err = np.abs(val - ref)
        print(name, 'max |oracle64 - reference|', err.max(), 'max bound', bound.max())
        assert (err <= bound).all(), name
        assert err.max() <= 1e-9 * max(np.abs(ref).max(), 1.0), name      # "closely": nothing like a wrong term hides here


def test_float32_oracle_is_within_its_bound_of_the_reference(golden):
    """The constants are the reference's rounded to float32: a monomial holds at most D + 1 rotations of chain A, as many
    of chain B and one pose offset, each carrying one rounding more."""
    D = max(bo.kin_oracle.depths(list(golden.case['parents'])))
    extra = 2 * (D + 1) + 1
    case = _with_constants(golden, np.float32)
    fwd = bo.forward(case, golden.coef, golden.jo)
    dcoef, djo = bo.backward(case, fwd, golden.cot)
    got = dict(fwd, coef=dcoef, joint_offset=djo)
    ex = bo.exact(_with_constants(golden, np.float64), golden.coef, golden.jo, golden.cot, extra)
    for name, ref in _reference(golden).items():
        assert got[name].dtype == np.float32
        err = np.abs(got[name].astype(np.float64) - ref)
        bound = ex[name][1] * (1 + 2 * U64 / bo.U)
        print(name, 'max |oracle32 - reference|', err.max(), 'max bound', bound.max())
        assert (err <= bound).all(), name


def test_from_layer_constants_are_within_a_rounding_of_the_reference(golden):
    """``pose_constants`` evaluates the reference's expressions in float64 and rounds once: u |x| for that rounding,
    plus the float64 evaluations' own error -- at most 64 roundings of values below 2 for a rotation by Rodrigues'
    formula, 512 for the route through the inverse, the quaternion and back, and 9 (J - 1) + 64 of the products'
    magnitudes for the pose offsets."""
    c = golden.case
    t = torch.from_numpy
    layer = types.SimpleNamespace(v_template=t(c['v_template']), shapedirs=t(c['shape_dirs']), expr_dirs=None,
                                  posedirs=t(c['posedirs']), J_regressor=t(c['J_regressor']), lbs_weights=t(c['weights']),
                                  parents=torch.tensor(list(c['parents'])))
    tpl = exa.BodyTemplate.from_layer(layer, c['faces'], t(c['pose']), face_offset=t(c['face_offset']))
    assert tpl.state_dict() == {} and tpl.upsampler.num_verts == 10242
    feat = np.abs(golden.ref['rot_pose'][1:] - np.eye(3)).reshape(1, -1)
    noise = dict(rot_pose=64 * U64 * 2, rot_inverse=512 * U64 * 2,
                 pose_offsets=(9 * 54 + 64) * U64 * (feat @ np.abs(c['posedirs'].astype(np.float64))).reshape(-1, 3))
    for name in ('rot_pose', 'rot_inverse', 'pose_offsets'):
        got, ref = getattr(tpl, name).numpy().astype(np.float64), golden.ref[name]
        err = np.abs(got - ref)
        bound = bo.U * np.abs(ref) + noise[name]
        print(name, 'max err', err.max(), 'max bound', np.max(bound))
        assert (err <= bound).all(), name
    rot, off, inv = body.pose_constants(t(c['pose']))
    assert off is None and torch.equal(rot, tpl.rot_pose) and torch.equal(inv, tpl.rot_inverse)


MESHES = {'triangle': bo.triangle, 'grid5x7': lambda: bo.grid(5, 7), 'icosphere2': lambda: human_case._icosphere(2),
          'icosphere3': lambda: human_case._icosphere(3)}


@pytest.mark.parametrize('mesh', sorted(MESHES))
@pytest.mark.parametrize('levels', [1, 2])
def test_upsampler_topology_is_the_chained_stand_ins(mesh, levels):
    verts, faces = MESHES[mesh]()
    m = p3d.Meshes(torch.from_numpy(verts)[None].float(), torch.from_numpy(faces)[None])
    for _ in range(levels):
        m = p3d.SubdivideMeshes(m)(m)
    up = exa.MeshUpsampler(faces, levels)
    assert up.num_verts == m.verts_padded().shape[1]
    assert up.faces.dtype == torch.int64 and torch.equal(up.faces, m.faces_padded()[0])
    assert up.state_dict() == {}
    if mesh == 'triangle':
        assert (up.num_coarse, up.num_mid, up.num_verts) == ((3, 6, 15) if levels == 2 else (3, 6, 6))
    # the flat plan and the dependants' lists against the oracle's own subdivision
    pl = bo.plan(faces, verts.shape[0], levels)
    assert pl['V'][-1] == up.num_verts and np.array_equal(pl['faces'], up.faces.numpy())
    assert np.array_equal(np.concatenate([e for _, e in pl['rounds']], 0), up._par.numpy())
    for (Vc, edges), off, dep in zip(pl['rounds'], (up._off1, up._off2), (up._dep1, up._dep2)):
        off, dep = off.numpy(), dep.numpy()
        assert off[0] == 0 and off[-1] == 2 * edges.shape[0] == dep.size
        for p in range(Vc):
            want = [Vc + e for e in range(edges.shape[0]) for s in (0, 1) if edges[e, s] == p] if Vc <= 64 else None
            seg = dep[off[p]:off[p + 1]]
            assert (np.diff(seg) >= 0).all() and (edges[seg - Vc] == p).any(1).all()
            if want is not None:
                assert seg.tolist() == want
