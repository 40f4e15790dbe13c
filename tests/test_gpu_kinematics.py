"""The HIP forward kinematics (exavatar_release_amd.joint_transforms / batch_rigid_transform) on the GPU.

From rotations, the transforms, the posed joints and every gradient (rotations, joints, pre) must equal the float32
oracle tests/kin_oracle.py BIT FOR BIT: the header fixes every rounding and the order of every sum.  From axis-angle the
same holds once the oracle is fed the kernel's own ``rot``; the trigonometric step itself -- the one place where the
device's sinf / cosf preclude bit equality with a CPU -- is held against float64 with an allowance derived from the CPU
float32 evaluation of the same formula: at most 4x that evaluation's own maximum error (a device library specified a
couple of ulp looser than libm, with two to spare), floored at one ulp of 1.0.  Against the reference's expression run
with torch on the device every element stays within the sum of both sides' first-order bounds.  Calls repeat bit for
bit, gradients that are not needed are skipped, a captured graph replays with a new pose and new joints, and the result
chains into skin_points with finite gradients at the all-zero pose."""
import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import lbs, p3d_standins
from tests import kin_oracle as ko

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
ULP1 = 2.0 ** -23
TREES = {'one': (-1,), 'smplx': lbs.SMPLX_PARENTS, 'chain': tuple(range(-1, 63)), 'star': (-1,) + (0,) * 63,
         'tree7': (-1, 0, 1, 1, 0, 4, 2)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b, what):
    bad = int((_bits(a) != _bits(b)).sum())
    assert a.shape == b.shape and bad == 0, '%s differs in %d of %d elements' % (what, bad, a.size)


def _case(tree, B, seed, pre=True):
    """CPU float32 tensors: pose with a zero row per skeleton, joints, pre (general matrices) and the cotangents."""
    J = len(TREES[tree])
    g = torch.Generator().manual_seed(seed)
    pose = 0.5 * torch.randn(B, J, 3, generator=g)
    pose[:, J // 2] = 0.0
    return {'pose': pose, 'joints': 0.3 * torch.randn(B, J, 3, generator=g),
            'pre': torch.randn(B, J, 4, 4, generator=g) if pre else None,
            'G': torch.randn(B, J, 4, 4, generator=g), 'Gp': torch.randn(B, J, 3, generator=g)}


def _run(c, tree, x=None, rotations=False, need=(True, True, True), cot=(True, True)):
    """joint_transforms on the device and its gradients for the cotangents (G, Gp); numpy results."""
    x = (c['pose'] if x is None else torch.as_tensor(x)).to(DEV).requires_grad_(need[0])
    joints = c['joints'].to(DEV).requires_grad_(need[1])
    pre = None if c['pre'] is None else c['pre'].to(DEV).requires_grad_(need[2])
    T, posed, rot = exa.joint_transforms(x, joints, TREES[tree], pre, rotations=rotations)
    assert not rot.requires_grad
    res = {'T': T.detach().cpu().numpy(), 'posed': posed.detach().cpu().numpy(), 'rot': rot.cpu().numpy()}
    inputs = [(n, t) for n, t, w in (('gx', x, need[0]), ('gjoints', joints, need[1]), ('gpre', pre, need[2]))
              if w and t is not None]
    outs = [(o, g.to(DEV)) for o, g, w in ((T, c['G'], cot[0]), (posed, c['Gp'], cot[1])) if w]
    if inputs and outs:
        grads = torch.autograd.grad([o for o, _ in outs], [t for _, t in inputs], [g for _, g in outs])
        res.update({n: g.cpu().numpy() for (n, _), g in zip(inputs, grads)})
    return res


def _n(x):
    return None if x is None else x.numpy()


def _oracle(c, tree, rot, cot=(True, True)):
    T, posed = ko.forward(rot, _n(c['joints']), TREES[tree], _n(c['pre']))
    grot, gj, gpre = ko.backward(rot, _n(c['joints']), TREES[tree], _n(c['pre']), _n(c['G']) if cot[0] else None,
                                 _n(c['Gp']) if cot[1] else None)
    return {'T': T, 'posed': posed, 'gx': grot, 'gjoints': gj, 'gpre': gpre}


SHAPES = [('one', 1, True), ('one', 2, False), ('smplx', 1, True), ('smplx', 1, False), ('chain', 1, True),
          ('star', 1, True), ('star', 2, False), ('smplx', 3, True), ('tree7', 3, False)]


@pytest.mark.parametrize('tree,B,pre', SHAPES)
def test_from_rotations_bit_exact(tree, B, pre):
    c = _case(tree, B, seed=11 * B + len(TREES[tree]), pre=pre)
    # rotations of the poses for the trees with a long path, general matrices elsewhere
    rot = (ko.axis_angle_to_matrix(c['pose'].numpy()) if tree in ('chain', 'smplx') else
           torch.randn(B, len(TREES[tree]), 3, 3, generator=torch.Generator().manual_seed(5)).numpy())
    got = _run(c, tree, rot, rotations=True)
    want = _oracle(c, tree, rot)
    _same(got['rot'], rot, 'rot (the copy of rot_in)')
    for k in ('T', 'posed', 'gx', 'gjoints') + (('gpre',) if pre else ()):
        _same(got[k], want[k], k)
    assert np.array_equal(got['T'][..., 3, :], c['pre'].numpy()[..., 3, :] if pre else
                          np.broadcast_to(np.float32([0, 0, 0, 1]), got['T'][..., 3, :].shape))


@pytest.mark.parametrize('tree,B,pre', [('smplx', 1, True), ('chain', 1, False), ('star', 3, True), ('one', 1, True)])
def test_from_axis_angle_bit_exact_given_the_kernels_own_rot(tree, B, pre):
    c = _case(tree, B, seed=7 * B + len(TREES[tree]), pre=pre)
    got = _run(c, tree)
    want = _oracle(c, tree, got['rot'])
    for k in ('T', 'posed', 'gjoints') + (('gpre',) if pre else ()):
        _same(got[k], want[k], k)
    assert got['gx'].shape == (B, len(TREES[tree]), 3) and np.isfinite(got['gx']).all()
    # the rotations path on the kernel's own rot gives the same bits, its own gradient included
    again = _run(c, tree, got['rot'], rotations=True)
    for k in ('T', 'posed', 'gjoints'):
        _same(again[k], got[k], k)
    _same(again['gx'], want['gx'], 'grad_rot')


def _trig_poses():
    """[3, 55, 3]: random poses; zero rows; angles just below and above the 1e-6 switch; angles near pi and beyond."""
    g = torch.Generator().manual_seed(31)
    pose = 0.7 * torch.randn(3, 55, 3, generator=g)
    axis = torch.nn.functional.normalize(torch.randn(55, 3, generator=g), dim=1)
    angles = torch.tensor([0.0, 0.5e-6, 0.99e-6, 1.01e-6, 2e-6, 1e-5, 1e-3, 3.14, 3.1415927, 3.15, 6.0])
    pose[1, :11] = angles[:, None] * axis[:11]
    pose[1, 23:25] = 0.0
    pose[2] *= 3.0
    return pose


def test_trigonometric_step_against_float64():
    c = _case('smplx', 3, seed=32)
    c['pose'] = _trig_poses()
    got = _run(c, 'smplx')
    pose64 = c['pose'].double()
    exact = ko.axis_angle_to_matrix(pose64.numpy(), np.float64)
    cpu32 = p3d_standins.axis_angle_to_matrix(c['pose']).numpy()
    err_dev = float(np.abs(got['rot'].astype(np.float64) - exact).max())
    err_cpu = float(np.abs(cpu32.astype(np.float64) - exact).max())
    print('rot: device max error %.3e, CPU float32 max error %.3e, ratio %.2f' % (err_dev, err_cpu, err_dev / err_cpu))
    # grad_pose for the cotangent the kernel itself applies: grad_rot of the chain on the kernel's own rot (bit-equal to
    # the oracle's, test above)
    grot = torch.from_numpy(_oracle(c, 'smplx', got['rot'])['gx'])
    p64 = pose64.clone().requires_grad_(True)
    (g64,) = torch.autograd.grad(p3d_standins.axis_angle_to_matrix(p64.view(-1, 3)), p64, grot.double().view(-1, 3, 3))
    p32 = c['pose'].clone().requires_grad_(True)
    (g32,) = torch.autograd.grad(p3d_standins.axis_angle_to_matrix(p32.view(-1, 3)), p32, grot.view(-1, 3, 3))
    assert np.isfinite(got['gx']).all() and np.isfinite(g64.numpy()).all()
    gerr_dev = float(np.abs(got['gx'].astype(np.float64) - g64.numpy()).max())
    gerr_cpu = float(np.abs(g32.numpy().astype(np.float64) - g64.numpy()).max())
    print('grad_pose: device max error %.3e, CPU float32 max error %.3e, ratio %.2f (max |grad| %.3e)' % (
        gerr_dev, gerr_cpu, gerr_dev / gerr_cpu, float(np.abs(g64.numpy()).max())))
    assert err_dev <= max(4 * err_cpu, ULP1), (err_dev, err_cpu)
    assert gerr_dev <= max(4 * gerr_cpu, ULP1), (gerr_dev, gerr_cpu)
    # the analytic Jacobian in float64 is the autograd of the stand-in (the zero rows included)
    assert np.abs(ko.axis_angle_backward(pose64.numpy(), grot.numpy(), np.float64) - g64.numpy()).max() <= \
        1e-9 * np.abs(g64.numpy()).max()


@pytest.mark.parametrize('tree,pre', [('smplx', True), ('chain', False)])
def test_against_the_reference_expression_on_the_device(tree, pre):
    parents = TREES[tree]
    J, D = len(parents), max(ko.depths(parents))
    c = _case(tree, 1, seed=41, pre=pre)
    rot = ko.axis_angle_to_matrix(c['pose'].numpy())
    got = _run(c, tree, rot, rotations=True)
    r = torch.from_numpy(rot[0]).to(DEV).requires_grad_(True)
    jt = c['joints'][0].to(DEV).requires_grad_(True)
    pr = c['pre'][0].to(DEV).requires_grad_(True) if pre else None
    T, posed, _ = ko.reference_expression(r, jt, parents, pr, rotations=True)
    grads = torch.autograd.grad([T, posed], [r, jt] + ([pr] if pre else []), [c['G'][0].to(DEV), c['Gp'][0].to(DEV)])
    mT, mposed, mrot, mj, mpre = ko.magnitudes(rot, _n(c['joints']), parents, _n(c['pre']), _n(c['G']), _n(c['Gp']))
    # both sides round the same operations (the reference's 4 x 4 products add exact zeros): twice the oracle's K
    kf, kb = 2 * ko.k_forward(D, pre), 2 * ko.k_backward(D, J, pre)
    pairs = [(got['T'], T, mT, kf), (got['posed'], posed, mposed, kf), (got['gx'], grads[0], mrot, kb),
             (got['gjoints'], grads[1], mj, kb)] + ([(got['gpre'], grads[2], mpre, kb)] if pre else [])
    for ours, theirs, mag, K in pairs:
        err = np.abs(ours[0].astype(np.float64) - theirs.detach().cpu().numpy().astype(np.float64))
        assert np.all(err <= K * ko.U * mag[0] + 1e-30), 'worst excess %g' % float((err - K * ko.U * mag[0]).max())


def test_repeated_calls_give_identical_bits():
    c = _case('smplx', 3, seed=51)
    first = _run(c, 'smplx')
    for _ in range(3):
        again = _run(c, 'smplx')
        for k in first:
            _same(again[k], first[k], k)


def test_partial_gradients_and_missing_cotangents():
    c = _case('smplx', 2, seed=61)
    full = _run(c, 'smplx')
    only_joints = _run(c, 'smplx', need=(False, True, False))
    assert 'gx' not in only_joints and 'gpre' not in only_joints
    _same(only_joints['gjoints'], full['gjoints'], 'grad_joints alone')
    only_pose = _run(c, 'smplx', need=(True, False, False))
    _same(only_pose['gx'], full['gx'], 'grad_pose alone')
    # a missing cotangent counts as zero
    for cot in ((True, False), (False, True)):
        got = _run(c, 'smplx', cot=cot)
        want = _oracle(c, 'smplx', got['rot'], cot=cot)
        for k in ('gjoints', 'gpre'):
            _same(got[k], want[k], '%s with cotangents %s' % (k, cot))
    assert not _run(c, 'smplx', cot=(False, True))['gpre'].any(), 'posed_joints do not depend on pre'


def test_shapes_broadcast_and_the_smplx_signature():
    c = _case('tree7', 3, seed=71, pre=False)
    parents = TREES['tree7']
    rot = torch.randn(3, 7, 3, 3, generator=torch.Generator().manual_seed(72)).to(DEV).requires_grad_(True)
    joints = c['joints'].to(DEV).requires_grad_(True)
    posed, rel = exa.batch_rigid_transform(rot, joints, torch.tensor(parents))
    want = _oracle(c, 'tree7', rot.detach().cpu().numpy())
    _same(posed.detach().cpu().numpy(), want['posed'], 'posed_joints')
    _same(rel.detach().cpu().numpy(), want['T'], 'rel_transforms')
    grot, gj = torch.autograd.grad([rel, posed], [rot, joints], [c['G'].to(DEV), c['Gp'].to(DEV)])
    _same(grot.cpu().numpy(), want['gx'], 'grad rot_mats')
    _same(gj.cpu().numpy(), want['gjoints'], 'grad joints')
    # no batch axis anywhere: none on the results
    T, p, r = exa.joint_transforms(c['pose'][0].to(DEV), c['joints'][0].to(DEV), parents)
    assert T.shape == (7, 4, 4) and p.shape == (7, 3) and r.shape == (7, 3, 3)
    # joints shared by the batch: every skeleton sees them, their gradient is the sum over the batch
    shared = c['joints'][0].to(DEV).requires_grad_(True)
    pose = c['pose'].to(DEV)
    T, p, _ = exa.joint_transforms(pose, shared, parents)
    (gs,) = torch.autograd.grad([T, p], [shared], [c['G'].to(DEV), c['Gp'].to(DEV)])
    rep = shared.detach()[None].repeat(3, 1, 1).requires_grad_(True)
    T2, p2, _ = exa.joint_transforms(pose, rep, parents)
    (gr,) = torch.autograd.grad([T2, p2], [rep], [c['G'].to(DEV), c['Gp'].to(DEV)])
    _same(T.detach().cpu().numpy(), T2.detach().cpu().numpy(), 'transforms with shared joints')
    # (torch adds the three skeletons' gradients in an order of its own: two additions, 2 u of the terms' magnitudes)
    per = gr.double().cpu().numpy()
    assert np.all(np.abs(gs.double().cpu().numpy() - per.sum(0)) <= 2 * ko.U * np.abs(per).sum(0) + 1e-30)


def test_graph_capture_replays_with_a_new_pose_and_new_joints():
    c = _case('smplx', 1, seed=81)
    pose = c['pose'].to(DEV).clone().requires_grad_(True)
    joints = c['joints'].to(DEV).clone().requires_grad_(True)
    pre = c['pre'].to(DEV).requires_grad_(True)
    G, Gp = c['G'].to(DEV), c['Gp'].to(DEV)

    def step():
        T, posed, rot = exa.joint_transforms(pose, joints, lbs.SMPLX_PARENTS, pre)
        return (T, posed, rot), torch.autograd.grad([T, posed], [pose, joints, pre], [G, Gp])

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs, grads = step()
    new = _case('smplx', 1, seed=82)
    with torch.no_grad():
        pose.copy_(new['pose'].to(DEV))
        joints.copy_(new['joints'].to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    ref = _run(dict(c, pose=new['pose'], joints=new['joints']), 'smplx')
    for a, k in zip(list(outs) + list(grads), ('T', 'posed', 'rot', 'gx', 'gjoints', 'gpre')):
        _same(a.detach().cpu().numpy(), ref[k], k + ' after the replay')


def test_chain_into_skin_points_is_finite_at_the_all_zero_pose():
    J, V = 55, 300
    g = torch.Generator().manual_seed(91)
    joints = (0.3 * torch.randn(J, 3, generator=g)).to(DEV).requires_grad_(True)
    W = torch.zeros(V, J)
    W.scatter_(1, torch.argsort(torch.rand(V, J, generator=g), 1)[:, :4], torch.softmax(torch.randn(V, 4, generator=g), 1))
    pts = torch.randn(V, 3, generator=g).to(DEV)
    for scale in (0.0, 0.3):
        pose = (scale * torch.randn(J, 3, generator=g)).to(DEV).requires_grad_(True)
        T, posed, rot = exa.joint_transforms(pose, joints, lbs.SMPLX_PARENTS)
        (out,) = exa.skin_points(pts, T, W.to(DEV))
        gpose, gjoints = torch.autograd.grad(out.sum() + posed.sum(), [pose, joints])
        assert torch.isfinite(gpose).all() and torch.isfinite(gjoints).all()
        assert float(gpose.abs().max()) > 0 and float(gjoints.abs().max()) > 0
        if scale == 0.0:      # the identity pose leaves the points where they are
            assert float((out - pts).abs().max()) <= 1e-5
