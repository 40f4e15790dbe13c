"""Child process of tests/test_gpu_pose.py::test_chain_replays_from_one_captured_graph_and_agrees_with_the_standin_chain.

The graph is ``SMPLXParamDict.forward(packed=True)`` -> ``joint_transforms`` -> ``pose_features`` for the two frames of
the fixture, plus a weighted sum of the transforms and the posed joints.  Forward and backward are captured into one
``torch.cuda.graph`` after a warm-up on a side stream and replayed after the parameters are changed in place: every
output and every 6D gradient of the replay equals an eager run of the new parameters bit for bit, and all of them moved.

The eager gradients at the 6D leaves are then compared with the same graph whose first stage is the stand-in expression
(``matrix_to_axis_angle(rotation_6d_to_matrix(p))`` on the device, which no capture can pass: it reads boolean masks
back).  Both are float32 evaluations of one formula, so each may be off the float64 value by the allowance of
test_gpu_pose.py's float64 test -- 4x the error of the CPU float32 evaluation of the chain (tests/pose_oracle.py into
tests/kin_oracle.py), floored at 2^-24 of the largest gradient -- and their difference by the sum of the two.  Prints
``RESULT ok``."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import exavatar_release_amd as exa      # noqa: E402
from exavatar_release_amd import lbs      # noqa: E402
from tests import kin_oracle as ko      # noqa: E402
from tests import pose_oracle as po      # noqa: E402

DEV = 'cuda:0'
POSES = ('root_pose', 'body_pose', 'jaw_pose', 'leye_pose', 'reye_pose', 'lhand_pose', 'rhand_pose')
PARENTS = lbs.SMPLX_PARENTS
N_BODY = 21


def same(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def cpu_gradients(d6, joints, WT, WP, dtype):
    """dL/d(d6) [55, 6] of one frame through the oracles, L = sum(WT * transforms) + sum(WP * posed_joints)."""
    aa, _ = po.forward(d6, dtype)
    rot = ko.axis_angle_to_matrix(aa[None], dtype)
    grot, _, _ = ko.backward(rot, joints[None], PARENTS, None, WT[None], WP[None], dtype)
    gaa = ko.axis_angle_backward(aa[None], grot, dtype)[0]
    return po.backward(d6, gaa, dtype)


def main():
    golden = np.load(os.path.join(ROOT, 'tests', 'golden', 'ref_pose.npz'))
    frames = [int(f) for f in golden['frames']]
    names = sys.modules['exavatar_release_amd.pose_params'].PARAM_NAMES
    m = exa.SMPLXParamDict()
    m.init({f: {n: torch.from_numpy(golden['raw/%d/%s' % (f, n)]).float() for n in names} for f in frames})
    m = m.to(DEV)
    leaves = [m.smplx_params[str(f)][n] for f in frames for n in POSES]
    rs = np.random.RandomState(7)
    joints_np = (0.3 * rs.randn(55, 3)).astype(np.float32)
    WT_np, WP_np = rs.randn(2, 55, 4, 4).astype(np.float32), rs.randn(2, 55, 3).astype(np.float32)
    WT_np[:, :, 3, :] = 0                                 # row 3 of a transform is the constant (0, 0, 0, 1)
    joints, WT, WP = (torch.from_numpy(a).to(DEV) for a in (joints_np, WT_np, WP_np))

    def chain(poses):
        outs, loss = [], 0.0
        for k, pose in enumerate(poses):
            T, posed, rot = exa.joint_transforms(pose, joints, PARENTS)
            pose6d, pose_feat = exa.pose_features(rot, N_BODY)
            loss = loss + (T * WT[k]).sum() + (posed * WP[k]).sum()
            outs += [pose, T, posed, pose6d, pose_feat]
        return outs + [loss] + list(torch.autograd.grad(loss, leaves))

    def step():
        return chain([frame['pose'] for frame in m(frames, packed=True)])

    def standin_step():
        return chain([torch.cat([po.standin_expression(m.smplx_params[str(f)][n]).view(-1, 3) for n in POSES])
                      for f in frames])

    labels = ['%s[%d]' % (n, f) for f in frames for n in ('pose', 'transforms', 'posed', 'pose6d', 'pose_feat')] + \
        ['loss'] + ['grad %d/%s' % (f, n) for f in frames for n in POSES]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                           # warm up the allocator outside the capture
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    torch.cuda.synchronize()
    before = [t.clone() for t in static]
    with torch.no_grad():
        for p in leaves:
            new = p.cpu().numpy() * 0.9 + 0.05 * rs.randn(*p.shape)
            p.copy_(torch.from_numpy(new.astype(np.float32)).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in static]
    want = step()
    torch.cuda.synchronize()
    assert len(labels) == len(got)
    differ = [n for n, a, b in zip(labels, got, want) if not same(a, b)]
    assert differ == [], 'the replay differs from the eager run in %s' % differ
    stale = [n for n, a, b in zip(labels, got, before) if same(a, b)]
    assert stale == [], 'the replay left %s as captured' % stale

    # the eager gradients against the same graph behind the stand-in expression
    theirs = standin_step()
    torch.cuda.synchronize()
    n_out = len(labels) - len(leaves)
    worst = 0.0
    for k, f in enumerate(frames):
        d6 = np.concatenate([m.smplx_params[str(f)][n].detach().cpu().numpy().reshape(-1, 6) for n in POSES])
        g64 = cpu_gradients(d6, joints_np, WT_np[k], WP_np[k], np.float64)
        g32 = cpu_gradients(d6, joints_np, WT_np[k], WP_np[k], np.float32)
        side = max(4 * float(np.abs(g32.astype(np.float64) - g64).max()), 2.0 ** -24 * float(np.abs(g64).max()))
        lo = n_out + 7 * k
        ours = np.concatenate([t.cpu().numpy().reshape(-1, 6) for t in want[lo:lo + 7]]).astype(np.float64)
        ref = np.concatenate([t.cpu().numpy().reshape(-1, 6) for t in theirs[lo:lo + 7]]).astype(np.float64)
        assert np.isfinite(ours).all() and np.isfinite(ref).all()
        diff, e64 = float(np.abs(ours - ref).max()), float(np.abs(ours - g64).max())
        print('frame %d: |ours - stand-in| %.3e, |ours - float64| %.3e, one side\'s bound %.3e, max |grad| %.3e' % (
            f, diff, e64, side, float(np.abs(g64).max())))
        assert diff <= 2 * side, 'frame %d: %.3e between the two chains (bound %.3e)' % (f, diff, 2 * side)
        worst = max(worst, diff / (2 * side))
    print('RESULT ok: %d tensors equal the eager run, all of them new; stand-in chain within %.2f of the bound' % (
        len(got), worst))


if __name__ == '__main__':
    main()
