"""The forward kinematics on the MI355X at the reference shape (J = 55, the SMPL-X tree, B = 1, with the big-pose
transforms ``pre``): pose -> transform_mat_joint, forward and forward + backward (gradients for pose, joints and pre),
eager and replayed from a captured graph, of

  seq     the sequential restatement of the reference (p3d_standins.axis_angle_to_matrix, one 4x4 matmul per joint,
          parents before children, the rest location removed, bmm with pre: tests/kin_oracle.reference_expression);
  level   lbs.joint_transforms, the per-level torch version (eleven batched matmuls), with the same axis-angle step and
          the same bmm;
  hip     exavatar_release_amd.joint_transforms (one launch each way).

The captured baselines use lbs.axis_angle_to_matrix (Rodrigues) for the axis-angle step: pytorch3d's, which the eager
ones run, picks the small angles with a boolean mask and cannot be captured.

Per-call medians over interleaved windows (tools/_timing.medians), the min / max of the windows next to them, and the
max abs difference of the three forwards.  Prints one JSON line; --out writes it to a file too.

    python tools/gpu_kin_times.py [--reps 15] [--iters 20] [--out kin_times.json]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import exavatar_release_amd as exa                              # noqa: E402
from exavatar_release_amd import build, lbs, p3d_standins       # noqa: E402
from tests import kin_oracle                                    # noqa: E402
from _timing import emit, medians                               # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_kin_times.py needs a ROCm device')
    dev = torch.device('cuda:0')
    J, parents = 55, lbs.SMPLX_PARENTS
    gen = torch.Generator().manual_seed(3)
    pose = (0.4 * torch.randn(J, 3, generator=gen)).to(dev).requires_grad_(True)
    joints = (0.3 * torch.randn(J, 3, generator=gen)).to(dev).requires_grad_(True)
    with torch.no_grad():
        pre = torch.linalg.inv(exa.joint_transforms(0.3 * torch.randn(J, 3, generator=gen).to(dev), joints, parents)[0])
    pre = pre.contiguous().requires_grad_(True)
    G = torch.randn(J, 4, 4, generator=gen).to(dev)
    inputs = [pose, joints, pre]

    def seq(aa=p3d_standins.axis_angle_to_matrix):
        return kin_oracle.reference_expression(aa(pose), joints, parents, pre, rotations=True)[0]

    def level(aa=p3d_standins.axis_angle_to_matrix):
        return torch.bmm(lbs.joint_transforms(aa(pose), joints, parents), pre)

    def hip():
        return exa.joint_transforms(pose, joints, parents, pre)[0]

    def fwd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def fwd_bwd(f):
        return lambda: torch.autograd.grad(f(), inputs, G)

    def graphed(fn):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        return graph.replay

    # the stand-in's axis-angle step (pytorch3d's) selects the small angles with a boolean mask, which synchronises and
    # cannot be captured: the captured baselines take lbs.axis_angle_to_matrix (Rodrigues, mask-free) in its place
    variants = {'seq': seq, 'level': level, 'hip': hip}
    capturable = {'seq': lambda: seq(lbs.axis_angle_to_matrix), 'level': lambda: level(lbs.axis_angle_to_matrix), 'hip': hip}
    fns = {}
    for name, f in variants.items():
        fns[name + '_fwd_eager'] = fwd(f)
        fns[name + '_fwd_bwd_eager'] = fwd_bwd(f)
    for name, f in capturable.items():
        fns[name + '_fwd_graph'] = graphed(fwd(f))
        fns[name + '_fwd_bwd_graph'] = graphed(fwd_bwd(f))
    med, spread = medians(fns, args.reps, args.iters)
    res = {'build_digest': build._digest()[:12], 'device': torch.cuda.get_device_name(0), 'J': J, 'B': 1, 'pre': True,
           'reps': args.reps, 'iters': args.iters}
    for k in fns:
        res[k + '_ms'] = med[k]
        res[k + '_min_max_ms'] = list(spread[k])
    with torch.no_grad():
        a, b, c = seq(), level(), hip()
        res['fwd_max_abs_diff_hip_vs_seq'] = float((c - a).abs().max())
        res['fwd_max_abs_diff_level_vs_seq'] = float((b - a).abs().max())
    emit(res, args.out)


if __name__ == '__main__':
    main()
