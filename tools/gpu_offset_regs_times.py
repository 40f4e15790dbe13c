"""The four offset regularisers of the loss block on the MI355X at an ASSUMED full-size avatar: B = 1, V = 167 281
upsampled vertices, J = 55 joints, the 24 right / left pairs of the SMPL-X names; hands of 8 % of the vertices each, a face
of 10 %, half of it expressive and a tenth of that the cavity.  These are assumptions about a training iteration, not
measurements of one.  In ONE process, forward (no grad) and forward + backward (gradients to the five inputs), eager, of the
four terms' ``.mean()`` (train.py:43) as

  reference  the lines of avatar/main/model.py:217-232, 253-257 and loss.py:133-146 as they stand: the two per-vertex
             weights and the joint weight rebuilt every call with boolean-mask / list assignments, the two Python index
             lists rebuilt and copied to the device every call;
  fused      the same expressions with constant weights and device index tensors (the `fused` form of tests/loss_case.py);
  hip        exa.OffsetRegs(...)(..., reduce='mean').

Per-call times from HIP events around windows of --iters calls, --reps windows per variant, interleaved, after a warm-up;
for each variant the median, the min / max and the spread (90th minus 10th percentile) of its windows.  `accepted` says
whether the HIP forward + backward median lies below the fused torch form's by more than three times the larger of the two
spreads.  The device launches of one call of each variant come from torch.profiler's device-side records
(--no-launch-counts skips them), and the traffic figures are computed from the shapes, not measured.  Prints one JSON line;
--out writes it to a file too.

    python tools/gpu_offset_regs_times.py [--reps 200] [--iters 50] [--out offset_regs_times.json]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import exavatar_release_amd as exa                              # noqa: E402
from exavatar_release_amd import build                          # noqa: E402
from tests.loss_case import JOINT_PART, JOINTS_NAME             # noqa: E402
from _timing import emit, window_ms                             # noqa: E402
from gpu_face_loss_times import launches                        # noqa: E402

B, V, J = 1, 167281, 55
TERMS = ('gaussian_mean_reg', 'gaussian_scale_reg', 'joint_offset_reg', 'joint_offset_sym_reg')


def make_inputs(dev):
    rs = np.random.RandomState(3)
    v = np.arange(V)
    masks = {'is_rhand': v < int(0.08 * V), 'is_lhand': (v >= int(0.08 * V)) & (v < int(0.16 * V)),
             'is_face': (v >= int(0.5 * V)) & (v < int(0.6 * V))}
    masks['is_face_expr'] = masks['is_face'] & (v < int(0.55 * V))
    masks['is_cavity'] = masks['is_face_expr'] & (v < int(0.505 * V))
    masks = {k: torch.from_numpy(m).to(dev) for k, m in masks.items()}
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dev)      # noqa: E731
    ref = 0.01 * rs.randn(J, 3)
    x = {'mean_offset': f32(0.01 * rs.randn(B, V, 3)), 'mean_offset_offset': f32(0.01 * rs.randn(B, V, 3)),
         'scale': f32(rs.uniform(0.0005, 0.0015, (B, V, 1))).repeat(1, 1, 3), 'scale_offset': f32(0.1 * rs.randn(B, V, 1)),
         'joint_offset': f32(ref + 0.005 * rs.randn(J, 3))}
    return masks, {k: t.requires_grad_(True) for k, t in x.items()}, f32(ref)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--no-launch-counts', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_offset_regs_times.py needs a ROCm device')
    dev = torch.device('cuda:0')
    masks, x, joint_ref = make_inputs(dev)
    joints_name, joint_part = list(JOINTS_NAME), {k: list(r) for k, r in JOINT_PART.items()}
    order = ('is_rhand', 'is_lhand', 'is_face', 'is_face_expr', 'is_cavity')
    weights = exa.loss_weights(*[masks[k] for k in order], joint_part=joint_part, joint_num=J)
    pairs = exa.symmetric_joint_pairs(joints_name)
    right_idx, left_idx = (torch.tensor(i, dtype=torch.int64, device=dev) for i in pairs)
    regs = exa.OffsetRegs(weights['gaussian_mean_reg'], weights['gaussian_scale_reg'], joint_ref,
                          weights['joint_offset_reg'], pairs)
    leaves = [x[k] for k in ('mean_offset', 'mean_offset_offset', 'scale', 'scale_offset', 'joint_offset')]

    def reference():
        loss = {}
        weight = torch.ones((1, V, 1)).float().cuda() * 10
        weight[:, masks['is_rhand'], :] = 1000
        weight[:, masks['is_lhand'], :] = 1000
        weight[:, masks['is_face'], :] = 1
        weight[:, masks['is_face_expr'], :] = 10
        loss['gaussian_mean_reg'] = (x['mean_offset'] ** 2 + x['mean_offset_offset'] ** 2) * weight
        weight = torch.ones((1, V, 1)).float().cuda()
        weight[:, masks['is_rhand'], :] = 1000
        weight[:, masks['is_lhand'], :] = 1000
        weight[:, masks['is_face_expr'], :] = 10
        weight[:, masks['is_cavity'], :] = 0
        loss['gaussian_scale_reg'] = (x['scale'] ** 2 + x['scale_offset'] ** 2) * weight
        weight = torch.ones((J, 3)).float().cuda()
        weight[joint_part['lhand'], :] = 10
        weight[joint_part['rhand'], :] = 10
        jo = x['joint_offset']
        loss['joint_offset_reg'] = (jo - joint_ref.cuda()) ** 2 * weight
        right_joint_idx, left_joint_idx = [], []
        for j in range(J):
            if joints_name[j][:2] == 'R_':
                right_joint_idx.append(j)
                left_joint_idx.append(joints_name.index('L_' + joints_name[j][2:]))
        loss['joint_offset_sym_reg'] = torch.abs(jo[right_joint_idx, 0] + jo[left_joint_idx, 0]) \
            + torch.abs(jo[right_joint_idx, 1] - jo[left_joint_idx, 1]) + torch.abs(jo[right_joint_idx, 2] - jo[left_joint_idx, 2])
        return {k: v.mean() for k, v in loss.items()}

    def fused():
        jo = x['joint_offset']
        r, l = jo.index_select(0, right_idx), jo.index_select(0, left_idx)
        loss = {'gaussian_mean_reg': (x['mean_offset'] ** 2 + x['mean_offset_offset'] ** 2) * weights['gaussian_mean_reg'],
                'gaussian_scale_reg': (x['scale'] ** 2 + x['scale_offset'] ** 2) * weights['gaussian_scale_reg'],
                'joint_offset_reg': (jo - joint_ref) ** 2 * weights['joint_offset_reg'],
                'joint_offset_sym_reg': torch.abs(r[:, 0] + l[:, 0]) + torch.abs(r[:, 1] - l[:, 1]) + torch.abs(r[:, 2] - l[:, 2])}
        return {k: v.mean() for k, v in loss.items()}

    def hip():
        return regs(*leaves, reduce='mean')

    def fwd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def fwd_bwd(f):
        def run():
            loss = f()
            torch.autograd.grad(sum(loss[k] for k in TERMS), leaves)
        return run

    variants = {'reference': reference, 'fused': fused, 'hip': hip}
    fns = {}
    for how, wrap in (('fwd', fwd), ('fwd_bwd', fwd_bwd)):
        for name, f in variants.items():
            fns['%s_%s' % (name, how)] = wrap(f)
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            times[k].append(window_ms(fn, args.iters))
    n = B * V
    res = {'build_digest': build._digest()[:12], 'device': torch.cuda.get_device_name(0), 'B': B, 'V': V, 'J': J,
           'pairs': len(pairs[0]), 'assumed_workload': True, 'reps': args.reps, 'iters': args.iters, 'warmup': args.warmup,
           # floats the HIP path must move, from the shapes: forward reads 3 + 3 + 3 + 1 per row and the two weights;
           # backward reads them again and writes 3 + 3 + 3 + 1 per row
           'hip_fwd_traffic_MB': 4e-6 * (10 * n + 2 * V), 'hip_bwd_traffic_MB': 4e-6 * (20 * n + 2 * V)}
    spread = {}
    for k, v in times.items():
        v = np.array(v)
        spread[k] = float(np.percentile(v, 90) - np.percentile(v, 10))
        res[k + '_ms'] = float(np.median(v))
        res[k + '_min_max_ms'] = [float(v.min()), float(v.max())]
        res[k + '_spread_ms'] = spread[k]
    for how in ('fwd', 'fwd_bwd'):
        for base in ('reference', 'fused'):
            res['ratio_%s_over_hip_%s' % (base, how)] = res['%s_%s_ms' % (base, how)] / res['hip_%s_ms' % how]
    gain = res['fused_fwd_bwd_ms'] - res['hip_fwd_bwd_ms']
    res['accepted'] = bool(gain > 3 * max(spread['fused_fwd_bwd'], spread['hip_fwd_bwd']))
    if not args.no_launch_counts:
        for k, f in fns.items():
            res[k + '_launches'] = launches(f)
    with torch.no_grad():
        a, b, c = reference(), fused(), hip()
        res['max_rel_diff_hip_vs_fused'] = max(abs(float(c[k]) - float(b[k])) / abs(float(b[k])) for k in TERMS)
        res['reference_equals_fused'] = all(float(a[k]) == float(b[k]) for k in TERMS)
    emit(res, args.out)


if __name__ == '__main__':
    main()
