"""The mesh terms of the fitting loss on the MI355X at an ASSUMED fitting batch: B = 64 frames, V = 5 023 FLAME vertices,
F = 9 976 faces, V_full = 10 475 SMPL-X vertices, J = 55 joints; a random triangle list, a random flip correspondence and a
neck of 15 % of the vertices.  These are assumptions about a fitting step, not measurements of one.  In ONE process, forward
+ backward (the gradient to the one optimised input), eager, of each term's ``.mean()`` as

  reference  the lines of fitting/common/nets/loss.py:73-87, 125-167 and fitting/main/model.py:235-237 restated in torch as
             they stand: the face list, closest_faces and bc copied from the host on every call;
  resident   the same expressions with those tables held on the device (the per-call host copies excluded);
  hip        exa.EdgeLengthLoss / FaceOffsetSymmetricReg / PoseLoss / centered_v2v_loss;

and of the block of model.py:235-239 as a whole (the centred term, the Laplacian term with exa.LaplacianReg on the `hip` side
and the reference's expression on the others, the edge term).  Per-call times from HIP events around windows of --iters
calls, --reps windows per variant, interleaved, after a warm-up; for each variant the median, the min / max and the spread
(90th minus 10th percentile) of its windows.  `accepted_<term>` says whether the HIP median lies below the resident torch
form's by more than three times the larger of the two spreads.  The device launches of one call of each variant come from
torch.profiler's device-side records (--no-launch-counts skips them).  Prints one JSON line; --out writes it to a file too.

    python tools/gpu_fit_terms_times.py [--reps 100] [--iters 20] [--out fit_terms_times.json]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import exavatar_release_amd as exa                              # noqa: E402
from exavatar_release_amd import build, p3d_standins            # noqa: E402
from tests import fit_oracle as fo                              # noqa: E402
from _timing import emit, window_ms                             # noqa: E402
from gpu_face_loss_times import launches                        # noqa: E402

B, V, F, V_FULL, J = 64, 5023, 9976, 10475, 55
TERMS = ('edge', 'sym', 'pose', 'v2v', 'block')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--no-launch-counts', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_fit_terms_times.py needs a ROCm device')
    dev = torch.device('cuda:0')
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    ce, cs, cp, cv = fo.edge_case(1, B, V, F), fo.sym_case(2, B, V_FULL, V), fo.pose_case(3, B * J, special=False), \
        fo.v2v_case(4, B, V)
    face_np = ce['face']
    face_np[:V, 0] = np.arange(V)             # every vertex in a face (LaplacianReg needs it) ..
    while True:                               # .. and three distinct corners again: torch's sqrt backward gives NaN otherwise
        c1 = face_np[:, 1] == face_np[:, 0]
        c2 = (face_np[:, 2] == face_np[:, 0]) | (face_np[:, 2] == face_np[:, 1])
        if not (c1 | c2).any():
            break
        face_np[c1, 1] = (face_np[c1, 1] + 1) % V
        face_np[c2, 2] = (face_np[c2, 2] + 1) % V
    coord, coord_gt = put(ce['out']).requires_grad_(True), put(ce['gt'])
    is_not_neck = put(cv['weight'])
    offset = put(cs['p']).requires_grad_(True)
    fvi_np, closest_np, bc_np = cs['face_vertex_idx'], cs['closest_faces'], cs['bc']
    pose, pose_gt = put(cp['out'].reshape(B, -1)).requires_grad_(True), put(cp['gt'].reshape(B, -1))
    target = put(cv['target'])
    face_dev, fvi_dev, closest_dev, bc_dev = put(face_np), put(fvi_np), put(closest_np), put(bc_np)

    edge_hip, sym_hip, pose_hip = exa.EdgeLengthLoss(face_np), exa.FaceOffsetSymmetricReg(V_FULL, fvi_np, closest_np, bc_np).to(dev), \
        exa.PoseLoss()
    lap_hip = exa.LaplacianReg(V, face_np)
    nbr_idx, nbr_w = lap_hip.neighbor_idxs, lap_hip.neighbor_weights

    def edge_torch(face):
        def d(x, a, b):
            return torch.sqrt(torch.sum((x[:, face[:, a], :] - x[:, face[:, b], :]) ** 2, 2, keepdim=True))
        parts = [torch.abs(d(coord, a, b) - d(coord_gt, a, b)) * (is_not_neck[:, face[:, a], :] * is_not_neck[:, face[:, b], :])
                 for a, b in ((0, 1), (0, 2), (1, 2))]
        return torch.cat(parts, 1)

    def sym_torch(closest, bc):
        full = torch.zeros((B, V_FULL, 3)).float().cuda()
        full[:, fvi_np, :] = offset
        flip = torch.sum(full[:, closest.view(-1), :].view(B, V_FULL, 3, 3) * bc.view(1, V_FULL, 3, 1), 2)
        loss = torch.abs(full[:, :, 0] + flip[:, :, 0]) + torch.abs(full[:, :, 1] - flip[:, :, 1]) + torch.abs(full[:, :, 2] - flip[:, :, 2])
        return loss[:, fvi_np]

    def sym_torch_resident():
        full = torch.zeros((B, V_FULL, 3), device=dev)
        full[:, fvi_dev, :] = offset
        flip = torch.sum(full[:, closest_dev.view(-1), :].view(B, V_FULL, 3, 3) * bc_dev.view(1, V_FULL, 3, 1), 2)
        loss = torch.abs(full[:, :, 0] + flip[:, :, 0]) + torch.abs(full[:, :, 1] - flip[:, :, 1]) + torch.abs(full[:, :, 2] - flip[:, :, 2])
        return loss[:, fvi_dev]

    def pose_torch():
        a = p3d_standins.axis_angle_to_matrix(pose.view(B, -1, 3))
        return torch.abs(a - p3d_standins.axis_angle_to_matrix(pose_gt.view(B, -1, 3)))

    def v2v_torch():
        return torch.abs((coord - coord.mean(1)[:, None, :]) - (target - target.mean(1)[:, None, :]).detach()) * is_not_neck * 10

    def lap_torch():
        lap = lambda x: x + (x[:, nbr_idx] * nbr_w[None, :, :, None]).sum(2)      # noqa: E731
        return (lap(coord) - lap(target)) ** 2 * is_not_neck * 100000

    variants = {
        'edge': {'reference': (lambda: edge_torch(torch.LongTensor(face_np).cuda()), coord),
                 'resident': (lambda: edge_torch(face_dev), coord),
                 'hip': (lambda: edge_hip(coord, coord_gt, is_not_neck), coord)},
        'sym': {'reference': (lambda: sym_torch(torch.LongTensor(closest_np).cuda(), torch.FloatTensor(bc_np).cuda()), offset),
                'resident': (sym_torch_resident, offset),
                'hip': (lambda: sym_hip(offset), offset)},
        'pose': {'reference': (pose_torch, pose), 'resident': (pose_torch, pose), 'hip': (lambda: pose_hip(pose, pose_gt), pose)},
        'v2v': {'reference': (v2v_torch, coord), 'resident': (v2v_torch, coord),
                'hip': (lambda: exa.centered_v2v_loss(coord, target, is_not_neck), coord)},
        'block': {'reference': (lambda: (v2v_torch(), lap_torch(), edge_torch(torch.LongTensor(face_np).cuda())), coord),
                  'resident': (lambda: (v2v_torch(), lap_torch(), edge_torch(face_dev)), coord),
                  'hip': (lambda: (exa.centered_v2v_loss(coord, target, is_not_neck),
                                   lap_hip(coord, target) * is_not_neck * 100000, edge_hip(coord, coord_gt, is_not_neck)), coord)},
    }

    def fwd_bwd(f, leaf):
        def run():
            out = f()
            out = out if isinstance(out, tuple) else (out,)
            torch.autograd.grad(sum(o.mean() for o in out), leaf)
        return run

    fns = {'%s_%s' % (term, name): fwd_bwd(f, leaf) for term, vs in variants.items() for name, (f, leaf) in vs.items()}
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            times[k].append(window_ms(fn, args.iters))
    res = {'build_digest': build._digest()[:12], 'device': torch.cuda.get_device_name(0), 'B': B, 'V': V, 'F': F,
           'V_full': V_FULL, 'J': J, 'assumed_workload': True, 'reps': args.reps, 'iters': args.iters, 'warmup': args.warmup,
           'what': 'forward + backward of the mean, eager, ms per call'}
    spread = {}
    for k, v in times.items():
        v = np.array(v)
        spread[k] = float(np.percentile(v, 90) - np.percentile(v, 10))
        res[k + '_ms'] = float(np.median(v))
        res[k + '_min_max_ms'] = [float(v.min()), float(v.max())]
        res[k + '_spread_ms'] = spread[k]
    for term in TERMS:
        for base in ('reference', 'resident'):
            res['ratio_%s_over_hip_%s' % (base, term)] = res['%s_%s_ms' % (term, base)] / res['%s_hip_ms' % term]
        gain = res[term + '_resident_ms'] - res[term + '_hip_ms']
        res['accepted_' + term] = bool(gain > 3 * max(spread[term + '_resident'], spread[term + '_hip']))
    if not args.no_launch_counts:
        for k, f in fns.items():
            res[k + '_launches'] = launches(f)
    res['gradients_finite'] = all(bool(torch.isfinite(torch.autograd.grad(sum(o.mean() for o in (
        out if isinstance(out, tuple) else (out,))), leaf)[0]).all()) for vs in variants.values() for f, leaf in vs.values()
        for out in (f(),))
    with torch.no_grad():
        for term in ('edge', 'sym', 'pose', 'v2v'):
            a, b = variants[term]['resident'][0](), variants[term]['hip'][0]()
            res['max_abs_diff_hip_vs_torch_' + term] = float((a.reshape(b.shape) - b).abs().max())
    emit(res, args.out)


if __name__ == '__main__':
    main()
