"""The keypoint path of the fitting on the MI355X at an ASSUMED fitting batch: B = 64 frames, V = 10 475 SMPL-X vertices,
J = 55 joints, 21 extra vertices, 51 static and 17 dynamic landmarks, K = 135 selected keypoints, two hands of 20 keypoints;
a random triangle list, random landmark tables and random neck rotations.  These are assumptions about a fitting step, not
measurements of one.  In ONE process, forward + backward (the gradients to vertices, joints and trans), eager, of

  reference  the reference's operation sequence restated in torch on the same device as it stands: the Rodrigues-free neck
             chain of lbs.py:85-103 with its ``bmm`` loop and clamp / round / mask ladder, ``vertices2landmarks`` with its
             ``einsum``, ``vertex_joint_selector``, the tail of ``get_smplx_coord`` (fitting/main/model.py:97-112) and
             ``CoordLoss`` (fitting/common/nets/loss.py:9-71) with its per-item Python loop and its read-backs, times ``weight``;
  hip        exa.BodyKeypoints -> exa.CoordLoss(weight=...).

(The reference additionally runs ``batch_rodrigues`` on the neck chain; the rotations are given here, as ``PosedBody`` returns
them, which favours the reference.)  Per-call times from HIP events around windows of --iters calls, --reps windows per
variant, interleaved, after a warm-up; for each variant the median, the min / max and the spread (90th minus 10th
percentile) of its windows.  ``accepted`` says whether the HIP median lies below the reference's by more than three times the
larger of the two spreads.  The device launches of one call of each variant come from torch.profiler's device-side records
(--no-launch-counts skips them).  Prints one JSON line; --out writes it to a file too.

    python tools/gpu_keypoints_times.py [--reps 30] [--iters 5] [--out keypoints_times.json]
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
from tests import kpt_oracle as ko                              # noqa: E402
from _timing import emit, window_ms                             # noqa: E402
from gpu_face_loss_times import launches                        # noqa: E402

B, V, J, K, LD = 64, 10475, 55, 135, 17


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-launch-counts', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_keypoints_times.py needs a ROCm device')
    dev = torch.device('cuda:0')
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    rs = np.random.RandomState(5)
    E, LS = 21, 51
    s = {'V': V, 'J': J, 'faces': ko.faces_of(rs, V, 600), 'extra': rs.randint(0, V, E), 'lmk_f': rs.randint(0, 600, LS),
         'lmk_w': ko.f32(rs.dirichlet(np.ones(3), LS)), 'dyn_f': rs.randint(0, 600, (ko.BINS, LD)),
         'dyn_w': ko.f32(rs.dirichlet(np.ones(3), (ko.BINS, LD))), 'chain': [12, 9, 6, 3, 0], 'append': np.zeros(0, np.int64),
         'kpt_idx': rs.permutation(J + E + LS + LD)[:K].astype(np.int64), 'root_idx': 0}
    s['kpt_idx'][0] = s['root_idx']           # the reference's root is a keypoint: kpt_cam[:, root_idx]
    cc = ko.coord_case(6, B, K)
    rot = put(ko.rotations(rs, B, J, s['chain']))
    vertices, joints = put(ko.f32(rs.randn(B, V, 3) * 0.3)).requires_grad_(True), put(ko.f32(rs.randn(B, J, 3) * 0.3)).requires_grad_(True)
    trans = put(ko.f32(rs.randn(B, 3) * 0.1 + [0, 0, 3.0])).requires_grad_(True)
    focal, princpt = put(ko.f32(rs.uniform(900, 1100, (B, 2)))), put(ko.f32(rs.uniform(200, 300, (B, 2))))
    gt, valid, weight = put(cc['gt']), put(cc['valid']), put(cc['weight'])
    lhand, rhand, lwrist, rwrist = ko.HANDS
    leaves = (vertices, joints, trans)

    kp = exa.BodyKeypoints(**ko.module_args(s)).to(dev)
    coord = exa.CoordLoss(*ko.HANDS)
    faces, extra, kpt_idx = put(s['faces']), put(s['extra']), put(s['kpt_idx'])
    lmk_f, lmk_w, dyn_f, dyn_w = put(s['lmk_f']), put(s['lmk_w']), put(s['dyn_f']), put(s['dyn_w'])
    chain = torch.tensor(s['chain'], dtype=torch.long, device=dev)

    def get_bbox(kpt_proj, kpt_valid, extend_ratio=1.2):
        x, y = kpt_proj[kpt_valid[:, 0] > 0, 0], kpt_proj[kpt_valid[:, 0] > 0, 1]
        xmin, ymin, xmax, ymax = torch.min(x), torch.min(y), torch.max(x), torch.max(y)
        x_center, width = (xmin + xmax) / 2., xmax - xmin
        xmin, xmax = x_center - 0.5 * width * extend_ratio, x_center + 0.5 * width * extend_ratio
        y_center, height = (ymin + ymax) / 2., ymax - ymin
        ymin, ymax = y_center - 0.5 * height * extend_ratio, y_center + 0.5 * height * extend_ratio
        return torch.FloatTensor([xmin, ymin, xmax - xmin, ymax - ymin]).cuda()

    def get_iou(box1, box2):
        box1, box2 = box1.clone(), box2.clone()
        box1[2:] += box1[:2]
        box2[2:] += box2[:2]
        xmin, ymin = torch.maximum(box1[0], box2[0]), torch.maximum(box1[1], box2[1])
        xmax, ymax = torch.minimum(box1[2], box2[2]), torch.minimum(box1[3], box2[3])
        inter = torch.maximum(torch.zeros_like(xmax - xmin), xmax - xmin) * torch.maximum(torch.zeros_like(ymax - ymin), ymax - ymin)
        union = (box1[2] - box1[0]) * (box1[3] - box1[1]) + (box2[2] - box2[0]) * (box2[3] - box2[1]) - inter
        return inter / (union + 1e-5)

    def coord_torch(kpt_proj, kpt_proj_gt, kpt_valid, kpt_cam):
        w = torch.ones_like(kpt_proj)
        with torch.no_grad():
            for i in range(w.shape[0]):
                if (kpt_valid[i, lhand, :].sum() == 0) or (kpt_valid[i, rhand, :].sum()) == 0:
                    continue
                iou = get_iou(get_bbox(kpt_proj[i, lhand, :], kpt_valid[i, lhand, :]), get_bbox(kpt_proj[i, rhand, :], kpt_valid[i, rhand, :]))
                if float(iou) > 0.5:
                    if kpt_cam[i, lhand, 2].mean() > kpt_cam[i, rhand, 2].mean():
                        w[i, lhand, :] = 0
                        w[i, lwrist, :] = 0
                    else:
                        w[i, rhand, :] = 0
                        w[i, rwrist, :] = 0
        return torch.abs(kpt_proj - kpt_proj_gt) * kpt_valid * w

    def reference():
        rot_mats = torch.index_select(rot, 1, chain)
        rel = torch.eye(3, device=dev, dtype=torch.float32).unsqueeze_(dim=0).repeat(B, 1, 1)
        for idx in range(len(chain)):
            rel = torch.bmm(rot_mats[:, idx], rel)
        sy = torch.sqrt(rel[:, 0, 0] * rel[:, 0, 0] + rel[:, 1, 0] * rel[:, 1, 0])
        y = torch.round(torch.clamp(-torch.atan2(-rel[:, 2, 0], sy) * 180.0 / np.pi, max=39)).to(dtype=torch.long)
        neg_mask, mask = y.lt(0).to(dtype=torch.long), y.lt(-39).to(dtype=torch.long)
        y = neg_mask * (mask * 78 + (1 - mask) * (39 - y)) + (1 - neg_mask) * y
        f_idx = torch.cat([lmk_f.unsqueeze(dim=0).expand(B, -1).contiguous(), torch.index_select(dyn_f, 0, y)], 1)
        bary = torch.cat([lmk_w.unsqueeze(dim=0).repeat(B, 1, 1), torch.index_select(dyn_w, 0, y)], 1)
        lmk_faces = torch.index_select(faces, 0, f_idx.view(-1)).view(B, -1, 3)
        lmk_faces = lmk_faces + torch.arange(B, dtype=torch.long, device=dev).view(-1, 1, 1) * V
        landmarks = torch.einsum('blfi,blf->bli', [vertices.view(-1, 3)[lmk_faces].view(B, -1, 3, 3), bary])
        full = torch.cat([torch.cat([joints, torch.index_select(vertices, 1, extra)], dim=1), landmarks], dim=1)
        kpt_cam = full[:, kpt_idx, :]
        root_cam = kpt_cam[:, 0, :]
        mesh_cam = vertices - root_cam[:, None, :] + trans[:, None, :]
        kpt_cam = kpt_cam - root_cam[:, None, :] + trans[:, None, :]
        x = kpt_cam[:, :, 0] / kpt_cam[:, :, 2] * focal[:, None, 0] + princpt[:, None, 0]
        y2 = kpt_cam[:, :, 1] / kpt_cam[:, :, 2] * focal[:, None, 1] + princpt[:, None, 1]
        kpt_proj = torch.stack((x, y2), 2)
        return coord_torch(kpt_proj, gt, valid, kpt_cam.detach()) * weight, mesh_cam

    def hip():
        out = kp(vertices, joints, rot=rot, trans=trans, focal=focal, princpt=princpt)
        return coord(out.kpt_proj, gt, valid, out.kpt_cam, weight=weight), out.mesh_cam

    def fwd_bwd(f):
        def run():
            loss, mesh = f()
            torch.autograd.grad(loss.mean() + mesh.mean(), leaves)
        return run

    fns = {'reference': fwd_bwd(reference), 'hip': fwd_bwd(hip)}
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            times[k].append(window_ms(fn, args.iters))
    res = {'build_digest': build._digest()[:12], 'device': torch.cuda.get_device_name(0), 'B': B, 'V': V, 'J': J, 'K': K,
           'assumed_workload': True, 'reps': args.reps, 'iters': args.iters, 'warmup': args.warmup,
           'what': 'BodyKeypoints -> CoordLoss, forward + backward of the means, eager, ms per call'}
    spread = {}
    for k, v in times.items():
        v = np.array(v)
        spread[k] = float(np.percentile(v, 90) - np.percentile(v, 10))
        res[k + '_ms'] = float(np.median(v))
        res[k + '_min_max_ms'] = [float(v.min()), float(v.max())]
        res[k + '_spread_ms'] = spread[k]
    res['ratio_reference_over_hip'] = res['reference_ms'] / res['hip_ms']
    res['accepted'] = bool(res['reference_ms'] - res['hip_ms'] > 3 * max(spread.values()))
    if not args.no_launch_counts:
        for k, f in fns.items():
            res[k + '_launches'] = launches(f)
    with torch.no_grad():
        (a, am), (b, bm) = reference(), hip()
        res['max_abs_diff_loss'] = float((a - b).abs().max())
        res['max_abs_diff_mesh_cam'] = float((am - bm).abs().max())
    emit(res, args.out)


if __name__ == '__main__':
    main()
