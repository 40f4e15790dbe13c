"""The face-composited L1 term on the MI355X at an assumed full-size frame: B = 1, 1024 x 1024, a person bbox of
500 x 800 at (262, 112) inside the image and a face disc 120 px across inside it (every channel a face's colour, coverage 1
in the core and 0.5 on a 6 px rim; -1 / 0 elsewhere).  These are assumptions about a training frame, not measurements of one.
In ONE process, forward (no grad) and forward + backward (gradients to the render and to the face render), eager, of

  dropin  the two reference lines (avatar/main/model.py:200-201) in torch, exa.RGBLoss over the bbox and .mean();
  hip     exa.FaceRGBLoss()(..., reduce='mean').

Per-call times from HIP events around windows of --iters calls, --reps windows per variant, interleaved, after a warm-up;
for each variant the median, the min / max and the spread (90th minus 10th percentile) of its windows.  `accepted` says
whether the HIP forward + backward median lies below the drop-in's by more than three times the larger of the two spreads.
The device launches of one call of each variant come from torch.profiler's device-side records (--no-launch-counts skips
them), and the traffic figures are computed from the shapes, not measured.  Prints one JSON line; --out writes it to a file too.

    python tools/gpu_face_loss_times.py [--reps 200] [--iters 50] [--out face_loss_times.json]
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
from _timing import emit, window_ms                             # noqa: E402

B, H, W = 1, 1024, 1024
BBOX = (262, 112, 500, 800)
FACE = (512, 300, 60, 6)      # centre x, y, radius, rim


def launches(fn):
    """Device-side records (kernels, memcpys, memsets) of one call of ``fn``."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if getattr(e, 'device_type', None) == torch.autograd.DeviceType.CUDA)


def make_inputs(dev):
    rs = np.random.RandomState(3)
    img = rs.uniform(0.02, 0.98, (B, 3, H, W)).astype(np.float32)
    target = rs.uniform(0.02, 0.98, (B, 3, H, W)).astype(np.float32)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    d = np.sqrt((xx - FACE[0]) ** 2 + (yy - FACE[1]) ** 2)[None, None]
    rgb = np.where(d < FACE[2], rs.uniform(0.02, 0.98, (B, 3, H, W)), -1.0)
    cov = np.where(d < FACE[2] - FACE[3], 1.0, np.where(d < FACE[2], 0.5, 0.0)) * np.ones((B, 1, 1, 1))
    face = np.concatenate([rgb, cov], 1).astype(np.float32)
    t = lambda a, grad: torch.from_numpy(a).to(dev).requires_grad_(grad)      # noqa: E731
    return t(img, True), t(face, True), t(target, False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--no-launch-counts', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_face_loss_times.py needs a ROCm device')
    dev = torch.device('cuda:0')
    img, face, target = make_inputs(dev)
    bbox = torch.tensor([BBOX] * B, dtype=torch.float32)
    rgb_loss, face_loss = exa.RGBLoss(), exa.FaceRGBLoss()

    def dropin():
        is_face = ((face[:, :3] != -1) * (face[:, 3:] == 1)).float()
        return rgb_loss(img * (1 - is_face) + face[:, :3] * is_face, target, bbox=bbox).mean()

    def hip():
        return face_loss(img, face, target, bbox=bbox, reduce='mean')

    def fwd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def fwd_bwd(f):
        return lambda: torch.autograd.grad(f(), (img, face))

    fns = {'dropin_fwd': fwd(dropin), 'hip_fwd': fwd(hip), 'dropin_fwd_bwd': fwd_bwd(dropin), 'hip_fwd_bwd': fwd_bwd(hip)}
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            times[k].append(window_ms(fn, args.iters))
    crop_px, img_px = BBOX[2] * BBOX[3], H * W
    res = {'build_digest': build._digest()[:12], 'device': torch.cuda.get_device_name(0), 'B': B, 'H': H, 'W': W,
           'bbox': list(BBOX), 'face_disc_px': 2 * FACE[2], 'assumed_workload': True, 'reps': args.reps, 'iters': args.iters,
           'warmup': args.warmup,
           # floats the fused path must move, from the shapes: forward reads 3 + 4 + 3 per crop pixel; backward reads them
           # again and writes 3 + 4 per image pixel
           'hip_fwd_traffic_MB': 4e-6 * B * 10 * crop_px,
           'hip_bwd_traffic_MB': 4e-6 * B * (10 * crop_px + 7 * img_px)}
    spread = {}
    for k, v in times.items():
        v = np.array(v)
        spread[k] = float(np.percentile(v, 90) - np.percentile(v, 10))
        res[k + '_ms'] = float(np.median(v))
        res[k + '_min_max_ms'] = [float(v.min()), float(v.max())]
        res[k + '_spread_ms'] = spread[k]
    for how in ('fwd', 'fwd_bwd'):
        res['ratio_' + how] = res['dropin_%s_ms' % how] / res['hip_%s_ms' % how]
    gain = res['dropin_fwd_bwd_ms'] - res['hip_fwd_bwd_ms']
    res['accepted'] = bool(gain > 3 * max(spread['dropin_fwd_bwd'], spread['hip_fwd_bwd']))
    if not args.no_launch_counts:
        for k, f in fns.items():
            res[k + '_launches'] = launches(f)
    with torch.no_grad():
        res['mean_abs_diff'] = abs(float(dropin()) - float(hip()))
    emit(res, args.out)


if __name__ == '__main__':
    main()
