"""The LPIPS term on the MI355X at an assumed full-size frame: B = 1, 1024 x 1024, a person bbox of 500 x 800 at
(262, 112).  These are assumptions about a training frame, not measurements of one; the weights are random (tests/lpips_case).
In ONE process, eager, each for

  hip    exa.LPIPS (csrc/lpips.hip), and
  torch  the oracle expression on the same device (F.conv2d / F.max_pool2d and autograd, tests/lpips_oracle.py), same weights,
  mixed  torch's trunk with exa.lpips_distance as the head:

  fwd            one forward, no grad
  fwd_bwd        one forward + the gradient to the render
  iteration      the reference's pattern (model.py:199,206): two calls, two renders against one target, forward + backward
  iteration_shared   (hip) the same with target_features run once and forward(target=) twice
  trunk / head   (hip) the target trunk alone (target_features minus the normalisation is not split off: trunk =
                 target_features) and the head alone (lpips_distance on the five taps), forward + backward

Per-call times from HIP events around windows of --iters calls, --reps windows per variant, interleaved, after a warm-up;
for each variant the median, min / max and the spread (90th minus 10th percentile).  The convolution stage's achieved
TFLOP/s is computed from the shapes (2 x 9 Cin Cout per output pixel, pooled sizes floored) against the trunk's time; the
head's GB/s from the floats it must move.  Prints one JSON line; --out writes it to a file too.

    python tools/gpu_lpips_times.py [--reps 10] [--iters 2] [--out lpips_times.json]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import exavatar_release_amd as exa                              # noqa: E402
from exavatar_release_amd import _lib, build                    # noqa: E402
from exavatar_release_amd.lpips import CHANNELS, TAP_CHANNELS   # noqa: E402
from tests import lpips_case as lc                              # noqa: E402
from tests import lpips_oracle as lo                            # noqa: E402
from _timing import emit, window_ms                             # noqa: E402

B, H, W = 1, 1024, 1024
BBOX = (262, 112, 500, 800)
BLOCK_OF = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)


def trunk_flop(h, w):
    return sum(2 * 9 * ci * co * (h >> b) * (w >> b) for (ci, co), b in zip(CHANNELS, BLOCK_OF))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--iters', type=int, default=2)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--height', type=int, default=H)
    ap.add_argument('--width', type=int, default=W)
    ap.add_argument('--bbox', type=int, nargs=4, default=BBOX)
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_lpips_times.py needs a ROCm device')
    dev = torch.device('cuda:0')
    convs, lins = lc.weights()
    module = exa.LPIPS.from_arrays(convs, lins).to(dev)
    cv, ln = lo.as_tensors(convs, lins, torch.float32)
    cv, ln = [(w.to(dev), b.to(dev)) for w, b in cv], [x.to(dev) for x in ln]
    a, t = lc.image_pair(1, B, args.height, args.width)
    b2, _ = lc.image_pair(2, B, args.height, args.width)
    x1, x2 = (torch.from_numpy(v).to(dev).requires_grad_(True) for v in (a, b2))
    tgt = torch.from_numpy(t).to(dev)
    bbox = torch.tensor([list(args.bbox)] * B, dtype=torch.float32)
    crop_h, crop_w = lo.crop(tgt, bbox).shape[2:]

    def torch_lpips(x):
        return lo.lpips(x, tgt, cv, ln, bbox)[0]

    def torch_taps(x):
        return lo.trunk(lo.input_map(lo.crop(x, bbox)), cv)

    def mixed(x):
        with torch.no_grad():
            ft = torch_taps(tgt)
        return exa.lpips_distance(torch_taps(x), ft, ln)

    with torch.no_grad():
        taps_t = [f.contiguous() for f in torch_taps(tgt)]
    taps_o = [f.detach().clone().requires_grad_(True) for f in torch_taps(x1)]

    def no_grad(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def hip_shared():
        feats = module.target_features(tgt, bbox)
        for x in (x1, x2):
            torch.autograd.grad(module(x, None, bbox, target=feats).sum(), x)

    fns = {
        'hip_fwd': no_grad(lambda: module(x1, tgt, bbox)),
        'torch_fwd': no_grad(lambda: torch_lpips(x1)),
        'hip_fwd_bwd': lambda: torch.autograd.grad(module(x1, tgt, bbox).sum(), x1),
        'torch_fwd_bwd': lambda: torch.autograd.grad(torch_lpips(x1).sum(), x1),
        'mixed_fwd_bwd': lambda: torch.autograd.grad(mixed(x1).sum(), x1),
        'hip_iteration': lambda: [torch.autograd.grad(module(x, tgt, bbox).sum(), x) for x in (x1, x2)],
        'torch_iteration': lambda: [torch.autograd.grad(torch_lpips(x).sum(), x) for x in (x1, x2)],
        'hip_iteration_shared': hip_shared,
        'hip_trunk': no_grad(lambda: module.target_features(tgt, bbox)),
        'torch_trunk': no_grad(lambda: torch_taps(tgt)),
        'hip_head_fwd_bwd': lambda: torch.autograd.grad(exa.lpips_distance(taps_o, taps_t, ln).sum(), taps_o),
        'torch_head_fwd_bwd': lambda: torch.autograd.grad(lo.head(taps_o, taps_t, ln)[0].sum(), taps_o),
    }
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            times[k].append(window_ms(fn, args.iters))
    flop = B * trunk_flop(crop_h, crop_w)
    head_floats = B * sum(c * (crop_h >> t) * (crop_w >> t) for t, c in enumerate(TAP_CHANNELS))
    res = {'build_digest': build._digest()[:12], 'device': torch.cuda.get_device_name(0), 'B': B, 'H': args.height,
           'W': args.width, 'bbox': list(args.bbox), 'crop_hw': [int(crop_h), int(crop_w)], 'assumed_workload': True,
           'reps': args.reps, 'iters': args.iters, 'warmup': args.warmup, 'trunk_GFLOP_per_image': flop * 1e-9,
           'workspace_MB': _lib.lpips_workspace_size(B, int(crop_h), int(crop_w)) * 1e-6,
           # the head reads f_out twice and the target once per pass and writes dL/df once: 3 + 4 floats per tap element
           'head_fwd_bwd_traffic_MB': 4e-6 * 7 * head_floats}
    for k, v in times.items():
        v = np.array(v)
        res[k + '_ms'] = float(np.median(v))
        res[k + '_min_max_ms'] = [float(v.min()), float(v.max())]
        res[k + '_spread_ms'] = float(np.percentile(v, 90) - np.percentile(v, 10))
    res['hip_trunk_TFLOPs'] = flop / res['hip_trunk_ms'] * 1e-9
    res['torch_trunk_TFLOPs'] = flop / res['torch_trunk_ms'] * 1e-9
    res['f32_mfma_ceiling_TFLOPs'] = 155.0
    res['hip_head_GBps'] = res['head_fwd_bwd_traffic_MB'] / res['hip_head_fwd_bwd_ms']
    for how in ('fwd', 'fwd_bwd', 'iteration', 'trunk', 'head_fwd_bwd'):
        res['ratio_' + how] = res['torch_%s_ms' % how] / res['hip_%s_ms' % how]
    res['ratio_iteration_shared'] = res['torch_iteration_ms'] / res['hip_iteration_shared_ms']
    with torch.no_grad():
        res['value_hip_torch'] = [float(module(x1, tgt, bbox)), float(torch_lpips(x1))]
    emit(res, args.out)


if __name__ == '__main__':
    main()
