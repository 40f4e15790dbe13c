"""The mesh Laplacian regulariser on the MI355X, against the reference expression run by PyTorch on the same device in
the same process: a 409 x 409 triangulated grid (V = 167 281, the size of the reference's upsampled human mesh), K = 10,
``[1, V, 3]`` inputs.  Every figure is the median over --reps windows of the time per call, each window --iters calls
between two HIP events after a warm-up; the two sides' windows alternate.

  {ref,hip}_fwd_{none,target}_ms       forward alone (no_grad), without and with a target.
  {ref,hip}_fwd_bwd_{none,target}_ms   forward + autograd backward for a dense upstream gradient.
  {ref,hip}_block_ms                   the whole of model.py:237-247: six calls with their weights, constants and
                                       .mean()s, and the backward to the six inputs.  ``hip_block_ms`` is the one-line swap
                                       (the ``* weight`` stays in PyTorch); ``hip_block_weight_ms`` passes ``weight=``.
  speedup_*                            ref / hip of the same row.

ref = the reference's ``x + (x[:, idx] * w[None, :, :, None]).sum(2)`` and its squares, whose backward is PyTorch's
``index_put_(accumulate=True)``.  Also the largest difference between the two sides' losses and gradients.  Prints one
JSON line; --out writes it to a file too.

    python tools/gpu_lap_times.py [--reps 7] [--iters 200] [--out lap_times.json]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import exavatar_release_amd as exa                          # noqa: E402
from exavatar_release_amd import build                       # noqa: E402
from _timing import emit, medians                           # noqa: E402


def grid_faces(rows, cols):
    r, c = np.meshgrid(np.arange(rows - 1), np.arange(cols - 1), indexing='ij')
    a = (r * cols + c).reshape(-1)
    return np.concatenate([np.stack([a, a + 1, a + cols], 1), np.stack([a + 1, a + cols + 1, a + cols], 1)]).astype(np.int64)


class ReferenceExpression:
    """``LaplacianReg.forward`` as the reference writes it (loss.py:118-131), on a given table."""

    def __init__(self, idxs, weights):
        self.idxs, self.weights = idxs, weights

    def lap(self, x):
        return x + (x[:, self.idxs] * self.weights[None, :, :, None]).sum(2)

    def __call__(self, out, target):
        if target is None:
            return self.lap(out) ** 2
        return (self.lap(out) - self.lap(target)) ** 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--grid', type=int, default=409)
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_lap_times.py needs a ROCm device')
    dev = torch.device('cuda:0')
    V = args.grid * args.grid
    hip = exa.LaplacianReg(V, grid_faces(args.grid, args.grid))
    ref = ReferenceExpression(hip.neighbor_idxs, hip.neighbor_weights)
    gen = torch.Generator().manual_seed(5)
    rand = lambda *s: torch.randn(*s, generator=gen).to(dev)      # noqa: E731
    neutral = rand(1, V, 3)
    x = (neutral + 0.01 * rand(1, V, 3)).requires_grad_(True)
    G = rand(1, V, 3)
    res = {'build_digest': build._digest()[:12], 'device': torch.cuda.get_device_name(0), 'V': V, 'K': 10, 'C': 3,
           'reps': args.reps, 'iters': args.iters}

    fns = {}
    for side, reg in (('ref', ref), ('hip', hip)):
        for mode, target in (('none', None), ('target', neutral)):
            def fwd(reg=reg, target=target):
                with torch.no_grad():
                    return reg(x, target)

            def fwd_bwd(reg=reg, target=target):
                return torch.autograd.grad(reg(x, target), x, G)
            fns['%s_fwd_%s_ms' % (side, mode)] = fwd
            fns['%s_fwd_bwd_%s_ms' % (side, mode)] = fwd_bwd

    # model.py:237-247: lap_mean (two calls with a target), lap_scale and lap_rgb (two calls each without)
    ins = [(neutral + 0.01 * rand(1, V, 3)).requires_grad_(True) for _ in range(2)] + \
        [rand(1, V, 3).requires_grad_(True) for _ in range(4)]
    w_mean, w_scale, w_rgb = [(torch.rand(1, V, 1, generator=gen) * s).to(dev) for s in (50.0, 10.0, 100.0)]

    def block(reg, fused):
        a, b, s1, s2, c1, c2 = ins
        if fused:
            lap_mean = (reg(a, neutral, w_mean) + reg(b, neutral, w_mean)) * 100000
            lap_scale = (reg(s1, None, w_scale) + reg(s2, None, w_scale)) * 100000
            lap_rgb = reg(c1, None, w_rgb) + reg(c2, None, w_rgb)
        else:
            lap_mean = (reg(a, neutral) + reg(b, neutral)) * 100000 * w_mean
            lap_scale = (reg(s1, None) + reg(s2, None)) * 100000 * w_scale
            lap_rgb = (reg(c1, None) + reg(c2, None)) * w_rgb
        total = lap_mean.mean() + lap_scale.mean() + lap_rgb.mean()
        return torch.autograd.grad(total, ins)

    fns['ref_block_ms'] = lambda: block(ref, False)
    fns['hip_block_ms'] = lambda: block(hip, False)
    fns['hip_block_weight_ms'] = lambda: block(hip, True)

    med, spread = medians(fns, args.reps, args.iters)
    res.update(med)
    res['min_max_ms'] = {k: [round(a, 5), round(b, 5)] for k, (a, b) in spread.items()}
    for k in list(med):
        if k.startswith('hip_'):
            r = 'ref_block_ms' if k.startswith('hip_block') else 'ref_' + k[4:]
            res['speedup_' + k[4:-3]] = med[r] / med[k]

    with torch.no_grad():
        res['loss_max_abs_diff_vs_ref'] = float((hip(x, neutral) - ref(x, neutral)).abs().max())
    g_hip, g_ref = torch.autograd.grad(hip(x, neutral), x, G)[0], torch.autograd.grad(ref(x, neutral), x, G)[0]
    res['grad_max_abs_diff_vs_ref'] = float((g_hip - g_ref).abs().max())
    res['grad_max_abs'] = float(g_ref.abs().max())
    again = torch.autograd.grad(ref(x, neutral), x, G)[0]
    res['ref_grad_elements_differing_between_two_calls'] = int((again != g_ref).sum())
    res['hip_grad_elements_differing_between_two_calls'] = int((torch.autograd.grad(hip(x, neutral), x, G)[0] != g_hip).sum())
    emit(res, args.out)


if __name__ == '__main__':
    main()
