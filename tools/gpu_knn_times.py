"""knn_points on the MI355X: HIP-event medians after warm-up of the HIP search with culling on, with culling off, and of
the PyTorch stand-in (p3d_standins.knn_points), at the reference's two shapes:

  k1   K = 1, 167 000 queries (scenes.dist_b_avatar points plus offsets of 5 mm) against 10 475 refs drawn from the same
       surface: the per-frame nearest-vertex search of module.py:543.
  k4   K = 4 self-query on 300 000 scattered points: the scene-Gaussian scale of module.py:86.

Also the fraction of the P1 x P2 point pairs the culled search compared (from the kernel's per-wave counters), and
whether the three paths agree (idx equal; dists bit-equal between the two HIP modes).  Prints one JSON line; --out
writes it to a file too.

    python tools/gpu_knn_times.py [--reps 10] [--out knn_times.json]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import exavatar_release_amd as exa                          # noqa: E402
from exavatar_release_amd import _lib, build, p3d_standins, scenes   # noqa: E402
from exavatar_release_amd.rasterizer import _ptr, _stream_ptr  # noqa: E402
from _timing import emit, median_ms                         # noqa: E402


def shapes():
    g = torch.Generator().manual_seed(0)
    refs = scenes.dist_b_avatar(10475, seed=1)['mean_3d']
    q = scenes.dist_b_avatar(167000, seed=2)['mean_3d'] + 0.005 * torch.randn(167000, 3, generator=g)
    xyz = torch.cat([torch.randn(150000, 3, generator=g) * 2, torch.rand(150000, 3, generator=g) * 8 - 4])
    xyz = xyz[torch.randperm(300000, generator=g)].contiguous()
    return {'k1': (q[None], refs[None], 1), 'k4': (xyz[None], xyz[None], 4)}


def visited_fraction(p1, p2, K):
    """Pairs the culled search compared / P1 x P2, from exa_knn_forward's per-wave ref counts."""
    N, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    dev = p1.device
    nbytes = _lib.knn_workspace_size(N, P1, P2, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dists = torch.empty((N, P1, K), dtype=torch.float32, device=dev)
    idx = torch.empty((N, P1, K), dtype=torch.int64, device=dev)
    waves = (P1 + 63) // 64
    refs = torch.zeros((N, waves), dtype=torch.int32, device=dev)
    _lib.KNN.check(_lib.load().exa_knn_forward(N, P1, P2, K, _ptr(p1), _ptr(p2), 0, _ptr(ws), nbytes, _ptr(dists),
                                               _ptr(idx), _ptr(refs), _stream_ptr(dev)))
    qcount = torch.full((waves,), 64.0, dtype=torch.float64, device=dev)
    qcount[-1] = P1 - 64 * (waves - 1)
    pairs = (refs.double() * qcount).sum().item()
    return pairs / (N * P1 * P2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--standin-reps', type=int, default=3)
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_knn_times.py needs a ROCm device')
    dev = torch.device('cuda:0')
    res = {'build_digest': build._digest()[:12], 'device': torch.cuda.get_device_name(0)}
    for name, (p1, p2, K) in shapes().items():
        p1, p2 = p1.to(dev), p2.to(dev)
        row = {'P1': p1.shape[1], 'P2': p2.shape[1], 'K': K}
        outs = {}

        def hip(cull):
            exa.config.knn_cull = cull
            outs[cull] = exa.knn_points(p1, p2, K=K)

        with torch.no_grad():
            row['hip_cull_ms'] = median_ms(lambda: hip(True), args.reps, 3)
            row['hip_nocull_ms'] = median_ms(lambda: hip(False), args.reps, 3)
            row['standin_ms'] = median_ms(lambda: outs.__setitem__('s', p3d_standins.knn_points(p1, p2, K=K)),
                                          args.standin_reps, 1)
            row['visited_pair_fraction'] = visited_fraction(p1, p2, K)
        row['cull_equals_nocull'] = bool(torch.equal(outs[True].idx, outs[False].idx) and
                                         torch.equal(outs[True].dists.view(torch.int32), outs[False].dists.view(torch.int32)))
        row['idx_equals_standin'] = bool(torch.equal(outs[True].idx, outs['s'].idx))
        row['speedup_cull_vs_standin'] = row['standin_ms'] / row['hip_cull_ms']
        row['speedup_cull_vs_nocull'] = row['hip_nocull_ms'] / row['hip_cull_ms']
        res[name] = row
    emit(res, args.out)


if __name__ == '__main__':
    main()
