"""The fused MLP on the MI355X: HIP-event medians after warm-up, at the reference shape (167 000 rows; the four nets of
HumanGaussian: geo_net + two heads, geo_offset_net with the 126-column pose folded, rgb_net, rgb_offset_net with the
pose folded and the normal per row), each net alone and all four in turn:

  hip_fwd_ms        FusedMLP forward (one launch per net).
  hip_bwd_ms        its autograd backward alone (retained graph; three launches per net).
  hip_fwd_bwd_ms    forward + autograd backward through FusedMLP.
  ref_*             the reference expression: the fp32 nn.Sequential (pose repeated per row, as the reference builds
                    it) and its head Linears, with autograd.
  hip_fwd_bwd_tflops  forward + backward FLOP (2 per multiply-add of every Linear; the backward counted as twice the
                    forward) over the HIP time, to hold against the 155 TF f32 MFMA rate.

Prints one JSON line; --out writes it to a file too.

    python tools/gpu_mlp_times.py [--reps 20] [--out mlp_times.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import exavatar_release_amd as exa                          # noqa: E402
from exavatar_release_amd import build                      # noqa: E402
from _timing import emit, median_ms                         # noqa: E402

TRI, POSE, NORMAL = 96, 126, 3


def trunk(widths, trailing=0):
    mods = []
    for a, b in zip(widths[:-1], widths[1:]):
        mods += [nn.Linear(a, b), nn.GroupNorm(4, b), nn.ReLU(inplace=True)]
    if trailing:
        mods.append(nn.Linear(widths[-1], trailing))
    return nn.Sequential(*mods)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rows', type=int, default=167000)
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_mlp_times.py needs a ROCm device')
    dev = torch.device('cuda:0')
    N = args.rows
    torch.manual_seed(0)
    nets = {
        'geo': (trunk([TRI, 128, 128, 128]), [nn.Linear(128, 3), nn.Linear(128, 1)], ('tri',)),
        'geo_offset': (trunk([TRI + POSE, 128, 128, 128]), [nn.Linear(128, 3), nn.Linear(128, 1)], ('tri', 'pose')),
        'rgb': (trunk([TRI, 128, 128, 128], 3), [], ('tri',)),
        'rgb_offset': (trunk([TRI + POSE + NORMAL, 128, 128, 128], 3), [], ('tri', 'pose', 'normal')),
    }
    for tr, heads, _ in nets.values():
        tr.to(dev)
        for h in heads:
            h.to(dev)
    gen = torch.Generator().manual_seed(1)
    tri = torch.randn(N, TRI, generator=gen).to(dev).requires_grad_(True)
    pose = torch.randn(POSE, generator=gen).to(dev)
    normal = torch.nn.functional.normalize(torch.randn(N, NORMAL, generator=gen), dim=1).to(dev)
    blocks = {'tri': tri, 'pose': pose, 'normal': normal}
    ref_blocks = {'tri': tri, 'pose': pose[None].repeat(N, 1), 'normal': normal}

    def flop(tr, heads):
        mads = sum(m.in_features * m.out_features for m in list(tr) + heads if isinstance(m, nn.Linear))
        return 3 * 2 * mads * N

    def hip_call(name):
        tr, heads, bl = nets[name]
        fm = exa.FusedMLP(tr, heads=heads or None)
        return lambda: fm(*[blocks[b] for b in bl])

    def ref_call(name):
        tr, heads, bl = nets[name]

        def f():
            h = tr(torch.cat([ref_blocks[b] for b in bl], 1))
            return tuple(hd(h) for hd in heads) if heads else h
        return f

    def as_list(o):
        return list(o) if isinstance(o, tuple) else [o]

    def params(name):
        tr, heads, _ = nets[name]
        return list(tr.parameters()) + [p for h in heads for p in h.parameters()]

    res = {'build_digest': build._digest()[:12], 'device': torch.cuda.get_device_name(0), 'rows': N, 'nets': {}}
    for label, names in [(n, [n]) for n in nets] + [('all4', list(nets))]:
        hip = [hip_call(n) for n in names]
        ref = [ref_call(n) for n in names]
        wrt = [tri] + [p for n in names for p in params(n)]
        r = {}
        with torch.no_grad():
            r['hip_fwd_ms'] = median_ms(lambda: [f() for f in hip], args.reps, 3)
            r['ref_fwd_ms'] = median_ms(lambda: [f() for f in ref], args.reps, 3)

        def fwd_bwd(calls):
            outs = [o for f in calls for o in as_list(f())]
            return torch.autograd.grad(outs, wrt, [torch.ones_like(o) for o in outs])
        r['hip_fwd_bwd_ms'] = median_ms(lambda: fwd_bwd(hip), args.reps, 3)
        r['ref_fwd_bwd_ms'] = median_ms(lambda: fwd_bwd(ref), args.reps, 3)
        for kind, calls in (('hip', hip), ('ref', ref)):
            outs = [o for f in calls for o in as_list(f())]
            gos = [torch.ones_like(o) for o in outs]
            r[kind + '_bwd_ms'] = median_ms(lambda: torch.autograd.grad(outs, wrt, gos, retain_graph=True), args.reps, 3)
        fl = sum(flop(nets[n][0], nets[n][1]) for n in names)
        r['fwd_bwd_gflop'] = fl / 1e9
        r['hip_fwd_bwd_tflops'] = fl / (r['hip_fwd_bwd_ms'] * 1e-3) / 1e12
        r['ref_fwd_bwd_tflops'] = fl / (r['ref_fwd_bwd_ms'] * 1e-3) / 1e12
        r['fraction_of_155tf'] = r['hip_fwd_bwd_tflops'] / 155.0
        for k in ('fwd', 'bwd', 'fwd_bwd'):
            r['speedup_' + k] = r['ref_%s_ms' % k] / r['hip_%s_ms' % k]
        res['nets'][label] = r
        print(label, json.dumps(r), file=sys.stderr, flush=True)
    emit(res, args.out)


if __name__ == '__main__':
    main()
