"""The scene-Gaussian stage on the MI355X at the C3 shape (P = 100 000 scene Gaussians, Mr = 15), SH degrees 0 and 3:
parameters -> the rasterizer's asset dict, forward and forward + backward (gradients for all six parameters), eager and
replayed from a captured graph, of

  torch   the reference's expression restated with torch (tests/scene_oracle.reference_expression: the stand-ins'
          rotation_6d_to_matrix, matrix_to_quaternion's candidate table with the candidate selected by gather on the
          argmax -- the reference's boolean-mask gather synchronises and cannot be captured --, torch.inverse, eval_sh's
          polynomial with a host int degree); torch.inverse checks its result on the host and cannot be captured either,
          so the captured runs take the camera centre computed beforehand (the inverse's few launches are missing there);
  hip     exavatar_release_amd.scene_assets (one launch each way).

Per-call medians over interleaved windows (tools/_timing.medians), the min / max of the windows next to them, the
device launches of one forward and one forward + backward of each variant (torch.profiler's device-side kernel and memcpy
records; --no-launch-counts skips them) and the max abs difference of the two forwards.  Prints one JSON line; --out
writes it to a file too.

    python tools/gpu_scene_times.py [--P 100000] [--reps 15] [--iters 20] [--out scene_times.json]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import exavatar_release_amd as exa                              # noqa: E402
from exavatar_release_amd import build                          # noqa: E402
from tests import scene_oracle                                  # noqa: E402
from _timing import emit, medians                               # noqa: E402

OUT = ('opacity', 'scale', 'rotation', 'rgb')


def launches(fn):
    """Device-side records (kernels, memcpys, memsets) of one call of ``fn``."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if getattr(e, 'device_type', None) == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--P', type=int, default=100000)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--no-launch-counts', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_scene_times.py needs a ROCm device')
    dev = torch.device('cuda:0')
    case = scene_oracle.make_case(args.P, 15, 3, special=False)
    params = [torch.from_numpy(case[k]).to(dev).requires_grad_(True) for k in scene_oracle.PARAMS]
    R, t = torch.from_numpy(case['R']).to(dev), torch.from_numpy(case['t']).to(dev)
    G = [torch.from_numpy(case[k]).to(dev) for k in scene_oracle.COTANGENTS]

    def fwd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def fwd_bwd(f):
        return lambda: torch.autograd.grad(f(), params, G, allow_unused=True)      # degree 0 never reads `mean`

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

    cam_pos = torch.matmul(torch.inverse(R), -t.view(3, 1)).view(1, 3)
    fns, eager = {}, {}
    for deg in (0, 3):
        def ref(deg=deg, cam_pos=None):
            a = scene_oracle.reference_expression(*params, deg, R, t, cam_pos)
            return [a[k] for k in OUT]

        def ref_captured(ref=ref):
            return ref(cam_pos=cam_pos)

        def hip(deg=deg):
            a = exa.scene_assets(*params, deg, {'R': R, 't': t})
            return [a[k] for k in OUT]

        for name, f, captured in (('torch', ref, ref_captured), ('hip', hip, hip)):
            tag = '%s_deg%d' % (name, deg)
            eager[tag + '_fwd'], eager[tag + '_fwd_bwd'] = fwd(f), fwd_bwd(f)
            for how, wrap in (('fwd', fwd), ('fwd_bwd', fwd_bwd)):
                fns['%s_%s_eager' % (tag, how)] = wrap(f)
                fns['%s_%s_graph' % (tag, how)] = graphed(wrap(captured))
    med, spread = medians(fns, args.reps, args.iters)
    res = {'build_digest': build._digest()[:12], 'device': torch.cuda.get_device_name(0), 'P': args.P, 'Mr': 15,
           'reps': args.reps, 'iters': args.iters}
    for k in fns:
        res[k + '_ms'] = med[k]
        res[k + '_min_max_ms'] = list(spread[k])
    if not args.no_launch_counts:
        for k, f in eager.items():
            res[k + '_launches'] = launches(f)
    with torch.no_grad():
        for deg in (0, 3):
            a = scene_oracle.reference_expression(*params, deg, R, t)
            b = exa.scene_assets(*params, deg, {'R': R, 't': t})
            res['fwd_max_abs_diff_deg%d' % deg] = max(float((a[k] - b[k]).abs().max()) for k in ('rotation', 'rgb'))
    emit(res, args.out)


if __name__ == '__main__':
    main()
