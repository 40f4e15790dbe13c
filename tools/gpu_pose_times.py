"""The pose-parameter stage on the MI355X: the 6D rotation parameters of one frame (55 rows in seven tensors) and of
eight frames -> axis-angle, forward and forward + backward (gradients for every 6D tensor), of

  torch   the reference's expression, matrix_to_axis_angle(rotation_6d_to_matrix(p)) by the stand-ins, per tensor as
          SMPLXParamDict.forward runs it, eagerly only: it indexes with boolean masks nine times per tensor, each a
          read-back of the device (`nonzero`), which a stream capture refuses -- there is no captured column for it;
  hip     exavatar_release_amd.SMPLXParamDict.forward(packed=True) (one launch each way), eagerly and replayed from a
          captured graph.

Per-call medians over interleaved windows (tools/_timing.medians), the min / max of the windows next to them, the
device launches of one forward and one forward + backward of each variant (torch.profiler's device-side kernel and memcpy
records; --no-launch-counts skips them) and the max abs difference of the two forwards.  Prints one JSON line; --out
writes it to a file too.

    python tools/gpu_pose_times.py [--reps 15] [--iters 20] [--out pose_times.json]
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
from tests import pose_oracle                                   # noqa: E402
from _timing import emit, medians                               # noqa: E402

POSES = ('root_pose', 'body_pose', 'jaw_pose', 'leye_pose', 'reye_pose', 'lhand_pose', 'rhand_pose')
SHAPES = {'root_pose': (3,), 'body_pose': (21, 3), 'jaw_pose': (3,), 'leye_pose': (3,), 'reye_pose': (3,),
          'lhand_pose': (15, 3), 'rhand_pose': (15, 3), 'expr': (50,), 'trans': (3,)}


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
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--no-launch-counts', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_pose_times.py needs a ROCm device')
    dev = torch.device('cuda:0')
    rs = np.random.RandomState(3)
    m = exa.SMPLXParamDict()
    m.init({f: {n: torch.from_numpy((0.3 * rs.randn(*s)).astype(np.float32)) for n, s in SHAPES.items()}
            for f in range(8)}, device=dev)

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

    fns, eager = {}, {}
    res = {'build_digest': build._digest()[:12], 'device': torch.cuda.get_device_name(0), 'reps': args.reps,
           'iters': args.iters}
    for F in (1, 8):
        frames = list(range(F))
        leaves = [m.smplx_params[str(f)][n] for f in frames for n in POSES]
        G = [torch.randn(p.shape[:-1] + (3,), device=dev) for p in leaves]
        Gp = [torch.cat([g.view(-1, 3) for g in G[7 * f:7 * f + 7]]) for f in frames]

        def hip(frames=frames):
            return [frame['pose'] for frame in m(frames, packed=True)]

        def ref(leaves=leaves):
            return [pose_oracle.standin_expression(p) for p in leaves]

        def fwd(f):
            def run():
                with torch.no_grad():
                    f()
            return run

        hip_fb = lambda hip=hip, leaves=leaves, Gp=Gp: torch.autograd.grad(hip(), leaves, Gp)      # noqa: E731
        ref_fb = lambda ref=ref, leaves=leaves, G=G: torch.autograd.grad(ref(), leaves, G)         # noqa: E731
        tag = 'frames%d' % F
        for name, f, fb in (('hip', hip, hip_fb), ('torch', ref, ref_fb)):
            eager['%s_%s_fwd' % (name, tag)], eager['%s_%s_fwd_bwd' % (name, tag)] = fwd(f), fb
            fns['%s_%s_fwd_eager' % (name, tag)], fns['%s_%s_fwd_bwd_eager' % (name, tag)] = fwd(f), fb
        fns['hip_%s_fwd_graph' % tag], fns['hip_%s_fwd_bwd_graph' % tag] = graphed(fwd(hip)), graphed(hip_fb)
        with torch.no_grad():
            a, b = torch.cat(hip()), torch.cat([x.view(-1, 3) for x in ref()])
            res['fwd_max_abs_diff_' + tag] = float((a - b).abs().max())
    med, spread = medians(fns, args.reps, args.iters)
    for k in fns:
        res[k + '_ms'] = med[k]
        res[k + '_min_max_ms'] = list(spread[k])
    if not args.no_launch_counts:
        for k, f in eager.items():
            res[k + '_launches'] = launches(f)
    emit(res, args.out)


if __name__ == '__main__':
    main()
