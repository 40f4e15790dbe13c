"""The posed SMPL-X stage on the MI355X at the reference's sizes: V = 10 475 vertices, J = 55 with the SMPL-X tree,
Lb = 100 shape and Le = 50 expression coefficients, 486 pose-corrective rows -- the per-frame pose, the coefficients,
the translation and joint_offset -> the camera-space vertices, the posed joints and the world-space mesh of
get_smplx_outputs, forward and forward + backward (gradients for all five inputs), of

  ref     the reference's expression restated with torch on the same device (tests/posed_oracle.reference_expression):
          Rodrigues, the shape einsum, the joint einsum, the 486 x 3 V corrective matmul, one 4x4 matmul per joint, the
          dense skinning matmul, torch.inverse(R), with autograd replaying it all;
  hip     exavatar_release_amd.PosedBody (one autograd node: 7 launches forward, at most 10 backward, and the
          wrapper's torch.inverse(R)).

The eager timings include the camera step on both sides.  torch.inverse synchronises on ROCm and cannot be captured, so
the graph timings are of the same calls without the camera (vertices and joints only) on both sides.  Per-call medians
over interleaved windows (tools/_timing.medians), the min / max of the windows next to them, the kernel launches of one
forward and one forward + backward on each side as the profiler counts them, and the max abs differences of the outputs
and the gradients.  Prints one JSON line; --out writes it to a file too.

    python tools/gpu_posed_times.py [--reps 15] [--iters 20] [--out posed_times.json]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import exavatar_release_amd as exa                              # noqa: E402
from exavatar_release_amd import build, lbs                     # noqa: E402
import posed_oracle as po                                       # noqa: E402
from _timing import emit, medians                               # noqa: E402


def launches(fn):
    """Device kernels of one call of ``fn`` as torch's profiler sees them (None where it records no device activity)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(e.device_type).endswith('CUDA') and 'memcpy' not in e.name.lower()
            and 'memset' not in e.name.lower())
    return n or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--verts', type=int, default=10475)
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_posed_times.py needs a ROCm device')
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(5)
    V, J, Lb, Le, parents = args.verts, 55, 100, 50, list(lbs.SMPLX_PARENTS)
    verts = rng.standard_normal((V, 3))
    verts = verts / np.linalg.norm(verts, axis=1, keepdims=True) * np.asarray([0.3, 0.9, 0.2])
    case = po.random_case(verts, np.zeros((0, 3), np.int64), Lb + Le, parents, 6)
    case['pose_mean'][:25] = 0
    inp = po.random_inputs(case, Lb, 7, zero_rows=(23, 24))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    body = exa.PosedBody(t(case['v_template']), t(case['shape_dirs']), t(case['posedirs']), t(case['J_regressor']),
                         t(case['weights']), parents, pose_mean=t(case['pose_mean']), face_offset=t(case['face_offset']))
    c = {k: t(case[k]) for k in ('v_template', 'face_offset', 'shape_dirs', 'posedirs', 'J_regressor', 'weights', 'pose_mean')}
    c['parents'] = parents
    x = [t(inp[k]).requires_grad_(True) for k in po.INPUTS]
    R, tt = t(inp['R']), t(inp['t'])
    G = [t(rng.standard_normal(s).astype(np.float32)) for s in ((V, 3), (J, 3), (V, 3))]

    ref_cam = lambda: po.reference_expression(c, *x, R, tt)                  # noqa: E731
    hip_cam = lambda: tuple(body(*x, R, tt))[:3]                             # noqa: E731
    ref = lambda: po.reference_expression(c, *x)[:2]                         # noqa: E731
    hip = lambda: tuple(body(*x))[:2]                                        # noqa: E731

    def fwd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def fwd_bwd(f):
        return lambda: torch.autograd.grad(list(f()), x, G[:len(f())])

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

    fns = {}
    for name, f_cam, f in (('ref', ref_cam, ref), ('hip', hip_cam, hip)):
        fns[name + '_fwd_eager'] = fwd(f_cam)
        fns[name + '_fwd_bwd_eager'] = fwd_bwd(f_cam)
        fns[name + '_nocam_fwd_eager'] = fwd(f)
        fns[name + '_nocam_fwd_bwd_eager'] = fwd_bwd(f)
        fns[name + '_nocam_fwd_graph'] = graphed(fwd(f))
        fns[name + '_nocam_fwd_bwd_graph'] = graphed(fwd_bwd(f))
    med, spread = medians(fns, args.reps, args.iters)
    res = {'build_digest': build._digest()[:12], 'device': torch.cuda.get_device_name(0), 'V': V, 'J': J, 'Lb': Lb, 'Le': Le,
           'regressor_nonzeros': body.nnz, 'hip_launches_fwd': 7, 'hip_launches_bwd_max': 10, 'reps': args.reps,
           'iters': args.iters}
    for k in fns:
        res[k + '_ms'] = med[k]
        res[k + '_min_max_ms'] = list(spread[k])
    for name, f in (('ref', ref_cam), ('hip', hip_cam)):
        res[name + '_kernels_fwd'] = launches(fwd(f))
        res[name + '_kernels_fwd_bwd'] = launches(fwd_bwd(f))
    a, b = ref_cam(), hip_cam()
    ga, gb = torch.autograd.grad(list(a), x, G), torch.autograd.grad(list(b), x, G)
    names = po.OUTPUTS + tuple('grad_' + k for k in po.INPUTS)
    for name, p, q in zip(names, list(a) + list(ga), list(b) + list(gb)):
        res['max_abs_diff_' + name] = float((p.detach() - q.detach()).abs().max())
    emit(res, args.out)


if __name__ == '__main__':
    main()
