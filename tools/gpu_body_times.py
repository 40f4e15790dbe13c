"""The SMPL-X template stage on the MI355X at the reference's sizes: a closed coarse mesh of 10 242 vertices and 20 480
faces (a level-5 icosphere; SMPL-X has 10 475 and 20 908) subdivided twice to 163 842 fine vertices, J = 55 with the
SMPL-X tree, L = 100 shape coefficients, 486 pose-corrective rows -- shape_param and joint_offset -> the four results of
get_neutral_pose_human(True, True) and joint_zero_pose, forward and forward + backward (gradients for both), eager and
replayed from a captured graph, of

  ref     the reference's expression restated with torch on the same device (tests/body_oracle.reference_expression):
          two full lbs (shape einsum, joint einsum, Rodrigues, the 486 x 3 V corrective matmul, one 4x4 matmul per joint,
          the dense skinning matmul), a third chain and two SubdivideMeshes stand-ins, with autograd replaying it all;
  hip     exavatar_release_amd.BodyTemplate (one autograd node: 7 launches forward, at most 10 backward).

Per-call medians over interleaved windows (tools/_timing.medians), the min / max of the windows next to them, and the
max abs differences of the outputs and the gradients.  Prints one JSON line; --out writes it to a file too.

    python tools/gpu_body_times.py [--reps 15] [--iters 20] [--out body_times.json]
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import exavatar_release_amd as exa                              # noqa: E402
from exavatar_release_amd import build, lbs                     # noqa: E402
import body_oracle as bo                                        # noqa: E402
import human_case                                               # noqa: E402
from _timing import emit, medians                               # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--level', type=int, default=5, help='icosphere level of the coarse mesh')
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_body_times.py needs a ROCm device')
    dev = torch.device('cuda:0')
    verts, faces = human_case._icosphere(args.level)
    verts = verts * np.asarray(human_case.RADII)
    J, L, parents = 55, 100, list(lbs.SMPLX_PARENTS)
    case, coef, jo = bo.random_case(verts, faces, L, parents, 2, 3)
    rng = np.random.RandomState(4)
    V = verts.shape[0]
    pose = np.zeros((J, 3), dtype=np.float32)
    pose[1:22] = (0.3 * rng.standard_normal((21, 3))).astype(np.float32)
    posedirs = (0.01 * rng.standard_normal((9 * (J - 1), 3 * V))).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    layer = types.SimpleNamespace(v_template=t(case['v_template']), shapedirs=t(case['shape_dirs']), expr_dirs=None,
                                  posedirs=t(posedirs), J_regressor=t(case['J_regressor']), lbs_weights=t(case['weights']),
                                  parents=parents)
    tpl = exa.BodyTemplate.from_layer(layer, faces, t(pose), face_offset=t(case['face_offset']))
    c = {k: t(case[k]) for k in ('v_template', 'face_offset', 'shape_dirs', 'J_regressor', 'weights')}
    c.update(pose=t(pose), posedirs=t(posedirs), parents=parents, root=0, rot_inverse=tpl.rot_inverse)
    subs = [s.to(dev) for s in bo.stand_in_subdividers(case['v_template'], faces, 2)]
    coef, jo = t(coef).requires_grad_(True), t(jo).requires_grad_(True)
    Vn = tpl.upsampler.num_verts
    G = [t(rng.standard_normal(s).astype(np.float32)) for s in ((Vn, 3), (V, 3), (J, 3), (J, 4, 4), (J, 3))]

    ref = lambda: bo.reference_expression(c, coef, jo, subs)      # noqa: E731
    hip = lambda: tuple(tpl(coef, jo))                            # noqa: E731

    def fwd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def fwd_bwd(f):
        return lambda: torch.autograd.grad(list(f()), [coef, jo], G)

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
    for name, f in (('ref', ref), ('hip', hip)):
        fns[name + '_fwd_eager'] = fwd(f)
        fns[name + '_fwd_bwd_eager'] = fwd_bwd(f)
        fns[name + '_fwd_graph'] = graphed(fwd(f))
        fns[name + '_fwd_bwd_graph'] = graphed(fwd_bwd(f))
    med, spread = medians(fns, args.reps, args.iters)
    res = {'build_digest': build._digest()[:12], 'device': torch.cuda.get_device_name(0), 'V': V, 'faces': int(faces.shape[0]),
           'V_upsampled': Vn, 'J': J, 'L': L, 'regressor_nonzeros': tpl.nnz, 'hip_launches_fwd': 7, 'hip_launches_bwd_max': 10,
           'reps': args.reps, 'iters': args.iters}
    for k in fns:
        res[k + '_ms'] = med[k]
        res[k + '_min_max_ms'] = list(spread[k])
    a, b = ref(), hip()
    ga, gb = torch.autograd.grad(list(a), [coef, jo], G), torch.autograd.grad(list(b), [coef, jo], G)
    for name, x, y in zip(bo.OUTPUTS + ('grad_coef', 'grad_joint_offset'), list(a) + list(ga), list(b) + list(gb)):
        res['max_abs_diff_' + name] = float((x.detach() - y.detach()).abs().max())
    emit(res, args.out)


if __name__ == '__main__':
    main()
