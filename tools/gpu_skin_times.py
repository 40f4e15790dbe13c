"""The skinning on the MI355X: HIP-event medians after warm-up, at the reference shape (167 000 avatar points, J = 55
rigid joint transforms, S = 2 point sets, the camera step, idx from knn_points against a 10 475-point subset with the
identity on a hand / face mask: tests/test_gpu_skinning.py's _reference_shape):

  hip_fwd_ms        skin_points forward (one launch, plus torch.inverse(R) in the wrapper).
  hip_bwd_ms        its backward alone (exa_skin_backward: two launches).
  hip_fwd_bwd_ms    forward + autograd backward through skin_points.
  ref_fwd_ms        the reference's PyTorch expression (get_transform_mat_vertex + two lbs + the camera step).
  ref_bwd_ms        its autograd backward alone (retained graph).
  ref_fwd_bwd_ms    the same forward plus its autograd backward.

Also whether the HIP forward matches the reference expression (max abs difference).  Prints one JSON line; --out
writes it to a file too.

    python tools/gpu_skin_times.py [--reps 50] [--out skin_times.json]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import exavatar_release_amd as exa                          # noqa: E402
from exavatar_release_amd import _lib, build, lbs, scenes    # noqa: E402
from exavatar_release_amd.rasterizer import _ptr, _stream_ptr, _workspace  # noqa: E402
from exavatar_release_amd.skinning import _ptrs              # noqa: E402
from _timing import emit, median_ms                         # noqa: E402


def reference_expression(points, T, weights, idx, trans, R, t):
    J, V = T.shape[0], points[0].shape[0]
    tmv = torch.matmul(weights[idx, :], T.view(J, 16)).view(V, 4, 4)
    outs = []
    for x in points:
        xyz = torch.cat((x, torch.ones_like(x[:, :1])), 1)
        xyz = torch.bmm(tmv, xyz[:, :, None]).view(V, 4)[:, :3] + trans
        outs.append(torch.matmul(torch.inverse(R), (xyz - t.view(1, 3)).permute(1, 0)).permute(1, 0))
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--points', type=int, default=167000)
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_skin_times.py needs a ROCm device')
    dev = torch.device('cuda:0')
    V, J = args.points, 55
    gen = torch.Generator().manual_seed(3)
    pts = scenes.dist_b_avatar(V, seed=1)['mean_3d']
    sub = torch.randperm(V, generator=gen)[:10475]
    nn = exa.knn_points(pts[None].to(dev), pts[sub][None].to(dev), K=1).idx[0, :, 0].cpu()
    idx = sub[nn]
    mask = (pts[:, 1] > pts[:, 1].max() - 0.3) | (pts[:, 0].abs() > 0.55 * pts[:, 0].abs().max())
    idx[mask] = torch.arange(V)[mask]
    W = torch.zeros(V, J)
    W.scatter_(1, torch.argsort(torch.rand(V, J, generator=gen), 1)[:, :4],
               torch.softmax(torch.randn(V, 4, generator=gen), 1))
    T = lbs.joint_transforms(lbs.axis_angle_to_matrix(0.3 * torch.randn(J, 3, generator=gen)),
                             0.3 * torch.randn(J, 3, generator=gen))
    R = torch.linalg.qr(torch.randn(3, 3, generator=gen))[0]
    t = torch.randn(3, generator=gen)
    to = lambda x: x.to(dev).contiguous()      # noqa: E731
    points = [to(pts).requires_grad_(True), to(pts + 0.003 * torch.randn(V, 3, generator=gen)).requires_grad_(True)]
    T, W, idx, R, t = to(T).requires_grad_(True), to(W), to(idx), to(R), to(t)
    trans = to(0.3 * torch.randn(1, 3, generator=gen)).requires_grad_(True)
    grads = [to(torch.randn(V, 3, generator=gen)) for _ in range(2)]
    inputs = [T, trans] + points
    res = {'build_digest': build._digest()[:12], 'device': torch.cuda.get_device_name(0), 'V': V, 'J': J, 'S': 2,
           'camera_step': True, 'distinct_weight_rows': int(torch.unique(idx).numel())}

    Rinv = torch.inverse(R).contiguous()
    nbytes = _lib.skin_workspace_size(V, J)
    ws = _workspace(nbytes, dev)
    gp = [torch.empty_like(p) for p in points]
    gT = torch.empty_like(T)
    gtr = torch.empty(3, device=dev)
    det = [p.detach() for p in points]

    def hip_bwd():
        _lib.SKIN.check(_lib.load().exa_skin_backward(V, 2, J, V, _ptrs(det), _ptr(W), _ptr(idx), _ptr(T.detach()),
                                                      _ptr(Rinv), _ptrs(grads), _ptrs(gp), _ptr(gT), _ptr(gtr), _ptr(ws),
                                                      nbytes, _stream_ptr(dev)))

    with torch.no_grad():
        res['hip_fwd_ms'] = median_ms(lambda: exa.skin_points(points, T, W, idx, trans, R, t), args.reps, 5)
        res['ref_fwd_ms'] = median_ms(lambda: reference_expression(points, T, W, idx, trans, R, t), args.reps, 5)
    res['hip_bwd_ms'] = median_ms(hip_bwd, args.reps, 5)
    ref_out = reference_expression(points, T, W, idx, trans, R, t)
    res['ref_bwd_ms'] = median_ms(lambda: torch.autograd.grad(ref_out, inputs, grads, retain_graph=True), args.reps, 5)
    res['hip_fwd_bwd_ms'] = median_ms(
        lambda: torch.autograd.grad(exa.skin_points(points, T, W, idx, trans, R, t), inputs, grads), args.reps, 5)
    res['ref_fwd_bwd_ms'] = median_ms(
        lambda: torch.autograd.grad(reference_expression(points, T, W, idx, trans, R, t), inputs, grads), args.reps, 5)
    res['speedup_fwd'] = res['ref_fwd_ms'] / res['hip_fwd_ms']
    res['speedup_bwd'] = res['ref_bwd_ms'] / res['hip_bwd_ms']
    res['speedup_fwd_bwd'] = res['ref_fwd_bwd_ms'] / res['hip_fwd_bwd_ms']
    with torch.no_grad():
        ours = exa.skin_points(points, T, W, idx, trans, R, t)
        ref = reference_expression(points, T, W, idx, trans, R, t)
        res['fwd_max_abs_diff_vs_ref'] = max(float((a - b).abs().max()) for a, b in zip(ours, ref))
    emit(res, args.out)


if __name__ == '__main__':
    main()
