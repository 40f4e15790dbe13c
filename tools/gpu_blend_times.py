"""The blend-shape offsets on the MI355X, against the reference's two expressions run by PyTorch on the same device in
the same process with the FULL tables: V = 167 281 (the reference's upsampled human mesh), pose_dirs [486, 3 V] (976 MB),
expr_dirs [V, 3, 50] (100 MB).  Every figure is the median over --reps windows of the time per call, each window --iters
calls between two HIP events after a warm-up; the windows of all rows alternate.

  pose{40,100}_{ref,hip}_fwd_ms       module.py:484-493 forward alone (no_grad): 40 % of the vertices masked, and all of
                                      them -- the dense case moves the reference's bytes and shows what the kernel alone buys.
  pose{40,100}_{ref,hip}_fwd_bwd_ms   forward + autograd backward to mean_offset_offset (the pose is detached).
  expr_{ref,hip}_fwd_ms / _fwd_bwd_ms module.py:537 with 15 % of the rows non-zero; backward to expr.
  *_hip_fwd_GBps                      the compact table's bytes (K x N_pad x 4) over the hip forward time.
  speedup_*                           ref / hip of the same row.

The coverage shares are assumptions (the licensed SMPL-X assets are not here).  These are call times by HIP events on
the stream, launch overhead of the Python surface included; they are NOT per-kernel device times (no rocprofv3 run).
Prints one JSON line; --out writes it to a file too.

    python tools/gpu_blend_times.py [--reps 7] [--iters 100] [--out blend_times.json]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import exavatar_release_amd as exa                          # noqa: E402
from exavatar_release_amd import build                       # noqa: E402
from _timing import emit, medians                           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--vertices', type=int, default=167281)
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_blend_times.py needs a ROCm device')
    dev = torch.device('cuda:0')
    V, Kp, Ke = args.vertices, 486, 50
    g = torch.Generator(device=dev).manual_seed(5)
    rand = lambda *s: torch.randn(*s, generator=g, device=dev)      # noqa: E731
    pose_dirs = rand(Kp, 3 * V) * 0.02
    expr_dirs = rand(V, 3, Ke) * 0.05
    expr_dirs *= (torch.rand(V, generator=g, device=dev) < 0.15)[:, None, None]
    sel = torch.rand(V, generator=g, device=dev)
    masks = {'pose40': sel < 0.4, 'pose100': sel < 2.0}
    pose_feat = rand(1, Kp) * 0.3
    moo = (rand(V, 3) * 0.01).requires_grad_(True)
    expr = rand(Ke).requires_grad_(True)
    G1, G2 = rand(V, 3), rand(V, 3)
    res = {'build_digest': build._digest()[:12], 'device': torch.cuda.get_device_name(0), 'V': V, 'Kp': Kp, 'Ke': Ke,
           'reps': args.reps, 'iters': args.iters}

    fns, table_bytes, checks = {}, {}, {}
    for name, mask in masks.items():
        hip = exa.BlendShapes(pose_dirs, expr_dirs, mask)
        fmask = mask[:, None].float()
        table_bytes[name] = hip.pose_table.numel() * 4
        res[name + '_coverage'] = float(mask.float().mean())

        def ref_pose(fmask=fmask):
            # module.py:484-493
            offset = torch.matmul(pose_feat.detach(), pose_dirs).view(V, 3)
            masked = moo * (1 - fmask)
            return masked + offset * fmask, masked

        def hip_pose(hip=hip):
            return hip.pose_offsets(pose_feat, moo)

        for side, fn in (('ref', ref_pose), ('hip', hip_pose)):
            def fwd(fn=fn):
                with torch.no_grad():
                    return fn()

            def fwd_bwd(fn=fn):
                return torch.autograd.grad(list(fn()), moo, [G1, G2])
            fns['%s_%s_fwd_ms' % (name, side)] = fwd
            fns['%s_%s_fwd_bwd_ms' % (name, side)] = fwd_bwd
        with torch.no_grad():
            checks[name + '_max_abs_diff_vs_ref'] = float((hip_pose()[0] - ref_pose()[0]).abs().max())
    table_bytes['expr'] = hip.expr_table.numel() * 4
    res['expr_coverage'] = hip.expr_cols.numel() / (3.0 * V)

    def ref_expr():
        return (expr[None, None, :] * expr_dirs).sum(2)             # module.py:537

    def hip_expr(hip=hip):
        return hip.expr_offsets(expr)

    for side, fn in (('ref', ref_expr), ('hip', hip_expr)):
        def fwd(fn=fn):
            with torch.no_grad():
                return fn()

        def fwd_bwd(fn=fn):
            return torch.autograd.grad(fn(), expr, G1)
        fns['expr_%s_fwd_ms' % side] = fwd
        fns['expr_%s_fwd_bwd_ms' % side] = fwd_bwd
    with torch.no_grad():
        checks['expr_max_abs_diff_vs_ref'] = float((hip_expr() - ref_expr()).abs().max())
    g_hip, g_ref = torch.autograd.grad(hip_expr(), expr, G1)[0], torch.autograd.grad(ref_expr(), expr, G1)[0]
    checks['expr_grad_max_abs_diff_vs_ref'] = float((g_hip - g_ref).abs().max())
    checks['expr_grad_max_abs'] = float(g_ref.abs().max())
    checks['hip_expr_grad_elements_differing_between_two_calls'] = int(
        (torch.autograd.grad(hip_expr(), expr, G1)[0] != g_hip).sum())

    med, spread = medians(fns, args.reps, args.iters)
    res.update(med)
    res['min_max_ms'] = {k: [round(a, 5), round(b, 5)] for k, (a, b) in spread.items()}
    for k in list(med):
        if '_hip_' in k:
            res['speedup_' + k.replace('_hip_', '_')[:-3]] = med[k.replace('_hip_', '_ref_')] / med[k]
    for name, nbytes in table_bytes.items():
        res[name + '_table_bytes'] = nbytes
        res[name + '_hip_fwd_GBps'] = nbytes / (med[name + '_hip_fwd_ms'] * 1e-3) / 1e9
    res['pose_dirs_bytes'] = pose_dirs.numel() * 4
    res['ref_pose_fwd_GBps_of_full_table'] = pose_dirs.numel() * 4 / (med['pose100_ref_fwd_ms'] * 1e-3) / 1e9
    res.update(checks)
    emit(res, args.out)


if __name__ == '__main__':
    main()
