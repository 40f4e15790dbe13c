"""The arm and hand regularisers on the MI355X, against the reference expressions run by PyTorch on the same device in
the same process.  V = 167 281 (a 409 x 409 grid, the size of the reference's upsampled human mesh), B = 1.

The arm case is the two-tube mesh of tests/reg_oracle.py at 120 rings x 64 per arm: L = 10 320 lower-arm and U = 5 040
upper-arm vertices (53 M pairs).  THESE SIZES ARE ASSUMED: the SMPL-X model files are not available, so the true L and
U of the reference's arms are not known.  The hand case takes 2 x 12 000 hand vertices.

Every figure is the median over --reps windows of the time per call, each window a number of calls between two HIP
events after a warm-up (--iters for the HIP side, --ref-iters for the reference side, whose arm call takes tens of
milliseconds and synchronises the host).

  {ref,hip}_arm_fwd_ms / _fwd_bwd_ms        ArmRGBReg as the reference calls it: the neighbour sets are found per call
                                            (hip: ``ArmRGBReg().forward`` with a NEW mesh version per call, so no plan is reused).
  hip_arm_plan_ms                           ``arm_neighbors`` alone;  hip_arm_loss_fwd_ms / _fwd_bwd_ms  ``arm_rgb_loss`` on a plan.
  {ref,hip}_hand_rgb_fwd_ms / _fwd_bwd_ms   HandRGBReg.
  {ref,hip}_hand_mean_fwd_ms / _fwd_bwd_ms  HandMeanReg (ref: normals per call, as the reference; hip: ``normal=`` given).
  {ref,hip}_block_ms                        model.py:223,249-251 with their ``.mean()``s and the backward to the two colour
                                            and the two offset tensors.  ref: as the reference calls it -- three normals
                                            calls, the neighbour sets twice.  hip: one normals call, one plan.  Both
                                            sides compute ``get_arm``'s masks inside the block and then use the prepared
                                            two-tube masks (the grid's normals do not describe the tubes).
  speedup_*                                 ref / hip of the same row.

Prints one JSON line; --out writes it to a file too.

    python tools/gpu_reg_times.py [--reps 5] [--iters 50] [--ref-iters 3] [--out reg_times.json]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import exavatar_release_amd as exa                          # noqa: E402
from exavatar_release_amd import build                       # noqa: E402
from exavatar_release_amd.p3d_standins import Meshes         # noqa: E402
from _timing import emit, medians                           # noqa: E402


def grid_faces(rows, cols):
    r, c = np.meshgrid(np.arange(rows - 1), np.arange(cols - 1), indexing='ij')
    a = (r * cols + c).reshape(-1)
    return np.concatenate([np.stack([a, a + 1, a + cols], 1), np.stack([a + 1, a + cols + 1, a + cols], 1)]).astype(np.int64)


def two_tubes(rings, per_ring, rng):
    theta = 2 * np.pi * np.arange(per_ring) / per_ring
    pts, upper = [], []
    for x0 in (0.2, -0.2):
        for r in range(rings):
            x = x0 + 0.004 * r * np.sign(x0)
            pts.append(np.stack([np.full(per_ring, x), 0.04 * np.sin(theta), 0.04 * np.cos(theta)], 1))
            upper.append(np.sin(theta) > 0.5)
    pts = np.concatenate(pts)
    return pts + rng.uniform(-5e-4, 5e-4, size=pts.shape), np.concatenate(upper)


# ---- the reference side: the same operations as loss.py:148-197 and smpl_x.py:139-148, in PyTorch ------------------------
def ref_normals(mesh, face_t):
    return Meshes(verts=mesh[None], faces=face_t[None]).verts_normals_packed().reshape(-1, 3).detach()


def ref_arm(mesh, is_upper, is_lower, rgb):
    up, lo = mesh[is_upper], mesh[is_lower]
    near = (torch.abs(lo[:, None, 0] - up[None, :, 0]) < 0.01).float()
    count = int(torch.min(near.sum(1)))
    dist = torch.sqrt(torch.sum((lo[:, None, :] - up[None, :, :]) ** 2, 2))
    dist = dist * near + 9999 * (1 - near)
    k = min(50, count)
    pick = torch.topk(dist, k=k, dim=1, largest=False, sorted=False)[1]
    src = torch.arange(mesh.shape[0], device=mesh.device)[is_upper][pick].view(-1)
    target = rgb[:, src, :].view(rgb.shape[0], int(is_lower.sum()), k, 3).mean(2).detach()
    return (rgb[:, is_lower, :] - target) ** 2


def ref_hand_rgb(rgb, is_r, is_l):
    r, l = rgb[:, is_r, :], rgb[:, is_l, :]
    return (r - r.mean(1)[:, None, :].detach()) ** 2 + (l - l.mean(1)[:, None, :].detach()) ** 2


def ref_hand_mean(mesh, face_t, offset, is_r, is_l):
    hand = (is_r + is_l) > 0
    with torch.no_grad():
        normal = ref_normals(mesh, face_t)[None].repeat(offset.shape[0], 1, 1)
    return torch.clamp(torch.sum(normal * F.normalize(offset, p=2, dim=2), 2)[:, hand], min=0)


def ref_get_arm(mesh, face_t, weight, joints):
    normal = ref_normals(mesh, face_t)
    label = weight.argmax(1)
    is_arm = 0
    for j in joints:
        is_arm = is_arm + (label == j)
    is_arm = is_arm > 0
    return is_arm * (normal[:, 1] > math.cos(math.pi / 3)), is_arm * (normal[:, 1] <= math.cos(math.pi / 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--ref-iters', type=int, default=3)
    ap.add_argument('--grid', type=int, default=409)
    ap.add_argument('--rings', type=int, default=120)
    ap.add_argument('--hand', type=int, default=12000)
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_reg_times.py needs a ROCm device')
    dev = torch.device('cuda:0')
    V = args.grid * args.grid
    rng = np.random.RandomState(5)
    face = grid_faces(args.grid, args.grid)
    face_t = torch.from_numpy(face).to(dev)
    yy, xx = np.meshgrid(np.arange(args.grid), np.arange(args.grid), indexing='ij')
    verts = np.stack([2.0 + xx.reshape(-1) * 0.004, yy.reshape(-1) * 0.004, rng.uniform(-1e-3, 1e-3, V)], 1)
    tubes, upper = two_tubes(args.rings, 64, rng)
    n_arm = tubes.shape[0]
    verts[:n_arm] = tubes
    is_upper, is_lower = np.zeros(V, dtype=bool), np.zeros(V, dtype=bool)
    is_upper[:n_arm], is_lower[:n_arm] = upper, ~upper
    perm = rng.permutation(np.arange(n_arm, V))
    is_r, is_l = np.zeros(V, dtype=bool), np.zeros(V, dtype=bool)
    is_r[perm[:args.hand]] = True
    is_l[perm[args.hand:2 * args.hand]] = True
    joints = [16, 17, 18, 19]
    weight = rng.uniform(0, 1, (V, 55)).astype(np.float32)
    weight[:n_arm, joints[0]] = 2.0

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    mesh = t(verts.astype(np.float32))
    is_upper, is_lower, is_r, is_l, weight = t(is_upper), t(is_lower), t(is_r), t(is_l), t(weight)
    rgb1, rgb2 = (t(rng.uniform(0, 1, (1, V, 3)).astype(np.float32)).requires_grad_(True) for _ in range(2))
    off1, off2 = (t((rng.standard_normal((1, V, 3)) * 0.01).astype(np.float32)).requires_grad_(True) for _ in range(2))
    L, U = int(is_lower.sum()), int(is_upper.sum())
    G_arm, G_rgb, G_mean = torch.randn(1, L, 3, device=dev), torch.randn(1, args.hand, 3, device=dev), \
        torch.randn(1, 2 * args.hand, device=dev)
    res = {'build_digest': build._digest()[:12], 'device': torch.cuda.get_device_name(0), 'V': V, 'L': L, 'U': U,
           'hand': args.hand, 'sizes_assumed': True, 'reps': args.reps, 'iters': args.iters, 'ref_iters': args.ref_iters}

    arm, hand_rgb, hand_mean = exa.ArmRGBReg(), exa.HandRGBReg(), exa.HandMeanReg(face)
    normal = exa.vertex_normals(mesh, face)
    plan = exa.arm_neighbors(mesh, is_upper, is_lower)

    def hip_arm():
        mesh.add_(0.0)                                          # a new version: the plan is rebuilt, as per call in the reference
        return arm(mesh, is_upper, is_lower, rgb1)

    def grad_of(fn, x, G):
        return lambda: torch.autograd.grad(fn(), x, G)

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    pairs = {
        'arm': (lambda: ref_arm(mesh, is_upper, is_lower, rgb1), hip_arm, rgb1, G_arm),
        'hand_rgb': (lambda: ref_hand_rgb(rgb1, is_r, is_l), lambda: hand_rgb(rgb1, is_r, is_l), rgb1, G_rgb),
        'hand_mean': (lambda: ref_hand_mean(mesh, face_t, off1, is_r, is_l),
                      lambda: hand_mean(mesh, off1, is_r, is_l, normal=normal), off1, G_mean),
    }
    ref_fns, hip_fns = {}, {}
    for name, (ref, hip, x, G) in pairs.items():
        ref_fns['ref_%s_fwd_ms' % name], ref_fns['ref_%s_fwd_bwd_ms' % name] = no_grad(ref), grad_of(ref, x, G)
        hip_fns['hip_%s_fwd_ms' % name], hip_fns['hip_%s_fwd_bwd_ms' % name] = no_grad(hip), grad_of(hip, x, G)
    hip_fns['hip_arm_plan_ms'] = lambda: exa.arm_neighbors(mesh, is_upper, is_lower)
    hip_fns['hip_arm_loss_fwd_ms'] = no_grad(lambda: exa.arm_rgb_loss(plan, rgb1))
    hip_fns['hip_arm_loss_fwd_bwd_ms'] = grad_of(lambda: exa.arm_rgb_loss(plan, rgb1), rgb1, torch.randn(1, V, 3, device=dev))
    hip_fns['hip_normals_ms'] = lambda: exa.vertex_normals(mesh, face)

    def ref_block():
        mean_reg = ref_hand_mean(mesh, face_t, off1, is_l, is_r) + ref_hand_mean(mesh, face_t, off2, is_l, is_r)
        rgb_reg = (ref_hand_rgb(rgb1, is_r, is_l) + ref_hand_rgb(rgb2, is_r, is_l)) * 0.01
        ref_get_arm(mesh, face_t, weight, joints)
        arm_reg = (ref_arm(mesh, is_upper, is_lower, rgb1) + ref_arm(mesh, is_upper, is_lower, rgb2)) * 0.1
        return torch.autograd.grad(mean_reg.mean() + rgb_reg.mean() + arm_reg.mean(), [rgb1, rgb2, off1, off2])

    def hip_block():
        n = exa.vertex_normals(mesh, face)
        mean_reg = hand_mean(mesh, off1, is_l, is_r, normal=n) + hand_mean(mesh, off2, is_l, is_r, normal=n)
        rgb_reg = (hand_rgb(rgb1, is_r, is_l) + hand_rgb(rgb2, is_r, is_l)) * 0.01
        exa.get_arm(mesh, weight, face, joints, normal=n)
        p = exa.arm_neighbors(mesh, is_upper, is_lower)
        arm_reg = (exa.arm_rgb_loss(p, rgb1) + exa.arm_rgb_loss(p, rgb2)) * 0.1
        arm_mean = arm_reg.sum() / (3 * rgb1.shape[0] * p.count)           # .mean() over [B, L, 3] without a synchronisation
        return torch.autograd.grad(mean_reg.mean() + rgb_reg.mean() + arm_mean, [rgb1, rgb2, off1, off2])

    ref_fns['ref_block_ms'] = ref_block
    hip_fns['hip_block_ms'] = hip_block

    med, spread = medians(hip_fns, args.reps, args.iters)
    med_r, spread_r = medians(ref_fns, args.reps, args.ref_iters, warmup=2)
    med.update(med_r)
    spread.update(spread_r)
    res.update(med)
    res['min_max_ms'] = {k: [round(a, 5), round(b, 5)] for k, (a, b) in spread.items()}
    for k in med_r:
        res['speedup_' + k[4:-3]] = med_r[k] / med['hip_' + k[4:]]

    with torch.no_grad():
        res['arm_loss_max_abs_diff_vs_ref'] = float((hip_arm() - ref_arm(mesh, is_upper, is_lower, rgb1)).abs().max())
        res['hand_rgb_loss_max_abs_diff_vs_ref'] = float((hand_rgb(rgb1, is_r, is_l) - ref_hand_rgb(rgb1, is_r, is_l)).abs().max())
        res['hand_mean_loss_max_abs_diff_vs_ref'] = float((hand_mean(mesh, off1, is_r, is_l, normal=normal)
                                                           - ref_hand_mean(mesh, face_t, off1, is_r, is_l)).abs().max())
    res['k'], res['n_min'] = int(plan.k), int(plan.n_min)
    g_ref, g_hip = ref_block(), hip_block()
    res['block_grad_max_abs_diff_vs_ref'] = [float((a - b).abs().max()) for a, b in zip(g_ref, g_hip)]
    res['block_grad_max_abs'] = [float(a.abs().max()) for a in g_ref]
    emit(res, args.out)


if __name__ == '__main__':
    main()
