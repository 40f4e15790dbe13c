"""The triplane lookup on the MI355X: HIP-event medians after warm-up, at the reference shape (167 000 rows of the
synthetic avatar with a head subset as the face rows, C = 32, 128 x 128 planes, tests/test_gpu_triplane.py's _avatar):

  hip_fwd_ms       TriplaneFeatures forward (one launch).
  hip_bwd_ms       its backward alone (exa_triplane_backward, one launch).
  hip_fwd_bwd_ms   forward + autograd backward through TriplaneFeatures.
  ref_fwd_ms       the reference's PyTorch expression (extract_tri_feature: means, six F.grid_sample, cat, permute, the
                   face rows assigned).
  ref_fwd_bwd_ms   the same plus its autograd backward (grid_sample's atomic input gradient).

Also the plan's build time (once per model), list statistics, and whether the HIP forward matches the reference
expression within 2e-6.  Prints one JSON line; --out writes it to a file too.

    python tools/gpu_triplane_times.py [--reps 50] [--out triplane_times.json]
"""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import exavatar_release_amd as exa                          # noqa: E402
from exavatar_release_amd import _lib, build, scenes         # noqa: E402
from exavatar_release_amd.rasterizer import _ptr, _stream_ptr  # noqa: E402
from _timing import emit, median_ms                         # noqa: E402


def reference_expression(xyz, is_face, triplane, triplane_face, shape_3d=(2, 2, 2), face_shape_3d=(0.3, 0.3, 0.3)):
    def feats(planes, xyz, ext):
        xyz = xyz - torch.mean(xyz, 0)[None, :]
        x, y, z = xyz[:, 0] / (ext[0] / 2), xyz[:, 1] / (ext[1] / 2), xyz[:, 2] / (ext[2] / 2)
        out = []
        for k, grid in enumerate((torch.stack((x, y), 1), torch.stack((x, z), 1), torch.stack((y, z), 1))):
            out.append(F.grid_sample(planes[k, None], grid[None, :, None, :], align_corners=False)[0, :, :, 0])
        return torch.cat(out).permute(1, 0)

    tri_feat = feats(triplane, xyz, shape_3d)
    tri_feat[is_face] = feats(triplane_face, xyz[is_face, :], face_shape_3d)
    return tri_feat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rows', type=int, default=167000)
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_triplane_times.py needs a ROCm device')
    dev = torch.device('cuda:0')
    xyz = scenes.dist_b_avatar(args.rows, seed=1)['mean_3d']
    is_face = (xyz[:, 1] > xyz[:, 1].max() - 0.3).to(dev)
    xyz = xyz.to(dev)
    g = torch.Generator().manual_seed(0)
    body = (torch.randn(3, 32, 128, 128, generator=g)).to(dev).requires_grad_(True)
    face = (torch.randn(3, 32, 128, 128, generator=g)).to(dev).requires_grad_(True)
    gout = torch.randn(args.rows, 96, generator=g).to(dev)
    torch.cuda.synchronize()
    t = time.perf_counter()
    tf = exa.TriplaneFeatures(xyz, is_face)
    torch.cuda.synchronize()
    plan_ms = (time.perf_counter() - t) * 1e3
    p = tf.plan
    lens = p.list_lengths.float()
    res = {'build_digest': build._digest()[:12], 'device': torch.cuda.get_device_name(0), 'rows': args.rows,
           'face_rows': int(is_face.sum()), 'C': 32, 'H': 128, 'W': 128, 'plan_build_ms': plan_ms,
           'seg_len': p.seg_len, 'num_wg': p.num_wg, 'max_wg_segments': p.max_wg_segments,
           'max_list': int(lens.max()), 'mean_nonempty_list': float(lens[lens > 0].mean())}
    gb = torch.empty_like(body)
    gf = torch.empty_like(face)

    def hip_bwd():
        _lib.TRIPLANE.check(_lib.load().exa_triplane_backward(
            tf.num_rows, 32, 128, 128, _ptr(tf.coords), _ptr(gout), _ptr(p.entries), _ptr(p.seg_entry), _ptr(p.tex_seg),
            _ptr(p.wg_tex), p.num_wg, p.max_wg_segments, _ptr(gb), _ptr(gf), _stream_ptr(dev)))

    with torch.no_grad():
        res['hip_fwd_ms'] = median_ms(lambda: tf(body, face), args.reps, 5)
        res['ref_fwd_ms'] = median_ms(lambda: reference_expression(xyz, is_face, body, face), args.reps, 5)
    res['hip_bwd_ms'] = median_ms(hip_bwd, args.reps, 5)
    res['hip_fwd_bwd_ms'] = median_ms(lambda: torch.autograd.grad(tf(body, face), (body, face), gout), args.reps, 5)
    res['ref_fwd_bwd_ms'] = median_ms(
        lambda: torch.autograd.grad(reference_expression(xyz, is_face, body, face), (body, face), gout), args.reps, 5)
    res['speedup_fwd'] = res['ref_fwd_ms'] / res['hip_fwd_ms']
    res['speedup_fwd_bwd'] = res['ref_fwd_bwd_ms'] / res['hip_fwd_bwd_ms']
    with torch.no_grad():
        d = (tf(body, face) - reference_expression(xyz, is_face, body, face)).abs().max().item()
    res['fwd_max_abs_diff_vs_ref'] = d
    res['fwd_within_2e-6'] = bool(d <= 2e-6)
    emit(res, args.out)


if __name__ == '__main__':
    main()
