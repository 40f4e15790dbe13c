"""Times the face-texture unwrap (exavatar_release_amd.XY2UV.forward and TextureUnwrap.add) at the reference's sizes
(fitting/main/config.py): image 256 x 256, UV map 512 x 512, C = 3, B = 1 and 8, on a FLAME-sized mesh (5 124 vertices,
10 240 faces: tests/mesh_oracle.flame_sized_scene).  ASSUMED frame and mesh: FLAME's own UV atlas is licensed data and is
not here; the stand-in atlas is a spherical map of two spheres, so its charts overlap.

The yardstick is the operation sequence of the reference's XY2UV.forward (fitting/common/nets/layer.py:53-102) restated in
torch on the same device -- per item a torch.unique over the raster, two boolean-mask assignments, three gathers of vertex
ids and three of 2-D points, then grid_sample and four full-map passes -- with the SAME image raster
(exa.get_face_index_map_xy) on both sides, and for the accumulation the three lines of fitting/main/unwrap.py:78-83 with
their two device-to-host copies.

Method: device events around `--iters` calls per window, `--rounds` windows per variant, the variants alternating inside
each round; reported are the median and the spread (max - min) of the windows.  A gain counts as established only beyond
three times the larger spread.  Kernel launches per call are counted with torch.profiler in a run after the timing.
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import exavatar_release_amd as exa  # noqa: E402
from tests import mesh_oracle as mo  # noqa: E402


def torch_xy2uv(m, img, mesh_cam, face, face_dev, cam):
    """The reference's operation sequence on the device (module docstring); returns (uvmap, mask)."""
    B, C, H, W = img.shape
    Hu, Wu = m.uvmap_shape
    nF = face_dev.shape[0]
    pts = torch.stack((mesh_cam[:, :, 0] / mesh_cam[:, :, 2] * cam['focal'][:, None, 0] + cam['princpt'][:, None, 0],
                       mesh_cam[:, :, 1] / mesh_cam[:, :, 2] * cam['focal'][:, None, 1] + cam['princpt'][:, None, 1]), 2)
    p2f_xy = exa.get_face_index_map_xy(mesh_cam, face, cam, (H, W)).pix_to_face[:, :, :, 0]
    texel_face = m.pix_to_face_uv.view(-1)
    corners, hidden = [[], [], []], []
    for n in range(B):
        seen = torch.unique(p2f_xy[n])
        seen[seen != -1] = seen[seen != -1] - nF * n
        shown = torch.zeros(nF, device=img.device)
        shown[seen] = 1.0
        ids = face_dev.clone()
        ids[shown == 0, :] = -1
        vid = [ids[texel_face, k].view(Hu, Wu) for k in range(3)]
        hidden.append(vid[0] == -1)
        for k in range(3):
            corners[k].append(pts[n, vid[k].view(-1), :].view(Hu, Wu, 2))
    c0, c1, c2 = (torch.stack(c) for c in corners)
    hidden = torch.stack(hidden).float()
    b = m.bary_coords_uv
    pos = c0 * b[None, :, :, 0, None] + c1 * b[None, :, :, 1, None] + c2 * b[None, :, :, 2, None]
    grid = torch.stack((pos[:, :, :, 0] / (W - 1) * 2 - 1, pos[:, :, :, 1] / (H - 1) * 2 - 1), 3)
    uvmap = F.grid_sample(img, grid, align_corners=True)
    uvmap[m.pix_to_face_uv[None, None, :, :].repeat(B, C, 1, 1) == -1] = -1
    uvmap = uvmap * (1 - hidden)[:, None, :, :] - hidden[:, None, :, :]
    mask = uvmap != -1
    return uvmap * mask, mask


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3        # us per call


def launches(fn):
    """Device kernels per call, by torch.profiler; None when the profiler gives none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')
                and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())
        return n or None
    except Exception:       # noqa: BLE001  (a profiler that is not there leaves the count unmeasured)
        return None


def report(res, out):
    line = json.dumps(res)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(line + '\n')
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs a ROCm device'
    dev = torch.device('cuda:0')
    H = W = 256
    uvmap_shape = (512, 512)
    C = 3
    res = {'H': H, 'W': W, 'uvmap_shape': list(uvmap_shape), 'C': C, 'iters': a.iters, 'rounds': a.rounds,
           'mesh': 'ASSUMED: tests/mesh_oracle.flame_sized_scene (5 124 vertices, 10 240 faces, overlapping spherical atlas)'}
    m = None
    for B in (1, 8):
        sc = mo.flame_sized_scene(H, W, seed=0, N=B)
        if m is None:
            m = exa.XY2UV(sc['vertex_uv'].numpy(), sc['face_uv'].numpy(), uvmap_shape)
            uv_weight = (m.pix_to_face_uv >= 0).float()
        verts = sc['verts'].to(dev)
        face = sc['faces'].numpy()
        face_dev = sc['faces'].to(dev)
        cam = {'focal': sc['focal'].to(dev), 'princpt': sc['princpt'].to(dev)}
        img = mo.smooth_texture(B, C, H, W).float().to(dev)
        valid = torch.ones(B, device=dev)
        acc = exa.TextureUnwrap(m, uv_weight)
        host = {'t': 0, 'm': 0}

        def ours():
            m(img, verts, face, cam)

        def theirs():
            torch_xy2uv(m, img, verts, face, face_dev, cam)

        def ours_add():
            acc.add(img, verts, face, cam, valid)

        def theirs_add():
            t, k = torch_xy2uv(m, img, verts, face, face_dev, cam)
            t = t * uv_weight[None, None, :, :] * valid[:, None, None, None]
            k = k * uv_weight[None, None, :, :] * valid[:, None, None, None]
            host['t'] += t.sum(0).detach().cpu().numpy()
            host['m'] += k.sum(0).detach().cpu().numpy()

        variants = {'xy2uv': ours, 'torch_xy2uv': theirs, 'add': ours_add, 'torch_add': theirs_add}
        for fn in variants.values():
            for _ in range(3):
                fn()
        times = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                times[k].append(window(fn, a.iters))
        for k, t in times.items():
            res['B%d_%s_us_median' % (B, k)] = round(statistics.median(t), 2)
            res['B%d_%s_us_spread' % (B, k)] = round(max(t) - min(t), 2)
        got, ref = m(img, verts, face, cam), torch_xy2uv(m, img, verts, face, face_dev, cam)
        res['B%d_max_abs_diff' % B] = float((got[0] - ref[0]).abs().max())
        res['B%d_mask_differs' % B] = int((got[1] != ref[1]).sum())
        res['B%d_sampled_texels' % B] = int(got[1][:, 0].sum())
        report(res, a.out)                       # the timings are on record before the profiler is started
        for k, fn in variants.items():
            res['B%d_%s_launches' % (B, k)] = launches(fn)
    print(report(res, a.out))


if __name__ == '__main__':
    main()
