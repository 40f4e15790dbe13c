"""Times the Phong-shaded mesh render (exavatar_release_amd.shade_mesh / render_mesh) of an SMPL-X-sized mesh
(tests/shade_oracle.smplx_sized_scene: 10 242 vertices, 20 480 faces) at 1080 x 1920 and 1024 x 1024, next to the
untextured exa_mesh_forward (pix_to_face, zbuf, bary) of the same scene.  Prints one JSON line (and writes it to --out):

  <scene>_shaded_us      shade_mesh: vertex normals + prep + bin + shaded raster, device time by events
  <scene>_untextured_us  exa_mesh_forward without a texture on the same scene, device time by events
  <scene>_ratio          the two above
  <scene>_render_mesh_us one render_mesh call, wall time including the device-to-host copies and the numpy composite

Per-kernel device time: run this under `rocprofv3 --kernel-trace --stats` (with --quick for a short trace)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import exavatar_release_amd as exa  # noqa: E402
from exavatar_release_amd import build, mesh  # noqa: E402
from tests import shade_oracle as so  # noqa: E402


def _time(fn, iters):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def _wall(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--quick', action='store_true', help='20 iterations (for a profiler run)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    iters = 20 if a.quick else a.iters
    dev = torch.device('cuda:0')
    res = {'lib_digest': build._digest()[:16], 'iters': iters}
    for H, W in ((1080, 1920), (1024, 1024)):
        key = '%dx%d' % (H, W)
        sc = so.smplx_sized_scene(H, W)
        verts = sc['verts'].to(dev)
        faces = sc['faces'].numpy()
        cam = {'focal': sc['focal'].to(dev), 'princpt': sc['princpt'].to(dev)}
        topo = mesh._topology(faces, verts.shape[1], dev)
        focal, princpt = mesh._camera(cam, 1, dev)
        bkg = np.ones((H, W, 3), dtype=np.float32) * 255
        cam1 = {'focal': sc['focal'][0].to(dev), 'princpt': sc['princpt'][0].to(dev)}

        def shaded():
            exa.shade_mesh(verts, faces, cam, (H, W))

        def untextured():
            mesh._forward(verts, topo, focal, princpt, H, W, None, None, True)

        def panel():
            exa.render_mesh(verts[0], faces, cam1, bkg)
        for fn in (shaded, untextured, panel):
            for _ in range(5):
                fn()
        res[key + '_shaded_us'] = _time(shaded, iters)
        res[key + '_untextured_us'] = _time(untextured, iters)
        res[key + '_ratio'] = res[key + '_shaded_us'] / res[key + '_untextured_us']
        res[key + '_render_mesh_us'] = _wall(panel, max(iters // 10, 5))
        _, p2f = exa.shade_mesh(verts, faces, cam, (H, W))
        res[key + '_covered_px'] = int((p2f >= 0).sum())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
