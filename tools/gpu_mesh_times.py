"""Times the face render (exavatar_release_amd.MeshRenderer) of a FLAME-sized mesh (5 124 vertices, 10 240 faces) at
1024 x 1024: forward and forward + backward, N = 1 and N = 2 meshes per launch, against the float64 oracle
(tests/mesh_oracle.py) run on the same GPU in chunks.  Prints one JSON line (and writes it to --out).

Per-kernel device time: run this under `rocprofv3 --kernel-trace --stats` (with --quick for a short trace)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import exavatar_release_amd as exa  # noqa: E402
from tests import mesh_oracle as mo  # noqa: E402


def _time(fn, iters):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3, (time.perf_counter() - t0) / iters * 1e6     # us (events), us (host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--quick', action='store_true', help='20 iterations, no oracle (for a profiler run)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    iters = 20 if a.quick else a.iters
    dev = torch.device('cuda:0')
    H = W = 1024
    res = {'H': H, 'W': W}
    for N in (1, 2):
        sc = mo.flame_sized_scene(H, W, seed=0, N=N)
        verts = sc['verts'].to(dev)
        tex = sc['texture'].to(dev)
        faces = sc['faces'].numpy()
        cam = {'focal': sc['focal'].to(dev), 'princpt': sc['princpt'].to(dev),
               'R': torch.eye(3, device=dev)[None].repeat(N, 1, 1), 't': torch.zeros(N, 3, device=dev)}
        mr = exa.MeshRenderer(sc['vertex_uv'].numpy(), sc['face_uv'].numpy())
        G = torch.randn(N, 4, H, W, device=dev)
        v = verts.clone().requires_grad_(True)

        def fwd():
            with torch.no_grad():
                mr(tex, verts, faces, cam, (H, W))

        def fwd_bwd():
            v.grad = None
            (mr(tex, v, faces, cam, (H, W)) * G).sum().backward()
        for fn in (fwd, fwd_bwd):
            for _ in range(5):
                fn()
        res['N%d_fwd_us' % N], res['N%d_fwd_host_us' % N] = _time(fwd, iters)
        res['N%d_fwd_bwd_us' % N], res['N%d_fwd_bwd_host_us' % N] = _time(fwd_bwd, iters)
        res['N%d_covered_px' % N] = int((mr(tex, verts, faces, cam, (H, W))[:, 0] != -1).sum())
        if not a.quick:
            vr = verts.double().requires_grad_(True)
            fu = mo.face_uvs_of(sc['vertex_uv'], sc['face_uv']).to(dev)

            def oracle():
                vr.grad = None
                out, _ = mo.render(vr, sc['faces'].to(dev), cam['focal'], cam['princpt'], H, W, tex, fu)
                (out * G.double()).sum().backward()
            oracle()
            res['N%d_oracle_fwd_bwd_us' % N], _ = _time(oracle, 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
