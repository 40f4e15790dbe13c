"""Developer tool: per-kernel HIP-event times of ONE SH-degree-3 training render (in-kernel SH colours) of config C3's
Gaussians at 1024 x 1024, eager launches: the SH instantiations of the per-Gaussian kernels.  python tools/gpu_sh_times.py [view]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import exavatar_release_amd as exa
from exavatar_release_amd import scenes, _lib
from exavatar_release_amd.rasterizer import GaussianRasterizationSettings, rasterize_gaussians
from exavatar_release_amd.camera import make_raster_matrices

dev = torch.device('cuda:0')
H = W = 1024
P = 150000
REPS = 20
view = int(sys.argv[1]) if len(sys.argv) > 1 else 0
assets = scenes.dist_b_avatar(P, seed=0)
sh = scenes.sh_from_rgb(assets['rgb'], 3, seed=0, rest_sigma=0.3).to(dev).contiguous().requires_grad_(True)
m3, sc, rot, op = [assets[k].to(dev).requires_grad_(True) for k in ('mean_3d', 'scale', 'rotation', 'opacity')]
m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
G = torch.randn(3, H, W, device=dev)
tanx, tany, vm, pm, cpos = make_raster_matrices(scenes.ring_camera(H, W, view, 200), (H, W))
st = GaussianRasterizationSettings(H, W, tanx, tany, torch.ones(3, device=dev), 1.0, vm.to(dev), pm.to(dev), 3, cpos.to(dev), False, False)
exa.config.mode = 'exact'
acc = {}
for rep in range(3 + REPS):
    _lib.timing_enable(rep >= 3)
    color = rasterize_gaussians(m3, m2, sh, None, op, sc, rot, None, st)[0]
    torch.autograd.grad([color], [m3, sc, rot, op, sh, m2], grad_outputs=[G])
    torch.cuda.synchronize()
    if rep >= 3:
        for n, v in _lib.timing_read().items():
            acc[n] = acc.get(n, 0.0) + v / REPS * 1e3
print('SH3 view %d  ' % view + '  '.join('%s=%.1f' % (kk, vv) for kk, vv in acc.items()) + '  total=%.1f us' % sum(acc.values()))
