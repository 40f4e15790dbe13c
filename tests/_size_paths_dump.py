"""Helper of test_gpu_size_paths.py, run as ONE fresh child process: renders the cases of size_cases.LISTS forward only, in exact
mode (the two-stage protocol) and in capacity mode (the fused call), and saves what tests/_footprint_dump.py saves per case and
mode: the 64-byte Splat records the kernels read, the sub-tile ranges, the sorted ids of every list and the capacity."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _binning_dump import _lists                                              # noqa: E402
import size_cases as sc                                                       # noqa: E402

MODES = ('exact', 'capacity')


def render(assets, cam, H, W, dev, mode, capacity, out, tag):
    """One forward; returns the capacity it ran with."""
    import torch
    import exavatar_release_amd as exa
    from exavatar_release_amd import rasterizer as rz
    from exavatar_release_amd.renderer import _raster_job
    P = assets['mean_3d'].shape[0]
    exa.config.mode, exa.config.fixed_capacity, exa.config.keep_debug, exa.config.on_overflow = mode, capacity, True, 'retry'
    with torch.no_grad():
        job = _raster_job({k: v.to(dev) for k, v in assets.items()}, (H, W), {k: v.to(dev) for k, v in cam.items()}, None)
        rz.rasterize_gaussians_batch([job])
        torch.cuda.synchronize()
        rg, ids, cap = _lists(P, H, W)
        out[tag + '__records'] = rz._debug_last['geom'][:P * 64].cpu().numpy().view(np.uint32).reshape(P, 16).copy()
        out[tag + '__ranges'], out[tag + '__ids'], out[tag + '__capacity'] = rg, ids, np.int64(cap)
    return cap


def main(path):
    import torch
    dev = torch.device('cuda:0')
    out = {}
    for name in sc.LISTS:
        c = sc.BY_NAME[name]
        assets, cam = c.make()
        need = render(assets, cam, c.H, c.W, dev, 'exact', None, out, name + '__exact')
        render(assets, cam, c.H, c.W, dev, 'capacity', need + 128, out, name + '__capacity')
    np.savez(path, **out)


if __name__ == '__main__':
    main(sys.argv[1])
