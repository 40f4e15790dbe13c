"""Helper of test_gpu_binning_masks.py (run as a subprocess so that the library reads EXA_BIN_SINGLE_CELLS afresh): renders
every case of CASES -- the smallest scenes at which the entry-parallel scatter and the mask-ready counting of
csrc/binning.hip can go wrong -- in exact mode (scans in their own launches) and in capacity mode (scans merged into the
scatter; forward + backward), and saves the sub-tile ranges, the sorted ids of every list, the images and the gradients.

A scene is a set of splats given in PIXELS (centre, per-axis sigma, rotation about the view axis) under a pinhole camera
looking down +z; a sigma of s px reaches alpha >= 1/255 out to ~3.3 s px at opacity 1."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import exavatar_release_amd as exa                                          # noqa: E402
from exavatar_release_amd import rasterizer as rz, stats                      # noqa: E402
from exavatar_release_amd.camera import make_raster_matrices                 # noqa: E402

FOCAL = 2000.0


def splats(px, py, sig, z=None, angle=None, opacity=1.0, seed=0):
    """px, py: centres in pixels; sig: (P,) isotropic or (P, 2) sigmas in px along / across `angle` (radians)."""
    rng = np.random.RandomState(seed)
    px, py = np.atleast_1d(np.asarray(px, np.float64)), np.atleast_1d(np.asarray(py, np.float64))
    P = len(px)
    z = (2.0 + 4.0 * rng.permutation(P) / P) if z is None else np.broadcast_to(np.asarray(z, np.float64), (P,))
    sig = np.asarray(sig, np.float64)
    sig = np.broadcast_to(sig if sig.ndim == 2 else sig.reshape(-1, 1), (P, 2)).copy()
    angle = np.zeros(P) if angle is None else np.broadcast_to(np.asarray(angle, np.float64), (P,))
    return dict(px=px, py=py, z=z, sig=sig, angle=angle, opacity=np.full((P, 1), opacity), rgb=rng.rand(P, 3))


def cat(*parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def _cases():
    rng = np.random.RandomState(7)
    c = {}
    # P = 1, the splat inside one sub-tile
    c['one_subtile'] = ((128, 128), [splats([19.5], [27.5], 0.85)])
    # one splat centred on a four-cell corner
    c['four_cell_corner'] = ((128, 128), [splats([64.0], [64.0], 4.0)])
    # a second chunk that holds a single Gaussian
    c['second_chunk_of_one'] = ((128, 128), [splats(4 + 120 * rng.rand(1025), 4 + 120 * rng.rand(1025), 1.0 + 2.0 * rng.rand(1025), seed=1)])
    # border cells with padding sub-tiles; 2 x 1 cells (the column walk's two-cells-per-thread branch) and 3 x 1 (the other)
    c['border_72x40'] = ((40, 72), [splats(72 * rng.rand(300), 40 * rng.rand(300), 0.8 + 3.0 * rng.rand(300), seed=2)])
    c['border_136x40'] = ((40, 136), [splats(136 * rng.rand(300), 40 * rng.rand(300), 0.8 + 3.0 * rng.rand(300), seed=3)])
    # 5 000 small splats inside ONE cell: five parts, five chunks
    c['crowded_cell'] = ((128, 128), [splats(64 + 8 + 48 * rng.rand(5000), 8 + 48 * rng.rand(5000), 0.65 + 0.3 * rng.rand(5000), seed=4)])
    # 600 splats over the four-cell corner: 2 400 entries from one chunk, three tiles of the entry walk
    c['corner_crowd'] = ((128, 128), [splats(64 + 2 * (rng.rand(600) - 0.5), 64 + 2 * (rng.rand(600) - 0.5), 2.5 + rng.rand(600),
                                             opacity=0.3, seed=5)])
    # one splat over the whole image: 16 cells from one Gaussian (plus small ones, so that ids and ranks mix)
    c['whole_image'] = ((256, 256), [cat(splats(256 * rng.rand(40), 256 * rng.rand(40), 1.5, seed=6),
                                         splats([128.0], [128.0], 200.0, z=7.0, opacity=0.9),
                                         splats(256 * rng.rand(40), 256 * rng.rand(40), 1.5, seed=8))])
    # needles at several angles (a conic at the edge of the footprint arithmetic: NaN / degenerate rows keep everything)
    ang = np.deg2rad([0.0, 30.0, 45.0, 90.0, 135.0, 0.0, 45.0])
    sig = np.array([[300.0, 0.01]] * 5 + [[3000.0, 1e-4]] * 2)
    c['needles'] = ((128, 128), [splats([64, 50, 64, 70, 64, 30, 90], [64, 70, 64, 50, 64, 100, 20], sig, angle=ang, seed=9)])
    # two jobs with different P in one call (the lists recorded are the last job's)
    c['batch_of_two'] = ((128, 128), [splats(128 * rng.rand(3000), 128 * rng.rand(3000), 0.8 + 3.0 * rng.rand(3000), seed=10),
                                      splats(128 * rng.rand(700), 128 * rng.rand(700), 0.8 + 6.0 * rng.rand(700), seed=11)])
    c['batch_of_two_swapped'] = ((128, 128), c['batch_of_two'][1][::-1])
    return c


CASES = _cases()
OVERFLOW_CASE = 'second_chunk_of_one'          # also rendered into a buffer of 64 instances: overflow, then the repair


def _job(sc, H, W, dev, grad):
    z = sc['z'].astype(np.float32).astype(np.float64)
    x, y = (sc['px'] - (W - 1) / 2) * z / FOCAL, (sc['py'] - (H - 1) / 2) * z / FOCAL
    P = len(z)
    f32 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev).requires_grad_(grad)   # noqa: E731
    scales = np.concatenate([sc['sig'], sc['sig'][:, 1:]], 1) * (z / FOCAL)[:, None]
    rot = np.stack([np.cos(sc['angle'] / 2), np.zeros(P), np.zeros(P), np.sin(sc['angle'] / 2)], 1)
    cam = {'R': torch.eye(3), 't': torch.zeros(3), 'focal': torch.tensor([FOCAL, FOCAL]), 'princpt': torch.tensor([W / 2.0, H / 2.0])}
    tanx, tany, vm, pm, cp = make_raster_matrices(cam, (H, W))
    rs = exa.GaussianRasterizationSettings(H, W, tanx, tany, torch.tensor([0.1, 0.3, 0.2], device=dev), 1.0, vm.to(dev), pm.to(dev),
                                           0, cp.to(dev), False, False)
    return dict(raster_settings=rs, means3D=f32(np.stack([x, y, z], 1)), means2D=torch.zeros(P, 3, device=dev, requires_grad=grad),
                shs=None, colors_precomp=f32(sc['rgb']), opacities=f32(sc['opacity']), scales=f32(scales), rotations=f32(rot),
                cov3D_precomp=None)


GRAD_KEYS = ('means3D', 'means2D', 'colors_precomp', 'opacities', 'scales', 'rotations')


def _lists(P, H, W):
    dbg = rz._debug_last
    tile, binws, cap = dbg['tile'].cpu().numpy(), dbg['bin'].cpu().numpy(), int(dbg['capacity'])
    lay, bins = stats.tile_offsets(P, W, H), stats.bin_offsets(cap)
    nsub = lay['cells'] * 64
    rg = tile[lay['ranges'][0]:lay['ranges'][0] + nsub * 8].view(np.uint32).reshape(-1, 2).copy()
    order = binws[bins['sorted'][0]:bins['sorted'][0] + cap * 4].view(np.uint32)
    ids = [order[b:e] for b, e in rg.astype(np.int64) if e > b]
    return rg, (np.concatenate(ids) if ids else np.zeros(0, np.uint32)), cap


def render(scenes_, H, W, dev, mode, capacity, out, tag):
    grad = mode == 'capacity'
    jobs = [_job(sc, H, W, dev, grad) for sc in scenes_]
    exa.config.mode, exa.config.fixed_capacity, exa.config.keep_debug, exa.config.on_overflow = mode, capacity, True, 'retry'
    with torch.set_grad_enabled(grad):
        outs = rz.rasterize_gaussians_batch(jobs)
        torch.cuda.synchronize()
        rg, ids, cap = _lists(len(scenes_[-1]['z']), H, W)
        out[tag + '__ranges'], out[tag + '__ids'] = rg, ids
        for k, o in enumerate(outs):
            for name, t in zip(('color', 'radii', 'depth', 'alpha'), o):
                out['%s__job%d_%s' % (tag, k, name)] = t.detach().cpu().numpy()
        if grad:
            g = torch.Generator().manual_seed(5)
            loss = 0.0
            for o in outs:
                loss = loss + sum((t * torch.randn(t.shape, generator=g).to(dev)).sum() for t in (o[0], o[2], o[3]))
            loss.backward()
            for k, j in enumerate(jobs):
                for name in GRAD_KEYS:
                    out['%s__job%d_grad_%s' % (tag, k, name)] = j[name].grad.cpu().numpy()
    return cap


def main(path):
    dev = torch.device('cuda:0')
    if os.environ.get('EXA_TEST_POISON'):
        exa.config.poison = True
    out = {}
    for name, ((H, W), scenes_) in CASES.items():
        # exact mode measures what every job needs; capacity mode gets that and some unused batch slots behind the lists
        needs = [render([sc], H, W, dev, 'exact', None, {}, '') for sc in scenes_]
        render(scenes_, H, W, dev, 'exact', None, out, name + '__exact')
        render(scenes_, H, W, dev, 'capacity', [n + 128 for n in needs], out, name + '__capacity')
        if name == OVERFLOW_CASE:
            rz.overflow_events.clear()
            render(scenes_, H, W, dev, 'capacity', 64, out, name + '__overflow')
            out[name + '__overflow__events'] = np.array([[e[1], e[2]] for e in rz.overflow_events], dtype=np.int64).reshape(-1, 2)
    np.savez(path, **out)


if __name__ == '__main__':
    main(sys.argv[1])
