"""Helper of test_gpu_footprint_lists.py (run as a subprocess so that the library reads EXA_FOOTPRINT / EXA_BIN_SINGLE_CELLS
afresh) and case table of test_footprint_oracle.py: renders every case of CASES in exact mode and in capacity mode (forward
only) and saves, per case and mode, the 64-byte Splat records the kernels read (rasterizer._debug_last['geom'], taken after the
forward), the sub-tile ranges, the sorted ids of every list, the capacity and the image.

The cases are the smallest scenes that reach the branches of the footprint chain (csrc/preprocess_fwd.hip: sub-tile rect;
csrc/common.h make_footprint / footprint_band; csrc/binning.hip rows_mask), given in PIXELS like those of _binning_dump.py.
136 x 200 (H x W) is 4 x 3 cells with padding sub-tiles on both borders (25 x 17 sub-tiles); 128 x 128 is 2 x 2 cells, no padding."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _binning_dump import splats, cat, _job, _lists                           # noqa: E402

MODES = ('exact', 'capacity')
FAR_DISTANCES = (500.0, 1.0e4, 2.0e5)


def _logu(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _with_opacity(sc, op):
    sc['opacity'] = np.asarray(op, np.float64).reshape(-1, 1)
    return sc


def _cases():
    c = {}
    H, W = 136, 200
    # avatar-sized splats, centres up to 20 px outside every border, half of them translucent down to 255 o < 1
    rng = np.random.RandomState(101)
    n = 1500
    op = np.where(np.arange(n) % 2 == 0, 1.0, rng.uniform(0.004, 1.0, n))
    c['avatar'] = ((H, W), _with_opacity(splats(rng.uniform(-20, W + 20, n), rng.uniform(-20, H + 20, n),
                                                np.stack([_logu(rng, 0.3, 6.0, n), _logu(rng, 0.3, 6.0, n)], 1),
                                                angle=rng.uniform(0, np.pi, n), seed=1), op), {})
    # scene-sized splats: most rects span several cells, so the entry walk's further cells each get a mask with their own xm, ym
    rng = np.random.RandomState(102)
    n = 300
    op = np.where(np.arange(n) % 2 == 0, 1.0, rng.uniform(0.004, 1.0, n))
    c['scene'] = ((H, W), _with_opacity(splats(rng.uniform(-20, W + 20, n), rng.uniform(-20, H + 20, n),
                                               np.stack([_logu(rng, 3.0, 60.0, n), _logu(rng, 3.0, 60.0, n)], 1),
                                               angle=rng.uniform(0, np.pi, n), seed=2), op), {})
    # needles: long sigma up to 3 000 px, short sigma down to 1e-4; the first 48 at exactly 0, 45, 90 and 135 degrees
    rng = np.random.RandomState(103)
    n = 200
    ang = rng.uniform(0, np.pi, n)
    ang[:48] = np.deg2rad([0.0, 45.0, 90.0, 135.0] * 12)
    sig = np.stack([_logu(rng, 30.0, 3000.0, n), _logu(rng, 1e-4, 1.0, n)], 1)
    sig[:4], sig[4:8] = [3000.0, 1e-4], [300.0, 0.01]
    c['needles'] = ((H, W), splats(rng.uniform(0, W, n), rng.uniform(0, H, n), sig, angle=ang, seed=3), {})
    # one shape, its centre stepped in 1/8 px over 16 px across a sub-tile edge (40) and across the cell edge (64), in x and in y
    parts, step = [], np.arange(129) / 8.0
    for deg in (0.0, 30.0, 90.0):
        for start in (32.0, 56.0):
            for axis in (0, 1):
                fixed = np.full(129, 84.3)
                xy = (start + step, fixed) if axis == 0 else (fixed, start + step)
                parts.append(splats(xy[0], xy[1], np.array([[2.3, 1.1]]), angle=np.deg2rad(deg), seed=4))
    c['tangent_sweep'] = ((128, 128), cat(*parts), {})
    # opacities around the threshold 1/255 (thr -> 0: the ellipse shrinks to a point); centres on a pixel centre, on a sub-tile
    # corner, on the four-cell corner, and a pixel centre next to it
    ops = [(1 - 1e-6) / 255, 1.0 / 255, (1 + 1e-6) / 255, 1.01 / 255, 1.5 / 255, 0.99, 1.0]
    ctr = [(20.0, 20.0), (23.5, 39.5), (63.5, 63.5), (64.0, 63.0)]
    grid = [(o, x, y, s) for o in ops for (x, y) in ctr for s in (0.5, 2.0, 6.0, 25.0)]
    o, x, y, s = (np.array(v) for v in zip(*grid))
    c['threshold_opacity'] = ((128, 128), _with_opacity(splats(x, y, s, seed=5), o), {})
    # centres far outside the image with sigmas that reach in: at 500 px the interval margin grows with |x|; at 1e4 and 2e5 px
    # the +-1e6 clamps of the rect and of rows_mask are reached
    far = []
    for dist in FAR_DISTANCES:
        for k, (ux, uy) in enumerate([(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)]):
            for mult in (0.5, 1.5, 5.0, 50.0):
                for aniso in (False, True):
                    px = 63.5 + ux * (64 + dist) + (0.0 if ux else 11.3)         # `dist` px beyond the border
                    py = 63.5 + uy * (64 + dist) + (0.0 if uy else 7.9)
                    s0 = mult * dist
                    far.append((dist, px, py, s0, s0 / 3.0 if aniso else s0, np.deg2rad(30.0 * k) if aniso else 0.0,
                                1.0 if (k + aniso) % 2 else 0.5))
    dist, px, py, s0, s1, ang, op = (np.array(v) for v in zip(*far))
    c['far_centres'] = ((128, 128), _with_opacity(splats(px, py, np.stack([s0, s1], 1), angle=ang, seed=6), op), {'distance': dist})
    # a sigma-200 splat over all 12 cells, among 80 small ones
    rng = np.random.RandomState(107)
    c['one_huge'] = ((H, W), cat(splats(W * rng.rand(40), H * rng.rand(40), 1.5, seed=7),
                                 splats([100.0], [68.0], 200.0, z=7.0, opacity=0.9),
                                 splats(W * rng.rand(40), H * rng.rand(40), 1.5, seed=8)), {})
    return c


CASES = _cases()           # name -> ((H, W), scene, what the tests need to know about its splats)


def assert_case_has_teeth(name, cl, rec):
    """Conditions on the ORACLE's classes ``cl`` (footprint_oracle.classify of the records ``rec`` of case ``name``) without
    which the list tests would pass emptily.  Checked on the CPU model's records and again on the device's."""
    import footprint_oracle as fo
    n = fo.counts(cl)
    assert n['MUST'] > 0 and n['BAND'] <= 0.005 * n['MUST'], (name, n)
    if name in ('avatar', 'scene', 'needles'):
        assert n['MUST_NOT'] >= 0.2 * n['rect'], (name, n)
    r = fo.unpack(rec)
    P = len(r['px'])
    per = lambda k: np.bincount(cl['g'][cl['in_rect'] & (cl['cls'] == k)], minlength=P)                   # noqa: E731
    if name == 'tangent_sweep':
        both = (per(fo.MUST) > 0) & (per(fo.MUST_NOT) > 0)
        assert 2 * both.sum() >= P, (name, int(both.sum()), P)
    if name == 'far_centres':
        dist = CASES[name][2]['distance']
        for d in FAR_DISTANCES:
            assert per(fo.MUST)[dist == d].sum() >= 1, (name, d)
    if name == 'threshold_opacity':
        assert (r['n_inst'] == 0).any() and (r['n_inst'] == 1).any(), name
    if name == 'one_huge':
        assert r['n_inst'].max() == 25 * 17, name


def render(sc, H, W, dev, mode, capacity, out, tag):
    """One forward; returns the capacity it ran with."""
    import torch
    import exavatar_release_amd as exa
    from exavatar_release_amd import rasterizer as rz
    P = len(sc['z'])
    exa.config.mode, exa.config.fixed_capacity, exa.config.keep_debug, exa.config.on_overflow = mode, capacity, True, 'retry'
    with torch.no_grad():
        color = rz.rasterize_gaussians_batch([_job(sc, H, W, dev, False)])[0][0]
        torch.cuda.synchronize()
        rg, ids, cap = _lists(P, H, W)
        out[tag + '__records'] = rz._debug_last['geom'][:P * 64].cpu().numpy().view(np.uint32).reshape(P, 16).copy()
        out[tag + '__ranges'], out[tag + '__ids'], out[tag + '__capacity'] = rg, ids, np.int64(cap)
        out[tag + '__image'] = color.cpu().numpy()
    return cap


def main(path):
    import torch
    dev = torch.device('cuda:0')
    out = {}
    for name, ((H, W), sc, _) in CASES.items():
        need = render(sc, H, W, dev, 'exact', None, out, name + '__exact')
        render(sc, H, W, dev, 'capacity', need + 128, out, name + '__capacity')
    np.savez(path, **out)


if __name__ == '__main__':
    main(sys.argv[1])
