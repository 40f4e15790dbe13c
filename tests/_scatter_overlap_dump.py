"""Helper of test_gpu_scatter_overlap.py (run as a subprocess so that the library reads EXA_BIN_SINGLE_CELLS afresh): renders
every case of CASES -- the places where the ORDER of cell_scatter_kernel's phases can break (rows requested for threads past
P, barriers under the early returns, the publisher's place in the grid, the zero-fill on every way out) and that the cases of
_binning_dump.py do not reach -- in exact mode and in capacity mode (scans merged into the scatter; forward + backward), and
saves the sub-tile ranges, the sorted ids of every list, the images and the gradients.

Scenes, jobs and the render are those of _binning_dump.py (splats in pixels under a pinhole camera looking down +z)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _binning_dump import splats, render                                     # noqa: E402
import exavatar_release_amd as exa                                          # noqa: E402
from exavatar_release_amd import rasterizer as rz                            # noqa: E402

FAINT = 1.0 / 512.0            # below the 1/255 every pixel test needs: such a splat has no instance anywhere


def _scatter(P, H, W, rng, seed):
    return splats(W * rng.rand(P), H * rng.rand(P), 0.8 + 3.0 * rng.rand(P), seed=seed)


def _cases():
    rng = np.random.RandomState(11)
    c = {}
    # one partly filled wave: 15 waves hold no Gaussian, reach every barrier and request no row past P
    c['p1'] = ((128, 128), [splats([70.0], [60.0], 3.0)])
    c['p63'] = ((128, 128), [_scatter(63, 128, 128, rng, 1)])
    # exactly one full chunk: the publisher is workgroup 1
    c['p1024'] = ((128, 128), [_scatter(1024, 128, 128, rng, 2)])
    # a last chunk of one
    c['p2049'] = ((128, 128), [_scatter(2049, 128, 128, rng, 3)])
    # three cells (the walk's odd-cell branch) with three chunks
    c['p3000_three_cells'] = ((64, 192), [_scatter(3000, 64, 192, rng, 4)])
    # everything behind the camera: no entry anywhere
    behind = _scatter(2000, 128, 128, rng, 5)
    behind['z'] = -behind['z']
    c['all_culled'] = ((128, 128), [behind])
    # every second Gaussian without instances, next to live ones in every wave
    faint = _scatter(2000, 128, 128, rng, 6)
    faint['opacity'][1::2] = FAINT
    c['faint_interleaved'] = ((128, 128), [faint])
    # two jobs in one call: the workgroups past job 0's chunk and publisher leave before any barrier, job 1 runs all of them
    c['batch_1_and_3000'] = ((128, 128), [splats([40.0], [90.0], 2.0), _scatter(3000, 128, 128, rng, 7)])
    return c


CASES = _cases()
OVERFLOW_CASE = 'p2049'                        # also rendered into a buffer of 64 instances: overflow, then the repair


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
