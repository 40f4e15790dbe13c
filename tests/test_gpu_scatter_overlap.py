"""The order of cell_scatter_kernel's phases (csrc/binning.hip): where the splat rows are requested, where the zero-fill is
issued, which scans share a pair of barriers.  None of it may change a list, an image or a gradient.

Reference, as in test_gpu_binning_masks.py: the one-workgroup-per-cell path of the same library (cell_scatter_kernel<false>
writes rects, subtile_count_bin_kernel gathers the rows and computes the masks), forced by EXA_BIN_SINGLE_CELLS=1 in a fresh
child process.  Both processes render every case of tests/_scatter_overlap_dump.py in exact mode (scans in their own launches)
and in capacity mode (scans merged into the scatter; with a backward).  Required: identical sub-tile ranges, identical sorted
ids per list, bit-identical images and gradients.

The cases are the places a reordering can break that the eleven of _binning_dump.py do not reach: workgroups whose waves
hold no Gaussian (P = 1, 63), the publisher right behind one full chunk (P = 1024), a last chunk of one (P = 2049), the walk's
odd-cell branch over several chunks, a job without any entry, Gaussians without instances next to live ones in one wave,
a batch whose first job leaves most of the grid idle, and the overflow return behind the last barrier."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

CASE_NAMES = ('p1', 'p63', 'p1024', 'p2049', 'p3000_three_cells', 'all_culled', 'faint_interleaved', 'batch_1_and_3000')
CHUNK = 1024                                                    # Gaussians per scatter workgroup (csrc/common.h)


@pytest.fixture(scope='module')
def dumps(tmp_path_factory):
    """(reference, default path): every case rendered once per process, shared by all tests, never modified."""
    d = tmp_path_factory.mktemp('scatter_overlap')
    outs = []
    for name, env in (('single', {'EXA_BIN_SINGLE_CELLS': '1'}), ('parts', {})):
        path = str(d / (name + '.npz'))
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_scatter_overlap_dump.py'), path], cwd=ROOT,
                           env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(dict(np.load(path)))
    return outs


def test_the_cases_are_the_ones_rendered():
    import _scatter_overlap_dump
    assert tuple(_scatter_overlap_dump.CASES) == CASE_NAMES
    assert _scatter_overlap_dump.OVERFLOW_CASE == 'p2049'


@pytest.mark.parametrize('mode', ['exact', 'capacity'])
@pytest.mark.parametrize('case', CASE_NAMES)
def test_lists_images_and_gradients_equal_the_single_part_path(dumps, case, mode):
    single, parts = dumps
    tag = '%s__%s__' % (case, mode)
    keys = sorted(k for k in parts if k.startswith(tag))
    assert keys == sorted(k for k in single if k.startswith(tag))
    assert any('grad_' in k for k in keys) == (mode == 'capacity')
    for k in [tag + 'ranges', tag + 'ids'] + keys:                # lists first: a wrong list explains a wrong image
        assert single[k].shape == parts[k].shape and np.array_equal(single[k].view(np.uint8), parts[k].view(np.uint8)), k


def test_the_cases_reach_what_they_are_for(dumps):
    """Chunk counts, cell counts, Gaussians without instances, empty lists -- read from what the reference left."""
    single, _ = dumps
    P = lambda case, job=0: len(single['%s__exact__job%d_radii' % (case, job)])                                          # noqa: E731
    n = lambda case: (single[case + '__exact__ranges'][:, 1].astype(np.int64) - single[case + '__exact__ranges'][:, 0])   # noqa: E731
    chunks = lambda p: (p + CHUNK - 1) // CHUNK                                                                           # noqa: E731
    assert P('p1') == 1 and n('p1').sum() >= 1
    assert P('p63') == 63 and chunks(63) == 1 and n('p63').sum() >= 63
    assert P('p1024') == CHUNK and chunks(P('p1024')) == 1                          # one full chunk: the publisher is workgroup 1
    assert P('p2049') == 2 * CHUNK + 1 and chunks(P('p2049')) == 3                  # the last chunk holds one Gaussian ...
    assert single['p2049__exact__job0_radii'][-1] > 0                               # ... and it is visible
    three = n('p3000_three_cells')
    assert len(three) == 3 * 64 and chunks(P('p3000_three_cells')) == 3             # odd number of cells, several chunks
    assert (three.reshape(3, 64).sum(1) > 0).all()
    assert P('all_culled') == 2000 and n('all_culled').sum() == 0                   # no entry anywhere
    assert len(single['all_culled__exact__ids']) == 0 and (single['all_culled__exact__job0_radii'] == 0).all()
    # every second Gaussian has no instance: its id is in no list, while live ones of the same waves are
    listed = np.zeros(P('faint_interleaved'), bool)
    listed[single['faint_interleaved__exact__ids']] = True
    assert P('faint_interleaved') == 2000 and not listed[1::2].any() and listed[0::2].sum() > 900
    # a batch whose first job has one chunk and whose second has three
    assert P('batch_1_and_3000', 0) == 1 and P('batch_1_and_3000', 1) == 3000
    assert single['batch_1_and_3000__exact__job0_radii'][0] > 0 and n('batch_1_and_3000').sum() >= 3000


def test_overflowed_render_is_repaired_to_the_same_lists(dumps):
    """P = 2049 into a buffer of 64 instances: the scattering workgroups leave behind the last barrier every thread reaches,
    their zero-fill done; the repair renders again with room and leaves what a render that fitted leaves."""
    single, parts = dumps
    tag = 'p2049__overflow__'
    for d in (single, parts):
        ev = d[tag + 'events']
        assert len(ev) == 1 and ev[0, 1] == 64 and ev[0, 0] > 64
    for k in sorted(k for k in parts if k.startswith(tag)):
        assert np.array_equal(single[k], parts[k]), k
        fit = k.replace('__overflow__', '__capacity__')
        if fit in parts and not k.endswith('events'):
            assert np.array_equal(parts[k], parts[fit]), k
