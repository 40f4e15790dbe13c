"""Mask-ready entries (csrc/binning.hip): on the multi-part path with the footprint test on, cell_scatter_kernel<true> computes
the footprint masks itself -- entry-parallel, from rows staged in LDS -- and subtile_count_kernel only counts their bits.

Reference: the unchanged one-workgroup-per-cell path of the same library (cell_scatter_kernel<false> writes rects,
subtile_count_bin_kernel gathers the rows and computes the masks), forced by EXA_BIN_SINGLE_CELLS=1 in a fresh child process,
as test_one_workgroup_per_cell_binning_gives_the_same_lists does.  Both processes render every case of tests/_binning_dump.py
in exact mode (scans in their own launches) and in capacity mode (scans merged into the scatter; with a backward).  Required:
identical sub-tile ranges, identical sorted ids per list, bit-identical images and gradients."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

CASE_NAMES = ('one_subtile', 'four_cell_corner', 'second_chunk_of_one', 'border_72x40', 'border_136x40', 'crowded_cell',
              'corner_crowd', 'whole_image', 'needles', 'batch_of_two', 'batch_of_two_swapped')


@pytest.fixture(scope='module')
def dumps(tmp_path_factory):
    """(reference, default path): every case rendered once per process, shared by all tests, never modified."""
    d = tmp_path_factory.mktemp('binning_masks')
    outs = []
    for name, env in (('single', {'EXA_BIN_SINGLE_CELLS': '1'}), ('parts', {})):
        path = str(d / (name + '.npz'))
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_binning_dump.py'), path], cwd=ROOT,
                           env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(dict(np.load(path)))
    return outs


def test_the_cases_are_the_ones_rendered():
    import _binning_dump
    assert tuple(_binning_dump.CASES) == CASE_NAMES


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
    """The scenes are built in pixels; what each is for is checked on the lists the reference left."""
    single, _ = dumps
    n = lambda case: (single[case + '__exact__ranges'][:, 1].astype(np.int64) - single[case + '__exact__ranges'][:, 0])   # noqa: E731
    assert (n('one_subtile') > 0).sum() == 1 and n('one_subtile').sum() == 1
    corner = n('four_cell_corner').reshape(4, 64)
    assert ((corner > 0).sum(1) > 0).all() and corner.sum() >= 4                   # all four cells of the 128 x 128 image
    assert len(single['second_chunk_of_one__exact__job0_radii']) == 1025
    assert len(n('border_72x40')) == 2 * 64 and len(n('border_136x40')) == 3 * 64   # 2 and 3 cells, padding sub-tiles included
    crowd = n('crowded_cell').reshape(4, 64).sum(1)
    assert crowd[1] >= 5000 and crowd[[0, 2, 3]].sum() == 0                        # one cell, > 4 096 entries: five parts
    assert (n('corner_crowd').reshape(4, 64).sum(1) >= 600).all()                  # >= 2 400 entries from ONE chunk
    assert (n('whole_image') > 0).all() and len(n('whole_image')) == 16 * 64       # 16 cells from one Gaussian
    assert (single['needles__exact__job0_radii'] > 0).all()


def test_overflowed_render_is_repaired_to_the_same_lists(dumps):
    """A buffer of 64 instances: every cell of the overflowed render publishes empty ranges and nothing is read past the
    bucket array; the repair renders again with room and leaves what a render that fitted leaves."""
    single, parts = dumps
    tag = 'second_chunk_of_one__overflow__'
    for d in (single, parts):
        ev = d[tag + 'events']
        assert len(ev) == 1 and ev[0, 1] == 64 and ev[0, 0] > 64
    for k in sorted(k for k in parts if k.startswith(tag)):
        assert np.array_equal(single[k], parts[k]), k
        fit = k.replace('__overflow__', '__capacity__')
        if fit in parts and not k.endswith('events'):
            assert np.array_equal(parts[k], parts[fit]), k
