"""CPU check of the triplane backward's plan (exavatar_release_amd.triplane.plan_tables): built from step-1 keys computed
here, its tables drive a numpy emulation of the kernel's two passes (segment partials, then the partials of each texel
in order), which must equal the oracle's two-level backward bit for bit -- so the plan cuts the lists exactly where the
header and tests/triplane_oracle.py say it does, and every gradient element is written once."""
import numpy as np
import pytest
import torch

from exavatar_release_amd import triplane as tp
from tests import triplane_oracle as to


def _keys(coords, is_face, H, W):
    """Step 1 of the plan: key of entry e = (i * 3 + k) * 4 + t."""
    N, HW = coords.shape[0], H * W
    T = 6 * HW
    keys = np.empty((N, 3, 4), dtype=np.int64)
    for k in range(3):
        for t, (yx, _) in enumerate(to._taps(coords, k, H, W, np.float32)):
            keys[:, k, t] = np.where(yx >= 0, is_face * 3 * HW + k * HW + yx, T)
    return keys.reshape(-1).astype(np.int32)


def _emulate_backward(g, coords, C, H, W, tab):
    """The kernel's arithmetic on the plan's tables, operation by operation in float32."""
    HW = H * W
    grads = np.full((2, 3, C, HW), np.nan, dtype=np.float32)       # every element must be overwritten
    entries, seg_entry, tex_seg, wg_tex = (tab[k].numpy() for k in ('entries', 'seg_entry', 'tex_seg', 'wg_tex'))
    weights = {}
    for k in range(3):
        weights[k] = np.stack([w for _, w in to._taps(coords, k, H, W, np.float32)], 1)
    written = np.zeros((2, 3, HW), dtype=np.int64)
    for w in range(tab['num_wg']):
        t0, t1 = wg_tex[w], wg_tex[w + 1]
        s0, s1 = tex_seg[t0], tex_seg[t1]
        assert s1 - s0 <= tab['max_wg_segments']
        part = np.zeros((s1 - s0, C), dtype=np.float32)
        for s in range(s0, s1):
            acc = np.zeros(C, dtype=np.float32)
            for j in range(seg_entry[s], seg_entry[s + 1]):
                e = int(entries[j])
                i, k, t = e // 12, (e % 12) >> 2, e & 3
                acc = acc + g[i, k * C:(k + 1) * C] * weights[k][i, t]
            part[s - s0] = acc
        for tx in range(t0, t1):
            acc = np.zeros(C, dtype=np.float32)
            for s in range(tex_seg[tx], tex_seg[tx + 1]):
                acc = acc + part[s - s0]
            face, tt = divmod(tx, 3 * HW)
            k, yx = divmod(tt, HW)
            grads[face, k, :, yx] = acc
            written[face, k, yx] += 1
    assert np.all(written == 1)
    return grads[0].reshape(3, C, H, W), grads[1].reshape(3, C, H, W)


@pytest.mark.parametrize('C,H,W,N,face_frac', [(4, 3, 5, 700, 0.3), (1, 1, 1, 300, 0.5), (3, 2, 2, 200, 0.0),
                                               (33, 4, 4, 150, 1.0), (1024, 2, 2, 3000, 0.2), (8, 16, 16, 0, 0.0)])
def test_plan_tables_drive_the_oracles_two_level_order(C, H, W, N, face_frac):
    rng = np.random.default_rng(C + N)
    coords = rng.uniform(-1.2, 1.2, size=(N, 3)).astype(np.float32)
    is_face = rng.random(N) < face_frac
    g = rng.standard_normal((N, 3 * C)).astype(np.float32)
    tab = tp.plan_tables(torch.from_numpy(_keys(coords, is_face, H, W)), 6 * H * W, C)
    assert tab['max_wg_segments'] * C * 4 <= tp.MAX_LDS
    gb, gf = _emulate_backward(g, coords, C, H, W, tab)
    ob, of = to.backward(g, coords, is_face, C, H, W, seg_len=tab['seg_len'])
    assert np.array_equal(gb.view(np.uint32), ob.view(np.uint32))
    assert np.array_equal(gf.view(np.uint32), of.view(np.uint32))
    lens = to.list_lengths(coords, is_face, H, W).reshape(-1)
    assert np.array_equal(tab['list_lengths'].numpy(), lens)
    if C == 1024:
        assert tab['seg_len'] > 32, 'the longest list must have forced a longer segment'
