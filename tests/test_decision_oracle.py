"""tests/decision_oracle.py against oracle/raster_oracle.py in float64 (CPU).  Given the decisions raster_oracle takes
itself -- read off its own forward with tests/helpers.py extract_weights, the procedure the GPU test applies to the HIP
forward -- the decision oracle must reproduce its values to 1e-12 and every gradient to 1e-10 on the 16 edge-case fuzz
trials and the needle scene."""
import os

import pytest
import torch

from oracle import raster_oracle as ro
from tests import decision_oracle as do
from tests.decision_oracle import KEYS
from tests.helpers import extract_weights, fuzz_case, needle_scene


def _oracle_weights(a, H, W, cam, perm=None):
    """w [P, H, W] of the float64 raster_oracle forward, by one-hot colour probes."""
    def render_rgb(rgb):
        with torch.no_grad():
            return ro.render({**a, 'rgb': rgb}, (H, W), cam, torch.zeros(3), dtype=torch.float64)['img']
    return extract_weights(render_rgb, a['mean_3d'].shape[0], perm)


def _check(a, H, W, cam, bg, G, Gd, Ga):
    P = a['mean_3d'].shape[0]
    t = {k: v.clone().double().requires_grad_(True) for k, v in a.items()}
    r = ro.render(t, (H, W), cam, bg, dtype=torch.float64)
    ((r['img'] * G.double()).sum() + (r['depthmap'] * Gd.double()).sum() + (r['mask'] * Ga.double()).sum()).backward()
    w = _oracle_weights(a, H, W, cam)
    keep = w > 0
    # the probe: weights add up to the coverage, and another grouping of the probes reads the same decisions
    assert float((w.sum(0) - r['mask'].detach()[0]).abs().max()) <= 1e-6
    w2 = _oracle_weights(a, H, W, cam, torch.randperm(P, generator=torch.Generator().manual_seed(P)))
    assert torch.equal(w2 > 0, keep)
    vis = r['radius'] > 0
    with torch.no_grad():       # float64 oracle's own order: float64 depth, ties by index
        d = ro.preprocess(t['mean_3d'].detach(), None, None, t['scale'].detach(), t['rotation'].detach(), None,
                          ro.settings_from_camera(cam, (H, W), bg), torch.float64)['depth']
    idx = torch.nonzero(vis).flatten()
    order = idx[torch.argsort(d[idx], stable=True)]
    u = {k: v.clone().double().requires_grad_(True) for k, v in a.items()}
    o = do.render(u, (H, W), cam, bg, keep, vis, order=order)
    ((o['img'] * G.double()).sum() + (o['depthmap'] * Gd.double()).sum() + (o['mask'] * Ga.double()).sum()).backward()
    for k in ('img', 'depthmap', 'mask'):
        assert float((o[k].detach() - r[k].detach()).abs().max()) <= 1e-12, k
    assert float((o['w'] - w).abs().max()) <= 1e-12
    for k in KEYS + ('mean_2d',):
        got = u[k].grad if k != 'mean_2d' else o['mean_2d'].grad
        ref = t[k].grad if k != 'mean_2d' else r['mean_2d'].grad
        err = float((got - ref).abs().max())
        assert err <= 1e-10 * max(1.0, float(ref.abs().max())), 'grad %s off by %.3e' % (k, err)
    return keep


@pytest.mark.parametrize('trial', range(int(os.environ.get('EXA_FUZZ_TRIALS', '16'))))
def test_decision_oracle_equals_raster_oracle_on_the_fuzz(trial):
    a, H, W, cam, G, Gd, Ga, bg = fuzz_case(trial)
    _check(a, H, W, cam, bg, G, Gd, Ga)


def test_decision_oracle_equals_raster_oracle_on_needles():
    a, H, W, cam, bg, G = needle_scene()
    g = torch.Generator().manual_seed(78)
    keep = _check(a, H, W, cam, bg, G, torch.randn(1, H, W, generator=g), torch.randn(1, H, W, generator=g))
    assert int(keep[:4].flatten(1).any(1).sum()) >= 3          # the needles are blended


def test_decisions_are_inputs_not_derived():
    """Dropping one kept pair changes exactly that pixel: the module follows ``keep`` and takes no decision of its own."""
    a, H, W, cam, bg, G = needle_scene()
    w = _oracle_weights(a, H, W, cam)
    keep = w > 0
    vis = ro.render(a, (H, W), cam, bg)['radius'] > 0
    i, y, x = [int(v) for v in torch.nonzero(keep)[len(torch.nonzero(keep)) // 2]]
    k2 = keep.clone()
    k2[i, y, x] = False
    with torch.no_grad():
        o1 = do.render(a, (H, W), cam, bg, keep, vis)
        o2 = do.render(a, (H, W), cam, bg, k2, vis)
    d = (o1['mask'] - o2['mask']).abs()[0]
    assert float(d[y, x]) > 0 and int((d > 0).sum()) == 1
    assert float(o2['w'][i, y, x]) == 0.0
