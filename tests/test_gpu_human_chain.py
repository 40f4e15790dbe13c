"""The composed forward: eight HIP modules in ONE autograd graph against the reference's own ``HumanGaussian.forward``.

Every module has its own oracle, fixture and GPU test, fed by hand-made leaves.  Here ``tests/human_case.wire_hip`` wires
them exactly as INTEGRATION.md section 5 prescribes -- ``rot`` of ``joint_transforms`` into the 6D pose row and the
486-wide pose feature, the pose row folded into a bias, ``mean_offset_offset`` through ``pose_offsets`` and back as a
pair, the knn ``idx`` through the in-place hand / face overwrite into ``skin_points``, two point sets under one vertex
transform -- and the results are compared with ``tests/golden/ref_human.npz``: what the reference's forward, exec'd
unchanged in float64 by ``tests/golden/make_golden_human.py``, returns for the same inputs, with autograd's gradients.

The tolerance is not a number chosen here.  The fixture records, per tensor, the error of the reference's OWN float32
run against its float64 run (relative L2 and norm-scaled max, over the stored entries).  The HIP run is another float32
evaluation of the same expression in another summation order, so it may be off by a small multiple of one realisation of
that rounding noise: at most ``FACTOR`` = 4 times the recorded figure, floored at 2^-24 of the tensor's norm for what the
float32 run got exactly.  A wiring error moves a tensor by 1e-3 or more against a noise of ~1e-6.  Three kinds of tensor
get a scale derived from the modules' stated summation orders (``recorded``, ``head_allowance`` and ``trans_allowance``
below; DESIGN.md section 8j has the derivations and the measured ratios).  Whether a gradient passes
a ReLU whose input is within float32 noise of 0 is not a fact two evaluations share: the rows where that happens in the
float64 reference get zero cotangents (``human_case.cotangents``), on both sides."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import rasterizer
from tests import helpers
from tests import human_case as hc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 4.0
FLOOR = 2.0 ** -24


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'ref_human.npz'))


@pytest.fixture(scope='module')
def model():
    return hc.HipHuman(hc.build_case(), DEV)


def cotangents(golden, variant='full'):
    G = hc.cotangents(variant, golden['relu/ambiguous_rows'])
    return {n: torch.from_numpy(np.array(g)).to(DEV) for n, g in G.items()}


def run_chain(golden, m, is_world_coord, variant='full'):
    """One forward + backward of the wired graph: (outputs name -> tensor, the three dicts, nn_vertex_idxs, gradients
    leaf -> tensor or None)."""
    assets, refined, offsets = hc.wire_hip(m, is_world_coord)
    outs = hc.flat_outputs(assets, refined, offsets)
    G = cotangents(golden, variant)
    grads = torch.autograd.grad([outs[n] for n in G], list(m.leaves.values()), list(G.values()), allow_unused=True)
    return outs, (assets, refined, offsets), m.nn_vertex_idxs, dict(zip(m.leaves, grads))


@pytest.fixture(scope='module')
def full_runs(golden, model):
    """The two cases of the fixture, run once and shared: is_world_coord -> run_chain's result."""
    return {wc: run_chain(golden, model, wc) for wc in (False, True)}


def recorded(golden, key):
    """(rel_l2, rel_max) of the reference's own float32 run for one stored tensor, floored at 2^-24.  The gradient of a
    head's bias (1 or 3 entries) is ``sum over rows of t_i``, the same sum as every entry ``sum of t_i a_ik`` of that
    head's weight gradient with ``a_ik := 1``: one or three draws of that noise are no scale (a single draw can be
    arbitrarily near 0), so it takes the weight gradient's figures where they are larger."""
    l2, mx = float(golden[key + '#rel_l2']), float(golden[key + '#rel_max'])
    if key.endswith('.bias') and golden[key].size <= 3:
        w = key[:-len('bias')] + 'weight'
        l2, mx = max(l2, float(golden[w + '#rel_l2'])), max(mx, float(golden[w + '#rel_max']))
    return max(l2, FLOOR), max(mx, FLOOR)


def head_allowance(key):
    """Relative error the HIP head of ``scale_net`` adds to ``scale = exp(x)``, beyond the reference's noise.
    ``include/exa_mlp.h``: a head is ``acc = fma(Wh[o][k], a_k, acc)`` over 128 terms FROM ``acc = bh[o]``, where the
    reference rounds ``Wh a`` on its own and adds the bias once.  With ``|bh| = 4`` against ``|Wh a| ~ 0.05`` every one of
    the 128 partial sums is rounded at the bias's magnitude: 128 independent errors of at most ``2^-24 |bh|`` each,
    ``sqrt(128 / 3) 2^-24 |bh|`` in the root mean square, against the reference's single one; and ``d exp(x) = exp(x)
    dx`` makes an absolute error of x a relative error of scale.  Zero for every other tensor."""
    if not key.endswith(('/out/assets/scale', '/out/assets_refined/scale')):
        return 0.0
    bh = float(np.abs(hc.build_case()['scale_net.0.bias']).max())
    return (128 / 3.0) ** 0.5 * FLOOR * bh


def trans_allowance(golden, key):
    """Error, relative to the norm, that the skinning's stated order adds to ``grad trans`` [3] beyond the reference's
    noise.  ``include/exa_skin.h``: ``grad_trans[r] = sum over v of G_v[r][3]`` with ``G_v[r][3]`` the sum over the sets
    of ``(Rinv^T g_s[v])_r``, chunks of 256 vertices summed sequentially from +0, then the chunk partials sequentially.
    Every addition rounds its result s by at most ``2^-24 |s|``; the V + 11 roundings are independent, so the error of
    component r is ``2^-24 sqrt(sum of s^2)`` over the partial sums of that order.  The terms are the test's own
    cotangents, so the partial sums are evaluated here in float64 (PyTorch reduces pairwise: its own float32 figure for
    these three numbers, 1e-7, says nothing about a sequential sum of 2562 terms of either sign)."""
    if not key.endswith('/grad/trans'):
        return 0.0
    tag = key.split('/')[0]
    G = hc.cotangents('single' if tag.endswith('_single') else 'full', golden['relu/ambiguous_rows'])
    t = sum(G[n].astype(np.float64) for n in G if n.endswith('/mean_3d'))
    if tag.startswith('wc0'):
        t = t @ np.linalg.inv(hc.build_case()['cam_R'].astype(np.float64))          # g' = Rinv^T g
    chunks = [t[i:i + 256] for i in range(0, len(t), 256)]
    inner = np.concatenate([np.cumsum(c, 0) for c in chunks])
    outer = np.cumsum(np.stack([c.sum(0) for c in chunks]), 0)
    err = FLOOR * np.sqrt((inner ** 2).sum(0) + (outer ** 2).sum(0))
    return float(np.linalg.norm(err) / np.linalg.norm(golden[key]))


def ratio(golden, key, got):
    """(HIP error) / (the scale of one stored tensor): the larger of the L2 and the max figure."""
    ref = golden[key]
    got = hc.take_sample(key, got.detach().cpu().double().numpy())
    assert got.shape == ref.shape, (key, got.shape, ref.shape)
    e = got - ref
    norm, n = float(np.linalg.norm(ref)), ref.size
    if norm == 0.0:
        return 0.0 if not e.any() else float('inf')
    rel_l2, rel_max = recorded(golden, key)
    extra = (head_allowance(key) + trans_allowance(golden, key)) / FACTOR      # (an allowance is not multiplied by FACTOR)
    l2 = float(np.linalg.norm(e)) / ((rel_l2 + extra) * norm)
    mx = float(np.abs(e).max()) / ((rel_max + 4 * extra) * norm / np.sqrt(n))      # 4 sigma for the largest of n errors
    return max(l2, mx)


def all_ratios(golden, tag, outs, grads):
    """name -> ratio for every tensor the fixture stores under ``tag``; a leaf the fixture reaches must be reached."""
    res = {}
    if outs is not None:
        for n in hc.OUTPUTS:
            res['out/' + n] = ratio(golden, '%s/out/%s' % (tag, n), outs[n])
    unreached = set(str(s) for s in golden[tag + '/unreached']) - {''}
    for k, g in grads.items():
        if k in unreached:
            assert g is None or not bool(g.any()), 'leaf %s cannot be reached and has a gradient' % k
            continue
        assert g is not None, 'leaf %s got no gradient' % k
        res['grad/' + k] = ratio(golden, '%s/grad/%s' % (tag, k), g)
    return res


def check_ratios(tag, res):
    worst = sorted(res.items(), key=lambda kv: -kv[1])
    for k, r in worst:
        print('%s %-46s ratio %.3f' % (tag, k, r))
    helpers.record_stats('human_chain/' + tag, {'max_ratio': worst[0][1], 'at': worst[0][0], 'ratios': res})
    bad = [(k, round(r, 2)) for k, r in worst if not r <= FACTOR]
    assert not bad, '%s: HIP error above %g x the reference\'s own float32 error: %s' % (tag, FACTOR, bad)


def bits_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


@pytest.mark.parametrize('is_world_coord', [False, True])
def test_values_and_gradients_match_the_reference_forward(golden, full_runs, is_world_coord):
    tag = 'wc%d' % int(is_world_coord)
    outs, (assets, refined, offsets), idx, grads = full_runs[is_world_coord]
    assert tuple(assets) == hc.ASSET_KEYS and tuple(refined) == hc.ASSET_KEYS and tuple(offsets) == hc.OFFSET_KEYS
    V = hc.V
    shapes = {'mean_3d': (V, 3), 'opacity': (V, 1), 'scale': (V, 3), 'rotation': (V, 4), 'rgb': (V, 3),
              'mean_offset': (V, 3), 'mean_offset_offset': (V, 3), 'scale_offset': (V, 1), 'rgb_offset': (V, 3)}
    for d in (assets, refined, offsets):
        for k, v in d.items():
            assert tuple(v.shape) == shapes[k] and v.dtype == torch.float32, k
    assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), golden['nn_vertex_idxs'])
    for d in (assets, refined):
        assert np.array_equal(d['opacity'].cpu().numpy(), golden['opacity'])
        assert np.array_equal(d['rotation'].cpu().numpy(), golden['rotation'])
        s = d['scale']
        assert bits_equal(s[:, 0], s[:, 1]) and bits_equal(s[:, 0], s[:, 2])
    check_ratios(tag, all_ratios(golden, tag, outs, grads))


def test_the_composed_graph_gives_the_same_bits_twice(golden, model, full_runs):
    outs, _, idx, grads = full_runs[False]
    outs2, _, idx2, grads2 = run_chain(golden, model, False)
    assert torch.equal(idx, idx2)
    assert [n for n in outs if not bits_equal(outs[n], outs2[n])] == []
    assert [k for k in grads if not bits_equal(grads[k], grads2[k])] == []


def test_absent_cotangents(golden, model):
    """A cotangent for ``assets_refined['mean_3d']`` alone: every other output's gradient is absent (kinematics' missing
    cotangent travels as None, the MLP heads and the second point set get none)."""
    _, _, _, grads = run_chain(golden, model, False, 'single')
    check_ratios('wc0_single', all_ratios(golden, 'wc0_single', None, grads))


def _render_loss(m, assets, refined):
    r = exa.GaussianRenderer()
    rs = np.random.RandomState(31)
    loss = 0
    for a in (assets, refined):
        G = torch.from_numpy(rs.randn(3, *hc.IMG_SHAPE).astype(np.float32)).to(DEV)
        loss = loss + (r(a, hc.IMG_SHAPE, m.cam_param)['img'] * G).sum()
    return loss


def test_through_the_renderer(golden, model):
    m = model
    leaves = list(m.leaves.values())
    joined = {}
    for mode in ('auto', 'off'):
        exa.config.compiled_node = mode
        taken = rasterizer.compiled_calls
        assets, refined, _ = hc.wire_hip(m, False)
        joined[mode] = torch.autograd.grad(_render_loss(m, assets, refined), leaves, allow_unused=True)
        # 'auto' must have gone through the compiled node (its backward runs on the engine thread), 'off' must not
        assert rasterizer.compiled_calls - taken == (2 if mode == 'auto' else 0), mode
    names = list(m.leaves)
    assert [k for k, a, b in zip(names, joined['auto'], joined['off']) if not bits_equal(a, b)] == []
    # the same graph split at the assets: the renderer's gradients fed to the wired graph as cotangents
    assets, refined, _ = hc.wire_hip(m, False)
    keys = ('mean_3d', 'scale', 'rgb')
    cut = [{k: (v.detach().requires_grad_(True) if k in keys else v) for k, v in d.items()} for d in (assets, refined)]
    cot = torch.autograd.grad(_render_loss(m, *cut), [d[k] for d in cut for k in keys])
    split = torch.autograd.grad([d[k] for d in (assets, refined) for k in keys], leaves, cot, allow_unused=True)
    res = {}
    for k, gj, gs in zip(names, joined['auto'], split):
        assert gj is not None and gs is not None, k            # the render reaches every leaf the ten cotangents reach
        gj, gs = gj.double().cpu().numpy(), gs.double().cpu().numpy()
        assert np.isfinite(gj).all() and gj.any(), k
        norm, key = float(np.linalg.norm(gj)), 'wc0/grad/' + k
        rel_l2, rel_max = recorded(golden, key)
        l2 = float(np.linalg.norm(gs - gj)) / (rel_l2 * norm)
        mx = float(np.abs(gs - gj).max()) / (rel_max * norm / np.sqrt(gj.size))
        res['grad/' + k] = max(l2, mx)
    check_ratios('render_split_vs_joined', res)


def test_forward_and_backward_replay_from_one_captured_graph():
    """``is_world_coord=True`` (no ``torch.inverse``) with the index overwrite as a ``torch.where``: nothing reads the
    device back, so forward + backward are captured once and replayed with a new pose, expression and triplanes; the
    replay equals an eager run of the new inputs bit for bit (``tests/_human_capture.py``).  Runs in a child process
    under a time limit: a capture that hangs must not take the session with it."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_human_capture.py')], capture_output=True, text=True,
                       timeout=240, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT)
    assert r.returncode == 0 and 'RESULT ok' in r.stdout, 'child: rc %d\n%s\n%s' % (r.returncode, r.stdout[-800:],
                                                                                   r.stderr[-1500:])
