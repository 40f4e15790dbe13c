"""Generates tests/golden/ref_densify.npz by EXECUTING the reference's own densification.

``SceneGaussian.densify_and_prune`` with ``clone_points``, ``split_points``, ``densify`` and ``prune_points``, and the
optimizer surgery ``cat_params_to_optimizer`` / ``prune_params_from_optimizer``
(/root/reference/avatar/common/nets/module.py:17-56,159-245) are the code ``exavatar_release_amd.SceneGaussian`` replaces.
The file cannot be imported here (pytorch3d, the training config), so the functions are cut out of it with ``ast`` and
exec'd UNCHANGED -- as ``make_golden_scene.py`` does -- on the CPU in float32, in a namespace that holds what they use:
``nn``, ``rotation_6d_to_matrix`` from ``p3d_standins``, a stub for ``cfg``, and a ``torch`` whose ``normal`` is fed from
the recorded noise (``noise * std + mean``, what ``torch.normal`` computes from its own draws); ``Tensor.cuda`` is the
identity while they run.  Nothing of the reference's text is written anywhere: only inputs and outputs travel.

The case (``build_case``) is built so that every row keeps a margin from every threshold (asserted by
tests/test_densify_oracle.py) and all four classes occur; the arrays that are only ever copied (the SH coefficients and the
Adam moments) hold multiples of 1/64, which keeps the file small and loses nothing: a copy is compared bit for bit.
Run from the repo root:  python tests/golden/make_golden_densify.py
"""
import ast
import os
import sys
import textwrap
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))
REF_MODULE = '/root/reference/avatar/common/nets/module.py'

PARAMS = ('mean', 'feature_dc', 'feature_rest', 'opacity', 'scale', 'rotation')      # the reference's group order
HYPER = dict(densify_grad_thr=0.0002, opacity_min=0.005, dense_percent_thr=0.01)     # avatar/main/config.py:13-31
SCREEN = 20                                                                          # avatar/main/model.py:288-289
P0 = 701
EXTENT = 5.0


def build_case(P=P0, seed=5):
    """Inputs of one densification, float32 numpy: parameters, statistics, Adam moments and the noise for every split
    candidate.  Max scales sit well inside the five bands the thresholds cut (0.01 and 0.1 of the extent, and 0.8 x 0.1 of
    it for the children), opacities well off ``opacity_min``, mean gradients well off the threshold."""
    rng = np.random.RandomState(seed)
    f = lambda x: np.asarray(x, np.float32)      # noqa: E731
    bands = [(0.01, 0.04), (0.06, 0.45), (0.55, 0.75), (0.9, 2.0)]          # of max exp(scale), extent = 5
    band = rng.randint(0, 4, P)
    band[:300] = rng.randint(0, 2, 300)          # a long stretch without wide rows
    top = np.array([rng.uniform(*bands[b]) for b in band])
    frac = rng.uniform(0.05, 1.0, (P, 3))
    frac[np.arange(P), rng.randint(0, 3, P)] = 1.0
    scale = f(np.log(top[:, None] * frac))
    opacity = f(np.where(rng.rand(P) < 0.15, rng.uniform(-8.0, -6.0, P), rng.uniform(-4.0, 5.0, P)))[:, None]
    cnt = f(rng.randint(0, 6, P))
    hot = rng.rand(P) < 0.5
    accum = f(np.where(hot, rng.uniform(0.0003, 0.01, P), rng.uniform(0.0, 0.00015, P)) * np.maximum(cnt, 1))
    accum[cnt == 0] = np.where(rng.rand(int((cnt == 0).sum())) < 0.5, 0.0, accum[cnt == 0])     # 0 / 0 and x / 0
    rotation = f(rng.randn(P, 6))
    rotation[:3] = f([[1, 0, 0, 0, 1, 0], [0, 1, 0, 0, 0, 1], [1, 0, 0, 2, 0.5, 0]])
    coarse = lambda *s: f(rng.choice(np.r_[-127:0, 1:128], s) / 64.0)      # noqa: E731  (never zero)
    case = {'mean': f(2.0 * rng.randn(P, 3)), 'scale': scale, 'rotation': rotation, 'opacity': opacity,
            'feature_dc': coarse(P, 1, 3), 'feature_rest': coarse(P, 15, 3),
            'xyz_grad_accum': accum[:, None], 'track_cnt': cnt[:, None], 'radius_max': f(rng.randint(0, 41, P)),
            'cam_dist_radius': f([EXTENT]), 'step': f(7.0)}
    for k in PARAMS:
        case['exp_avg_' + k] = coarse(*case[k].shape)
        case['exp_avg_sq_' + k] = np.abs(coarse(*case[k].shape))
    case['noise'] = f(rng.randn(2 * P, 3))       # more rows than any number of candidates needs; the first 2 n_cand are used
    return case


def _cut(path, functions, cls=None):
    src = open(path).read()
    lines = src.splitlines()
    tree = ast.parse(src)
    body = tree.body
    if cls is not None:
        body = [n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == cls][0].body
    found = {f.name: textwrap.dedent('\n'.join(lines[f.lineno - 1: f.end_lineno]))
             for f in body if isinstance(f, ast.FunctionDef) and f.name in functions}
    if sorted(found) != sorted(functions):
        raise RuntimeError('%s were not all found in %s' % (functions, path))
    return found


class _Torch:
    """``torch`` with ``normal`` fed from recorded noise."""

    def __init__(self, noise):
        self._noise = noise

    def normal(self, mean, std):
        self.used = std.shape[0]
        z = torch.from_numpy(self._noise[:std.shape[0]].copy())
        return z * std + mean

    def __getattr__(self, name):
        return getattr(torch, name)


def run_reference(case, screen_size_max, hyper=HYPER):
    """The reference's densify_and_prune on ``case`` with a ``torch.optim.Adam`` that holds the case's moments; returns
    the outputs as float32 numpy."""
    from exavatar_release_amd import p3d_standins
    methods = ['densify_and_prune', 'clone_points', 'split_points', 'densify', 'prune_points']
    ns = {'torch': _Torch(case['noise']), 'nn': nn, 'cfg': types.SimpleNamespace(**hyper),
          'rotation_6d_to_matrix': p3d_standins.rotation_6d_to_matrix}
    free = _cut(REF_MODULE, ['cat_params_to_optimizer', 'prune_params_from_optimizer'])
    exec('\n\n'.join(free.values()), ns)
    cut = _cut(REF_MODULE, methods, cls='SceneGaussian')
    for m in methods:
        exec(cut[m], ns)
    Scene = type('SceneGaussian', (nn.Module,), {m: ns[m] for m in methods})
    scene = Scene()
    t = lambda k: torch.from_numpy(case[k].copy())      # noqa: E731
    for k in PARAMS:
        setattr(scene, k, nn.Parameter(t(k)))
    P = case['mean'].shape[0]
    scene.register_buffer('point_num', torch.LongTensor([P]))
    for k in ('radius_max', 'xyz_grad_accum', 'track_cnt', 'cam_dist_radius'):
        scene.register_buffer(k, t(k))
    opt = torch.optim.Adam([{'params': [getattr(scene, k)], 'name': k + '_scene', 'lr': 0.0} for k in PARAMS], lr=0.0, eps=1e-15)
    for k in PARAMS:
        opt.state[getattr(scene, k)] = {'step': torch.tensor(float(case['step'])), 'exp_avg': t('exp_avg_' + k),
                                        'exp_avg_sq': t('exp_avg_sq_' + k)}
    saved = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        with torch.no_grad():
            scene.densify_and_prune(screen_size_max, opt)
    finally:
        torch.Tensor.cuda = saved
    out = {}
    for group in opt.param_groups:
        k = group['name'][:-len('_scene')]
        p = group['params'][0]
        assert p is getattr(scene, k)
        out[k] = p.detach().numpy().copy()
        out['exp_avg_' + k] = opt.state[p]['exp_avg'].numpy().copy()
        out['exp_avg_sq_' + k] = opt.state[p]['exp_avg_sq'].numpy().copy()
        assert float(opt.state[p]['step']) == float(case['step'])
    out['point_num'] = scene.point_num.numpy().copy()
    for k in ('radius_max', 'xyz_grad_accum', 'track_cnt'):
        out[k] = getattr(scene, k).numpy().copy()
    out['n_noise'] = np.int64(ns['torch'].used)
    return out


def main():
    case = build_case()
    data = {'in_' + k: v for k, v in case.items()}
    for tag, ssm in (('none', None), ('s20', SCREEN)):
        data.update({'%s_%s' % (tag, k): v for k, v in run_reference(case, ssm).items()})
        print(tag, 'point_num', data[tag + '_point_num'])
    assert data['none_n_noise'] == data['s20_n_noise']
    data['in_noise'] = case['noise'][:int(data.pop('none_n_noise'))]      # the rows that were drawn: [2 * n_cand, 3]
    del data['s20_n_noise']
    path = os.path.join(HERE, 'ref_densify.npz')
    np.savez_compressed(path, **data)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
