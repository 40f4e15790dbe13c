"""Generates tests/golden/ref_scene.npz by EXECUTING the reference's own scene-Gaussian forward.

``SceneGaussian.forward`` (/root/reference/avatar/common/nets/module.py:253-272) and ``eval_sh`` with its coefficient
tables (/root/reference/avatar/common/utils/transforms.py:82-167) are the code ``exavatar_release_amd.scene_assets``
replaces.  Neither file can be imported here (pytorch3d, the training config), so the two functions and the tables are cut
out of the files with ``ast`` and exec'd UNCHANGED -- as ``make_golden_kinematics.py`` does -- in a namespace that holds
what they use: ``torch``, ``F`` and ``matrix_to_quaternion`` / ``rotation_6d_to_matrix`` from ``p3d_standins`` (the
restatements of pytorch3d's).  Everything runs in float64 on the CPU, with autograd for the gradients.  Nothing of the
reference's text is written anywhere: only inputs and outputs travel.  Run from the repo root:
python tests/golden/make_golden_scene.py
"""
import ast
import os
import sys
import textwrap
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))
REF_MODULE = '/root/reference/avatar/common/nets/module.py'
REF_TRANSFORMS = '/root/reference/avatar/common/utils/transforms.py'

from exavatar_release_amd import p3d_standins      # noqa: E402

# the rows every implementation has to get right: identity, zero, the four-way tie, the three half turns, a2 parallel to
# a1, a first axis below F.normalize's eps
SPECIAL = [(1, 0, 0, 0, 1, 0), (0, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 1), (1, 0, 0, 0, -1, 0), (-1, 0, 0, 0, 1, 0),
           (-1, 0, 0, 0, -1, 0), (1, 0, 0, 2, 0, 0), (1e-20, 0, 0, 0, 1, 0)]
P = 12


def _cut(path, functions=(), tables=(), cls=None):
    """The source of the functions (methods of ``cls`` when given) and module-level assignments named, unchanged."""
    src = open(path).read()
    lines = src.splitlines()
    text = lambda node: textwrap.dedent('\n'.join(lines[node.lineno - 1: node.end_lineno]))      # noqa: E731
    tree = ast.parse(src)
    body = tree.body
    if cls is not None:
        body = [n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == cls][0].body
    found = {f.name: text(f) for f in body if isinstance(f, ast.FunctionDef) and f.name in functions}
    for n in tree.body:
        if isinstance(n, ast.Assign) and len(n.targets) == 1 and getattr(n.targets[0], 'id', None) in tables:
            found[n.targets[0].id] = text(n)
    if sorted(found) != sorted(tuple(functions) + tuple(tables)):
        raise RuntimeError('%s were not all found in %s' % (tuple(functions) + tuple(tables), path))
    return found


def main():
    sh_src = _cut(REF_TRANSFORMS, ['eval_sh'], ['C0', 'C1', 'C2', 'C3', 'C4'])
    fwd_src = _cut(REF_MODULE, ['forward'], cls='SceneGaussian')['forward']
    ns = {'torch': torch, 'F': F, 'matrix_to_quaternion': p3d_standins.matrix_to_quaternion,
          'rotation_6d_to_matrix': p3d_standins.rotation_6d_to_matrix}
    exec('\n\n'.join(sh_src[k] for k in ('C0', 'C1', 'C2', 'C3', 'C4', 'eval_sh')) + '\n\n' + fwd_src, ns)

    g = torch.Generator().manual_seed(31)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    rotation = torch.cat((torch.tensor(SPECIAL, dtype=torch.float64), rnd(P - len(SPECIAL), 6)))
    mean, opacity, scale = 2.0 * rnd(P, 3), 3.0 * rnd(P, 1), rnd(P, 3) - 2.0
    dc, rest = 0.8 * rnd(P, 1, 3), 0.3 * rnd(P, 15, 3)
    dc[2] = -3.0                  # every channel clamped
    dc[5, 0, 1] = -2.5            # one channel clamped
    q, r = torch.linalg.qr(rnd(3, 3))
    R = q * torch.sign(torch.diagonal(r))[None, :]
    t = rnd(3)
    G = {'opacity': rnd(P, 1), 'scale': rnd(P, 3), 'rotation': rnd(P, 4), 'rgb': rnd(P, 3)}
    names = ['mean', 'opacity', 'scale', 'rotation', 'feature_dc', 'feature_rest']
    out = {'mean': mean, 'opacity': opacity, 'scale': scale, 'rotation': rotation, 'feature_dc': dc, 'feature_rest': rest,
           'R': R, 't': t}
    out.update({'G_' + k: v for k, v in G.items()})
    out = {k: v.numpy().copy() for k, v in out.items()}
    for deg in range(4):
        params = [x.clone().requires_grad_(True) for x in (mean, opacity, scale, rotation, dc, rest)]
        self = types.SimpleNamespace(**dict(zip(names, params)), active_sh_degree=deg)
        assets = ns['forward'](self, {'R': R, 't': t})
        assert assets['mean_3d'] is params[0]
        keys = ['opacity', 'scale', 'rotation', 'rgb']
        # degree 0 never reads the view direction: `mean` is then outside the graph and its gradient is zero
        grads = torch.autograd.grad([assets[k] for k in keys], params, [G[k] for k in keys], allow_unused=True)
        for k in keys:
            out['deg%d_%s' % (deg, k)] = assets[k].detach().numpy()
        for n, x, p in zip(names, grads, params):
            out['deg%d_grad_%s' % (deg, n)] = (torch.zeros_like(p) if x is None else x).numpy()
    path = os.path.join(HERE, 'ref_scene.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
