"""Generates tests/golden/ref_fit_terms.npz by EXECUTING the reference's own ``EdgeLengthLoss``, ``FaceOffsetSymmetricReg``
and ``PoseLoss``.

``/root/reference/fitting/common/nets/loss.py`` cannot be imported here (it imports pytorch3d, the fitting config and the
``smpl_x`` singleton at the top), so the source text of the three classes is cut out of the file with ``ast`` and exec'd
unchanged in a namespace holding torch / nn / np, a stub ``smpl_x`` (``vertex_num``, ``face_vertex_idx``, ``flip_corr``,
``joint``) and ``axis_angle_to_matrix`` from ``exavatar_release_amd.p3d_standins``.  pytorch3d is not installed, so
``PoseLoss`` is pinned ONLY by that stand-in (a restatement of pytorch3d's quaternion route in torch, itself tested in
tests/test_standins.py); the other two classes are the reference's own arithmetic.  ``Tensor.cuda()`` returns a copy for the
duration (this container has no GPU).  The float64 run is the same source on the same numbers with ``Tensor.float()``
widened to ``.double()`` and ``torch.FloatTensor`` to a float64 constructor.  The centred vertex-to-vertex term is the
expression of ``fitting/main/model.py:235-237`` evaluated by torch on the same numbers (restated below: it is one line of
a method that cannot be cut out).  Gradients are autograd's for a recorded random cotangent.
Run from the repo root:  python tests/golden/make_golden_fit.py
Nothing here is read at test time on the GPU box -- only the .npz travels.

Sizes: V_full = 60, Vf = 25, F = 40, B = 2, J = 7.  The seeds are searched so that NO sign decision (``d_out - d_gt``, each
symmetry term, each entry of ``R_out - R_gt``, each ``e``) lies within 1e-5 relative of zero in the float64 run, the
planted exact ties aside (asserted below; the tests' bar is a share of at most 1 %): one edge with ``out == gt`` at both
ends, one zero offset row whose taps read zeros, one pose row with ``out == gt``.
"""
import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from exavatar_release_amd import p3d_standins      # noqa: E402
from tests import fit_oracle as fo                 # noqa: E402

REF = '/root/reference/fitting/common/nets/loss.py'
V_FULL, VF, NF, B, J = 60, 25, 40, 2, 7
src = open(REF).read()
smpl_x = types.SimpleNamespace(vertex_num=V_FULL, face_vertex_idx=None, flip_corr=None,
                               joint={'num': J, 'name': ['J%d' % j for j in range(J)]})
ns = {'torch': torch, 'nn': nn, 'np': np, 'smpl_x': smpl_x, 'axis_angle_to_matrix': p3d_standins.axis_angle_to_matrix}
lines = src.splitlines()
for node in ast.parse(src).body:
    if isinstance(node, ast.ClassDef) and node.name in ('EdgeLengthLoss', 'FaceOffsetSymmetricReg', 'PoseLoss'):
        exec('\n'.join(lines[node.lineno - 1: node.end_lineno]), ns)


def run(fn, x, others, g, dtype):
    """(value, autograd gradient w.r.t. x) of fn(x, *others) in ``dtype``; ``.float()`` and FloatTensor widened for float64."""
    _float, _ft = torch.Tensor.float, torch.FloatTensor
    if dtype == torch.float64:
        torch.Tensor.float = lambda self, *a, **k: self.double()
        torch.FloatTensor = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    try:
        x = torch.from_numpy(x).to(dtype).requires_grad_(True)
        y = fn(x, *[torch.from_numpy(o).to(dtype) for o in others])
        assert y.dtype == dtype
        (gx,) = torch.autograd.grad(y, x, torch.from_numpy(g).to(dtype).reshape(y.shape))
    finally:
        torch.Tensor.float, torch.FloatTensor = _float, _ft
    return y.detach().numpy(), gx.numpy()


def centred(a, t, w):
    return torch.abs((a - a.mean(1)[:, None, :]) - (t - t.mean(1)[:, None, :]).detach()) * w * 10


def record(rec, name, inputs, results):
    (l32, g32), (l64, g64) = results
    rec.update({'%s_%s' % (name, k): v for k, v in inputs.items()})
    rec.update({name + '_loss32': l32, name + '_grad32': g32, name + '_loss64': l64, name + '_grad64': g64})


_cuda = torch.Tensor.cuda
torch.Tensor.cuda = lambda self, *a, **k: self.clone()
try:
    rec = {}
    # ---- edge length: the tie is edge (0, 1) of face 0, out == gt at both of its ends
    for seed in range(100, 200):
        c = fo.edge_case(seed, B, VF, NF)
        a, b = c['face'][0, 0], c['face'][0, 1]
        c['out'][:, [a, b]] = c['gt'][:, [a, b]]
        if not fo.edge_ambiguous(c['out'], c['gt'], c['face']).any():
            break
    else:
        raise SystemExit('no clean edge seed')
    m = ns['EdgeLengthLoss'](c['face'])
    res = [run(m, c['out'], (c['gt'], c['valid']), c['g'], dt) for dt in (torch.float32, torch.float64)]
    assert np.isfinite(res[0][1]).all() and res[0][0][:, 0, 0].max() == 0, 'the tied edge: loss 0, finite gradient'
    record(rec, 'edge', dict(c, seed=np.int64(seed)), res)
    print('edge: seed %d' % seed)

    # ---- flip symmetry: row 0 is the zero row whose taps carry no offset
    for seed in range(200, 300):
        c = fo.sym_case(seed, B, V_FULL, VF, hub=5)
        taps, weights, _, _ = fo.flip_plan(V_FULL, c['face_vertex_idx'], c['closest_faces'], c['bc'])
        if not fo.sym_ambiguous(c['p'], taps, weights).any():
            break
    else:
        raise SystemExit('no clean symmetry seed')
    assert (taps[0] == -1).all() and (taps == -1).sum() > 3 and taps[2, 1] == 2
    smpl_x.face_vertex_idx = c['face_vertex_idx']
    smpl_x.flip_corr = {'closest_faces': c['closest_faces'], 'bc': c['bc']}
    m = ns['FaceOffsetSymmetricReg']()
    res = [run(m, c['p'], (), c['g'], dt) for dt in (torch.float32, torch.float64)]
    assert (res[0][0][:, 0] == 0).all() and np.isfinite(res[0][1]).all(), 'the zero row: loss 0 (its gradient is what the rows that tap it send)'
    record(rec, 'sym', {k: (np.int64(v) if k == 'vertex_num' else v) for k, v in dict(c, seed=seed).items()}, res)
    print('sym: seed %d, %d taps of -1' % (seed, (taps == -1).sum()))

    # ---- pose (pinned by the stand-in only): row 3 has out == gt
    for seed in range(300, 400):
        c = fo.pose_case(seed, B * J, special=False)
        c['out'][3] = c['gt'][3]
        if not fo.pose_ambiguous(c['out'], c['gt']).any():
            break
    else:
        raise SystemExit('no clean pose seed')
    m = ns['PoseLoss']()
    c = {k: v.reshape(B, -1) for k, v in c.items()}
    res = [run(m, c['out'], (c['gt'],), c['g'], dt) for dt in (torch.float32, torch.float64)]
    assert res[0][0].shape == (B, J, 3, 3) and (res[0][1].reshape(-1, 3)[3] == 0).all()
    record(rec, 'pose', dict(c, seed=np.int64(seed)), res)
    print('pose: seed %d' % seed)

    # ---- the centred vertex-to-vertex term
    for seed in range(400, 500):
        c = fo.v2v_case(seed, B, VF)
        if not fo.v2v_ambiguous(c['out'], c['target']).any():
            break
    else:
        raise SystemExit('no clean v2v seed')
    res = [run(centred, c['out'], (c['target'], c['weight']), c['g'], dt) for dt in (torch.float32, torch.float64)]
    record(rec, 'v2v', dict(c, seed=np.int64(seed)), res)
    print('v2v: seed %d' % seed)
finally:
    torch.Tensor.cuda = _cuda

for name in ('edge', 'sym', 'pose', 'v2v'):
    e = np.abs(rec[name + '_loss32'] - rec[name + '_loss64']).max()
    ge = np.abs(rec[name + '_grad32'] - rec[name + '_grad64']).max()
    print('%-5s reference float32 error: loss %.3e, gradient %.3e (max |gradient| %.3e)' % (
        name, e, ge, np.abs(rec[name + '_grad64']).max()))
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ref_fit_terms.npz')
np.savez_compressed(path, **rec)
print('wrote', path, os.path.getsize(path), 'bytes')
assert os.path.getsize(path) < 100_000
