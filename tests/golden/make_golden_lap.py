"""Generates tests/golden/ref_lap.npz by EXECUTING the reference's own ``LaplacianReg``.

``/root/reference/avatar/common/nets/loss.py`` cannot be imported as a module here (it imports lpips, pytorch3d and
the training config at the top), so the source text of ``class LaplacianReg`` is cut out of the file with ``ast`` and
exec'd unchanged in a namespace holding only torch / nn / np; ``Tensor.cuda()`` is a no-op for the duration (this
container has no GPU).  Run from the repo root:  python tests/golden/make_golden_lap.py
Nothing here is read at test time on the GPU box -- only the .npz travels.

The fixture mesh: a 13 x 14 triangulated grid (corners of valence 2 and 3, edges of 4, interior of 6) and a closed fan
whose hub has 16 neighbours -- more than the table's ten slots.  The rim is numbered across a multiple of 64, so that
the order in which CPython iterates the hub's set is not ascending and the ten neighbours the reference keeps are not
the ten smallest (asserted below: a rim that the set happens to iterate in ascending order would prove nothing).
"""
import ast
import os

import numpy as np
import torch
import torch.nn as nn

REF = '/root/reference/avatar/common/nets/loss.py'
src = open(REF).read()
ns = {'torch': torch, 'nn': nn, 'np': np}
lines = src.splitlines()
for node in ast.parse(src).body:
    if isinstance(node, ast.ClassDef) and node.name == 'LaplacianReg':
        exec('\n'.join(lines[node.lineno - 1: node.end_lineno]), ns)

ROWS, COLS, RIM = 13, 14, 16
r, c = np.meshgrid(np.arange(ROWS - 1), np.arange(COLS - 1), indexing='ij')
a = (r * COLS + c).reshape(-1)
grid = np.concatenate([np.stack([a, a + 1, a + COLS], 1), np.stack([a + 1, a + COLS + 1, a + COLS], 1)])
hub = ROWS * COLS
rim = hub + 1 + np.random.RandomState(7).permutation(RIM)           # the fan walks the rim in a shuffled numbering
fan = np.stack([np.full(RIM, hub), rim, np.roll(rim, -1)], 1)
face = np.concatenate([grid, fan]).astype(np.int64)
V = hub + 1 + RIM

_cuda = torch.Tensor.cuda
torch.Tensor.cuda = lambda self, *a, **k: self
try:
    reg = ns['LaplacianReg'](V, face)
    idxs, weights = reg.neighbor_idxs.numpy(), reg.neighbor_weights.numpy()
    kept = idxs[hub]
    assert len(set(kept.tolist())) == 10 and hub not in kept, 'the hub row is full'
    assert sorted(kept.tolist()) != sorted(rim.tolist())[:10], 'the kept ten must not be the ten smallest'
    assert kept.tolist() != sorted(kept.tolist()), 'the kept ten must not come out ascending'
    valence = (weights != 0).sum(1)
    assert {2, 3, 4, 6, 10} <= set(valence.tolist())

    g = torch.Generator().manual_seed(2025)
    B, C = 2, 3
    out_ = torch.randn(B, V, C, generator=g)
    target = out_ + 0.3 * torch.randn(B, V, C, generator=g)
    target1 = target[:1].clone()
    G = torch.randn(B, V, C, generator=g)
    rec = dict(face=face, neighbor_idxs=idxs, neighbor_weights=weights, hub=np.int64(hub), rim=rim, out=out_.numpy(),
               target=target.numpy(), target1=target1.numpy(), G=G.numpy())
    for name, t in (('none', None), ('target', target), ('target1', target1)):
        x = out_.clone().requires_grad_(True)
        loss = reg(x, t)
        (loss * G).sum().backward()
        rec['loss_' + name] = loss.detach().numpy()
        rec['grad_' + name] = x.grad.numpy()
finally:
    torch.Tensor.cuda = _cuda
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ref_lap.npz')
np.savez_compressed(path, **rec)
print('wrote', path, os.path.getsize(path), 'bytes; hub row', kept.tolist())
