"""Generates tests/golden/ref_skinning.npz by EXECUTING the reference's own skinning code.

``HumanGaussian.get_transform_mat_vertex`` and ``HumanGaussian.lbs`` (/root/reference/avatar/common/nets/module.py:413-422)
and the camera -> world block of ``HumanGaussian.forward`` (``if not is_world_coord:``, module.py:554-556) are the code
``exavatar_release_amd.skin_points`` replaces.  ``module.py`` cannot be imported here (pytorch3d, smplx, the training
config), so the two methods and the block are cut out of the file with ``ast`` and exec'd UNCHANGED -- as
``make_golden_renderer.py`` does for ``GaussianRenderer`` -- in a namespace that holds what they use: ``torch`` and a stub
``smpl_x`` with the two attributes they read (``joint_num``, ``vertex_num_upsampled``).  ``Tensor.cuda()`` is the
identity for the duration.  Everything runs in float64 on the CPU, with autograd for the gradients.  Nothing of the
reference's text is written anywhere: only inputs and outputs travel.  Run from the repo root:
python tests/golden/make_golden_skinning.py
"""
import ast
import os
import sys
import textwrap
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))
REF_MODULE = '/root/reference/avatar/common/nets/module.py'


def reference_code():
    """(source of the two methods, source of the camera block), dedented, cut from the reference unchanged."""
    src = open(REF_MODULE).read()
    lines = src.splitlines()
    text = lambda node: textwrap.dedent('\n'.join(lines[node.lineno - 1: node.end_lineno]))      # noqa: E731
    methods, block = {}, None
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.ClassDef) and node.name == 'HumanGaussian':
            for f in node.body:
                if isinstance(f, ast.FunctionDef) and f.name in ('get_transform_mat_vertex', 'lbs'):
                    methods[f.name] = text(f)
                if isinstance(f, ast.FunctionDef) and f.name == 'forward':
                    for s in ast.walk(f):
                        if (isinstance(s, ast.If) and isinstance(s.test, ast.UnaryOp) and isinstance(s.test.op, ast.Not)
                                and isinstance(s.test.operand, ast.Name) and s.test.operand.id == 'is_world_coord'):
                            block = text(s)
    if sorted(methods) != ['get_transform_mat_vertex', 'lbs'] or block is None:
        raise RuntimeError('the skinning code was not found in ' + REF_MODULE)
    return methods['get_transform_mat_vertex'] + '\n\n' + methods['lbs'], block


def rigid(J, g):
    """[J, 4, 4] rigid transforms: a random rotation (QR of a Gaussian matrix) and translation, bottom row (0, 0, 0, 1)."""
    T = torch.zeros(J, 4, 4, dtype=torch.float64)
    for j in range(J):
        q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
        T[j, :3, :3] = q * torch.sign(torch.diagonal(r))[None, :]
        T[j, :3, 3] = 0.3 * torch.randn(3, generator=g, dtype=torch.float64)
    T[:, 3, 3] = 1.0
    return T


def sparse_weights(Vw, J, g):
    """At most 4 non-zeros per row that sum to 1 (the structure of SMPL-X's skinning weights)."""
    W = torch.zeros(Vw, J, dtype=torch.float64)
    for v in range(Vw):
        k = int(torch.randint(1, 5, (1,), generator=g))
        cols = torch.randperm(J, generator=g)[:k]
        w = torch.rand(k, generator=g, dtype=torch.float64) + 0.05
        W[v, cols] = w / w.sum()
    return W


def cases():
    """(name, V, Vw, J, S, use idx, camera step, rigid T, sparse weights)."""
    yield 'smplx', 700, 500, 55, 2, True, True, True, True
    yield 'dense', 300, 300, 24, 2, False, False, False, False
    yield 'cam_general', 260, 120, 7, 2, True, True, False, False


def main():
    methods, block = reference_code()
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        out = {}
        names = []
        for name, V, Vw, J, S, use_idx, cam, is_rigid, sparse in cases():
            g = torch.Generator().manual_seed(len(names) + 11)
            ns = {'torch': torch, 'smpl_x': types.SimpleNamespace(joint_num=J, vertex_num_upsampled=V)}
            exec(methods, ns)
            weights = sparse_weights(Vw, J, g) if sparse else torch.rand(Vw, J, generator=g, dtype=torch.float64)
            idx = torch.randint(0, Vw, (V,), generator=g) if use_idx else torch.arange(V)
            T = (rigid(J, g) if is_rigid else torch.randn(J, 4, 4, generator=g, dtype=torch.float64)).requires_grad_(True)
            trans = (0.5 * torch.randn(1, 3, generator=g, dtype=torch.float64)).requires_grad_(True)
            pts = [(0.4 * torch.randn(V, 3, generator=g, dtype=torch.float64)).requires_grad_(True) for _ in range(S)]
            R = rigid(1, g)[0, :3, :3]
            t = 0.7 * torch.randn(3, generator=g, dtype=torch.float64)
            self = types.SimpleNamespace(skinning_weight=weights)
            tmv = ns['get_transform_mat_vertex'](self, T, idx)
            mean_3d = ns['lbs'](self, pts[0], tmv, trans)
            mean_3d_refined = ns['lbs'](self, pts[1], tmv, trans)
            if cam:
                loc = {'mean_3d': mean_3d, 'mean_3d_refined': mean_3d_refined, 'is_world_coord': False,
                       'cam_param': {'R': R, 't': t}, 'torch': torch}
                exec(block, ns, loc)
                mean_3d, mean_3d_refined = loc['mean_3d'], loc['mean_3d_refined']
            posed = [mean_3d, mean_3d_refined]
            G = [torch.randn(V, 3, generator=g, dtype=torch.float64) for _ in range(S)]
            grads = torch.autograd.grad(posed, [T, trans] + pts, G)
            p = name + '_'
            out[p + 'dims'] = np.array([V, Vw, J, S, int(use_idx), int(cam)])
            out[p + 'weights'] = weights.numpy()
            out[p + 'idx'] = idx.numpy()
            out[p + 'T'] = T.detach().numpy()
            out[p + 'trans'] = trans.detach().numpy()
            out[p + 'R'] = R.numpy()
            out[p + 't'] = t.numpy()
            for s in range(S):
                out[p + 'points%d' % s] = pts[s].detach().numpy()
                out[p + 'posed%d' % s] = posed[s].detach().numpy()
                out[p + 'G%d' % s] = G[s].numpy()
                out[p + 'grad_points%d' % s] = grads[2 + s].numpy()
            out[p + 'grad_T'] = grads[0].numpy()
            out[p + 'grad_trans'] = grads[1].numpy()
            names.append(name)
        out['cases'] = np.array(names)
    finally:
        torch.Tensor.cuda = orig_cuda
    path = os.path.join(HERE, 'ref_skinning.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', names)


if __name__ == '__main__':
    main()
