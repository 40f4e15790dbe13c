"""Generates tests/golden/ref_blend.npz by EXECUTING the reference's own blend-shape code.

``HumanGaussian.get_mean_offset_offset`` (/root/reference/avatar/common/nets/module.py:473-493) and the expression
statement of ``HumanGaussian.forward`` (``smplx_expr_offset = ...``, module.py:537) are the code
``exavatar_release_amd.BlendShapes`` replaces.  ``module.py`` cannot be imported here (pytorch3d, smplx, the training
config), so the method and the statement are cut out of the file with ``ast`` and exec'd UNCHANGED -- as
``make_golden_skinning.py`` does -- in a namespace that holds what they use: ``torch``, a stub ``smpl_x`` with the
attributes they read (``joint_part``, ``joint_num``, ``vertex_num_upsampled``) and this repository's
``axis_angle_to_matrix``.  ``Tensor.cuda()`` is the identity for the duration.  Everything runs in float64 on the CPU,
with autograd for the gradients.

Inputs are stored as fp32-representable values, so that no input rounding enters the comparison.  The one input the
reference forms itself is the pose feature ``axis_angle_to_matrix(pose) - I``: the stub rounds the rotation matrices to
fp32 (values only; they stay float64 tensors), and the poses are kept below one radian, where every diagonal entry is
at least 0.5 and the subtraction of the identity is exact and fp32-representable -- asserted below.

Nothing of the reference's text is written anywhere: only inputs and outputs travel.  Run from the repo root:
python tests/golden/make_golden_blend.py
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

from exavatar_release_amd.p3d_standins import axis_angle_to_matrix as _axis_angle_to_matrix      # noqa: E402


def reference_code():
    """(source of get_mean_offset_offset, source of the expression statement), dedented, cut from the reference unchanged."""
    src = open(REF_MODULE).read()
    lines = src.splitlines()
    text = lambda node: textwrap.dedent('\n'.join(lines[node.lineno - 1: node.end_lineno]))      # noqa: E731
    method, stmt = None, None
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.ClassDef) and node.name == 'HumanGaussian':
            for f in node.body:
                if isinstance(f, ast.FunctionDef) and f.name == 'get_mean_offset_offset':
                    method = text(f)
                if isinstance(f, ast.FunctionDef) and f.name == 'forward':
                    for s in ast.walk(f):
                        if (isinstance(s, ast.Assign) and len(s.targets) == 1 and isinstance(s.targets[0], ast.Name)
                                and s.targets[0].id == 'smplx_expr_offset'):
                            stmt = text(s)
    if method is None or stmt is None:
        raise RuntimeError('the blend-shape code was not found in ' + REF_MODULE)
    return method, stmt


def f32(t):
    """The nearest fp32-representable values, as float64."""
    return t.float().double()


def small_poses(n, g):
    """[n, 3] axis-angle vectors of at most one radian."""
    p = 0.35 * torch.randn(n, 3, generator=g, dtype=torch.float64)
    norm = p.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return f32(p * torch.clamp(norm, max=1.0) / norm)


def pose_cases():
    """(name, V, body joints with the root, hand joints per hand, share of masked vertices)."""
    yield 'smplx', 96, 22, 15, 0.4           # 21 + 3 + 15 + 15 = 54 joints: K = 486
    yield 'small', 300, 3, 1, 0.25           # 2 + 3 + 1 + 1 = 7 joints: K = 63


def main():
    method, stmt = reference_code()
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    seen = []

    def axis_angle_to_matrix(p):
        R = f32(_axis_angle_to_matrix(p))
        seen.append(R)
        return R

    try:
        out, names = {}, []
        for name, V, body, hand, share in pose_cases():
            g = torch.Generator().manual_seed(len(names) + 41)
            joints = body - 1 + 3 + 2 * hand
            K = joints * 9
            smpl_x = types.SimpleNamespace(joint_part={'body': list(range(body)), 'lhand': list(range(hand)),
                                                       'rhand': list(range(hand))},
                                           joint_num=joints + 1, vertex_num_upsampled=V)
            ns = {'torch': torch, 'smpl_x': smpl_x, 'axis_angle_to_matrix': axis_angle_to_matrix}
            exec(method, ns)
            parts = torch.rand(V, generator=g)
            is_rhand, is_lhand = parts < share / 4, (parts >= share / 4) & (parts < share / 2)
            is_face_expr = (parts >= share / 2) & (parts < share)
            pose_dirs = f32(torch.randn(K, 3 * V, generator=g, dtype=torch.float64) * 0.02)
            self = types.SimpleNamespace(pose_dirs=pose_dirs, is_rhand=is_rhand, is_lhand=is_lhand, is_face_expr=is_face_expr)
            param = {'body_pose': small_poses(body - 1, g).reshape(-1), 'jaw_pose': small_poses(1, g).reshape(-1),
                     'leye_pose': small_poses(1, g).reshape(-1), 'reye_pose': small_poses(1, g).reshape(-1),
                     'lhand_pose': small_poses(hand, g).reshape(-1), 'rhand_pose': small_poses(hand, g).reshape(-1)}
            moo = f32(0.01 * torch.randn(V, 3, generator=g, dtype=torch.float64)).requires_grad_(True)
            del seen[:]
            combined, masked = ns['get_mean_offset_offset'](self, param, moo)
            feat = (seen[0] - torch.eye(3, dtype=torch.float64)[None]).reshape(1, K)
            assert len(seen) == 1 and torch.equal(feat, f32(feat)), 'the pose feature is not fp32-representable'
            G = [f32(torch.randn(V, 3, generator=g, dtype=torch.float64)) for _ in range(2)]
            grad, = torch.autograd.grad([combined, masked], moo, G)
            p = name + '_'
            out[p + 'pose_dirs'] = pose_dirs.numpy().astype(np.float32)
            out[p + 'pose_mask'] = (is_rhand | is_lhand | is_face_expr).numpy()
            out[p + 'pose_feat'] = feat.numpy().astype(np.float32)
            out[p + 'mean_offset_offset'] = moo.detach().numpy().astype(np.float32)
            out[p + 'G_combined'] = G[0].numpy().astype(np.float32)
            out[p + 'G_masked'] = G[1].numpy().astype(np.float32)
            out[p + 'combined'] = combined.detach().numpy()
            out[p + 'masked'] = masked.detach().numpy()
            out[p + 'grad_mean_offset_offset'] = grad.numpy()
            names.append(name)
        out['pose_cases'] = np.array(names)

        # the expression statement: expr_dirs non-zero on a subset of the rows only
        g = torch.Generator().manual_seed(53)
        V, Ke = 400, 10
        face = torch.rand(V, generator=g) < 0.3
        expr_dirs = f32(torch.randn(V, 3, Ke, generator=g, dtype=torch.float64) * 0.05) * face[:, None, None]
        expr = f32(torch.randn(Ke, generator=g, dtype=torch.float64)).requires_grad_(True)
        loc = {'smplx_param': {'expr': expr}, 'self': types.SimpleNamespace(expr_dirs=expr_dirs), 'torch': torch}
        exec(stmt, {'torch': torch}, loc)
        offset = loc['smplx_expr_offset']
        G = f32(torch.randn(V, 3, generator=g, dtype=torch.float64))
        grad, = torch.autograd.grad(offset, expr, G)
        out['expr_expr_dirs'] = expr_dirs.numpy().astype(np.float32)
        out['expr_expr'] = expr.detach().numpy().astype(np.float32)
        out['expr_G'] = G.numpy().astype(np.float32)
        out['expr_offset'] = offset.detach().numpy()
        out['expr_grad_expr'] = grad.numpy()
    finally:
        torch.Tensor.cuda = orig_cuda
    path = os.path.join(HERE, 'ref_blend.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', names)


if __name__ == '__main__':
    main()
