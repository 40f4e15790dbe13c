"""Generates tests/golden/ref_kinematics.npz by EXECUTING the reference's own forward kinematics.

``batch_rigid_transform`` and ``transform_mat`` (/root/reference/avatar/common/utils/smplx/smplx/lbs.py:348-417) and
``HumanGaussian.get_transform_mat_joint`` (/root/reference/avatar/common/nets/module.py:389-411) are the code
``exavatar_release_amd.joint_transforms`` replaces.  Neither file can be imported here (pytorch3d, smplx, the training
config), so the three functions are cut out of the files with ``ast`` and exec'd UNCHANGED -- as
``make_golden_skinning.py`` does -- in a namespace that holds what they use: ``torch``, ``F``, ``Tensor``, a stub
``smpl_x`` with the ``joint_part`` lengths, and ``axis_angle_to_matrix`` from ``p3d_standins`` (the restatement of
pytorch3d's).  Everything runs in float64 on the CPU, with autograd for the gradients.  Nothing of the reference's text
is written anywhere: only inputs and outputs travel.  Run from the repo root:
python tests/golden/make_golden_kinematics.py
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
REF_LBS = '/root/reference/avatar/common/utils/smplx/smplx/lbs.py'

from exavatar_release_amd import lbs, p3d_standins      # noqa: E402


def _cut(path, names, cls=None):
    """{name: source} of the functions ``names`` of ``path`` (methods of ``cls`` when given), dedented, unchanged."""
    src = open(path).read()
    lines = src.splitlines()
    text = lambda node: textwrap.dedent('\n'.join(lines[node.lineno - 1: node.end_lineno]))      # noqa: E731
    tree = ast.parse(src)
    body = tree.body
    if cls is not None:
        body = [n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == cls][0].body
    found = {f.name: text(f) for f in body if isinstance(f, ast.FunctionDef) and f.name in names}
    if sorted(found) != sorted(names):
        raise RuntimeError('%s were not all found in %s' % (names, path))
    return found


def rigid(J, g):
    """[J, 4, 4] rigid transforms: a random rotation (QR of a Gaussian matrix) and translation."""
    T = torch.zeros(J, 4, 4, dtype=torch.float64)
    for j in range(J):
        q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
        T[j, :3, :3] = q * torch.sign(torch.diagonal(r))[None, :]
        T[j, :3, 3] = 0.3 * torch.randn(3, generator=g, dtype=torch.float64)
    T[:, 3, 3] = 1.0
    return T


def main():
    fns = _cut(REF_LBS, ['transform_mat', 'batch_rigid_transform'])
    method = _cut(REF_MODULE, ['get_transform_mat_joint'], 'HumanGaussian')['get_transform_mat_joint']
    parts = {'body': list(range(22)), 'lhand': list(range(15)), 'rhand': list(range(15))}
    ns = {'torch': torch, 'F': F, 'Tensor': torch.Tensor, 'smpl_x': types.SimpleNamespace(joint_part=parts),
          'axis_angle_to_matrix': p3d_standins.axis_angle_to_matrix}
    exec(fns['transform_mat'] + '\n\n' + fns['batch_rigid_transform'] + '\n\n' + method, ns)
    out = {}

    # SMPL-X tree, J = 55, through get_transform_mat_joint (with the big-pose transforms); the eyes' poses are zero
    g = torch.Generator().manual_seed(21)
    parents = torch.tensor(lbs.SMPLX_PARENTS)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    param = {'root_pose': 0.8 * rnd(3), 'body_pose': 0.4 * rnd(63), 'jaw_pose': 0.2 * rnd(3),
             'leye_pose': torch.zeros(3, dtype=torch.float64), 'reye_pose': torch.zeros(3, dtype=torch.float64),
             'lhand_pose': 0.3 * rnd(45), 'rhand_pose': 0.3 * rnd(45), 'trans': rnd(3)}
    order = ['root_pose', 'body_pose', 'jaw_pose', 'leye_pose', 'reye_pose', 'lhand_pose', 'rhand_pose']
    for k in order:
        param[k].requires_grad_(True)
    joints = (0.3 * rnd(55, 3)).requires_grad_(True)
    pre = rigid(55, g).requires_grad_(True)
    self = types.SimpleNamespace(smplx_layer=types.SimpleNamespace(parents=parents))
    T = ns['get_transform_mat_joint'](self, pre, joints, param)
    G = rnd(55, 4, 4)
    grads = torch.autograd.grad(T, [param[k] for k in order] + [joints, pre], G)
    out['smplx_parents'] = parents.numpy()
    out['smplx_pose'] = torch.cat([param[k].detach().view(-1, 3) for k in order]).numpy()
    out['smplx_joints'] = joints.detach().numpy()
    out['smplx_pre'] = pre.detach().numpy()
    out['smplx_transforms'] = T.detach().numpy()
    out['smplx_G'] = G.numpy()
    out['smplx_grad_pose'] = torch.cat([x.view(-1, 3) for x in grads[:7]]).numpy()
    out['smplx_grad_joints'] = grads[7].numpy()
    out['smplx_grad_pre'] = grads[8].numpy()

    # J = 7, B = 3 through batch_rigid_transform alone: general (not orthogonal) matrices, both outputs
    g = torch.Generator().manual_seed(22)
    parents = torch.tensor([-1, 0, 1, 1, 0, 4, 2])
    rot = rnd(3, 7, 3, 3).requires_grad_(True)
    joints = rnd(3, 7, 3).requires_grad_(True)
    posed, rel = ns['batch_rigid_transform'](rot, joints, parents, dtype=torch.float64)
    Gp, Gr = rnd(3, 7, 3), rnd(3, 7, 4, 4)
    grads = torch.autograd.grad([posed, rel], [rot, joints], [Gp, Gr])
    out['tree7_parents'] = parents.numpy()
    out['tree7_rot'] = rot.detach().numpy()
    out['tree7_joints'] = joints.detach().numpy()
    out['tree7_posed'] = posed.detach().numpy()
    out['tree7_transforms'] = rel.detach().numpy()
    out['tree7_G_posed'] = Gp.numpy()
    out['tree7_G_transforms'] = Gr.numpy()
    out['tree7_grad_rot'] = grads[0].numpy()
    out['tree7_grad_joints'] = grads[1].numpy()

    path = os.path.join(HERE, 'ref_kinematics.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
