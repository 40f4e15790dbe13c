"""Generates tests/golden/ref_posed.npz by EXECUTING the reference's own posed SMPL-X layer.

``lbs``, ``blend_shapes``, ``vertices2joints``, ``batch_rodrigues``, ``transform_mat`` and ``batch_rigid_transform``
(/root/reference/avatar/common/utils/smplx/smplx/lbs.py) and ``Model.get_smplx_outputs``
(/root/reference/avatar/main/model.py:37-58) are the code ``exavatar_release_amd.PosedBody`` replaces.  Neither file can
be imported here (pytorch3d, smplx's model files, the training config), so the functions are cut out of the files with
``ast`` and exec'd UNCHANGED -- as ``make_golden_body.py`` does -- in a namespace that holds what they use: ``torch``, the
typing names, a stub ``smpl_x`` with the constants of the synthetic body and a stub ``smplx_layer`` that assembles the
full pose (``+ pose_mean``), the coefficients and the shape directions and applies ``transl`` as ``SMPLX.forward`` does
around that ``lbs``.  The run is made twice on the CPU with autograd over seeded cotangents on all three outputs
(``vertices``, ``joints`` and the world-space mesh ``get_smplx_outputs`` returns): in float64 -- the fixture's values --
and in float32, of which only the largest error of every output and gradient against the float64 run is kept
(``ref_f32_err/<name>``: what the reference's own arithmetic loses).  Nothing of the reference's text is written
anywhere: only outputs, gradients, those errors and a SHA-256 per input travel (the inputs are
``tests/posed_oracle.golden_inputs()``).  Run from the repo root:
python tests/golden/make_golden_posed.py
"""
import os
import sys
import types
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
HERE = os.path.dirname(os.path.abspath(__file__))
REF_MODEL = '/root/reference/avatar/main/model.py'
REF_LBS = '/root/reference/avatar/common/utils/smplx/smplx/lbs.py'

import posed_oracle      # noqa: E402
from make_golden_kinematics import _cut      # noqa: E402

NAMES = ('vertices', 'joints', 'vertices_world', 'rot', 'grad_pose', 'grad_betas', 'grad_expression', 'grad_transl',
         'grad_joint_offset')
ORDER = (('root_pose', 0, 1), ('body_pose', 1, 22), ('jaw_pose', 22, 23), ('leye_pose', 23, 24), ('reye_pose', 24, 25),
         ('lhand_pose', 25, 40), ('rhand_pose', 40, 55))


def run(dtype):
    """{name: numpy array} of the reference's run in ``dtype`` on the CPU."""
    torch.set_default_dtype(dtype)
    torch.Tensor.cuda = lambda self, *a, **k: self            # no device here: the tensors stay on the CPU
    case, inputs, cot = posed_oracle.golden_inputs()
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)      # noqa: E731
    J = 55

    names = ['lbs', 'blend_shapes', 'vertices2joints', 'batch_rodrigues', 'transform_mat', 'batch_rigid_transform']
    fns = _cut(REF_LBS, names)
    ns = {'torch': torch, 'F': F, 'Tensor': torch.Tensor, 'Tuple': Tuple, 'Optional': Optional, 'np': np}
    exec('\n\n'.join(fns[n] for n in names), ns)
    exec(_cut(REF_MODEL, ['get_smplx_outputs'], 'Model')['get_smplx_outputs'], ns)

    n_betas = inputs['betas'].shape[0]
    smpl_x = types.SimpleNamespace(joint_part={'body': list(range(22)), 'lhand': list(range(15)), 'rhand': list(range(15))},
                                   expr_param_dim=inputs['expression'].shape[0], face_offset=t(case['face_offset']))
    ns['smpl_x'] = smpl_x

    # the stub layer: SMPLX.forward's assembly around the reference's lbs
    parents = torch.tensor(list(case['parents']))
    shapedirs, expr_dirs = t(case['shape_dirs'][:, :, :n_betas]), t(case['shape_dirs'][:, :, n_betas:])
    pose_mean = t(case['pose_mean']).reshape(-1)
    seen = {}

    def smplx_layer(global_orient, body_pose, jaw_pose, leye_pose, reye_pose, left_hand_pose, right_hand_pose, expression,
                    betas, transl, face_offset=None, joint_offset=None):
        full_pose = torch.cat([global_orient.reshape(-1, 1, 3), body_pose.reshape(-1, 21, 3), jaw_pose.reshape(-1, 1, 3),
                               leye_pose.reshape(-1, 1, 3), reye_pose.reshape(-1, 1, 3),
                               left_hand_pose.reshape(-1, 15, 3), right_hand_pose.reshape(-1, 15, 3)], 1).reshape(-1, 165)
        full_pose += pose_mean
        seen['full_pose'] = full_pose.detach().clone()
        shape_components = torch.cat([betas, expression], dim=-1)
        dirs = torch.cat([shapedirs, expr_dirs], dim=-1)
        vertices = t(case['v_template']) if face_offset is None else t(case['v_template']) + face_offset
        vertices, joints = ns['lbs'](shape_components, full_pose, vertices, dirs, t(case['posedirs']),
                                     t(case['J_regressor']), joint_offset, None, parents, t(case['weights']))
        joints = torch.cat([joints, joints[:, :0]], dim=1)       # where the extra joints and the landmarks are appended
        joints += transl.unsqueeze(dim=1)
        vertices += transl.unsqueeze(dim=1)
        seen['output'] = types.SimpleNamespace(vertices=vertices, joints=joints)
        return seen['output']

    pose = t(inputs['pose'])
    param = {k: pose[a:b].reshape(-1).clone().requires_grad_(True) for k, a, b in ORDER}
    param['expr'] = t(inputs['expression']).requires_grad_(True)
    param['trans'] = t(inputs['transl']).requires_grad_(True)
    shape_param = t(inputs['betas']).requires_grad_(True)
    joint_offset = t(inputs['joint_offset']).requires_grad_(True)
    self = types.SimpleNamespace(smplx_layer=smplx_layer,
                                 human_gaussian=types.SimpleNamespace(shape_param=shape_param, joint_offset=joint_offset))
    cam = {'R': t(inputs['R']), 't': t(inputs['t'])}
    world = ns['get_smplx_outputs'](self, param, cam)
    vertices, joints = seen['output'].vertices[0], seen['output'].joints[0, :J]
    wrt = [param[k] for k, _, _ in ORDER] + [shape_param, param['expr'], param['trans'], joint_offset]
    grads = torch.autograd.grad([vertices, joints, world], wrt, [t(cot[k]) for k in posed_oracle.OUTPUTS])
    out = dict(vertices=vertices, joints=joints, vertices_world=world,
               rot=ns['batch_rodrigues'](seen['full_pose'].view(J, 3)), grad_pose=torch.cat([g.view(-1, 3) for g in grads[:7]]),
               grad_betas=grads[7], grad_expression=grads[8], grad_transl=grads[9], grad_joint_offset=grads[10])
    return {k: v.detach().numpy() for k, v in out.items()}, (case, inputs, cot)


def main():
    ref, (case, inputs, cot) = run(torch.float64)
    low, _ = run(torch.float32)
    torch.set_default_dtype(torch.float32)
    out = dict(ref)
    for k in NAMES:
        assert ref[k].dtype == np.float64 and low[k].dtype == np.float32 and ref[k].shape == low[k].shape, k
        out['ref_f32_err/' + k] = np.abs(low[k].astype(np.float64) - ref[k]).max()
        print('%-20s max |value| %.6g   ref_f32_err %.6g' % (k, np.abs(ref[k]).max(), out['ref_f32_err/' + k]))
    digests = posed_oracle.golden_digests(case, inputs, cot)
    out['digest_names'] = np.array(sorted(digests))
    out['digest_values'] = np.array([digests[k] for k in sorted(digests)])
    path = os.path.join(HERE, 'ref_posed.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
