"""Generates tests/golden/ref_keypoints.npz by EXECUTING the reference's own keypoint path on the CPU.

The reference's modules cannot be imported here (the fitting config, the ``smpl_x`` singleton and pytorch3d are pulled in at
the top), so the source text of ``find_dynamic_lmk_idx_and_bcoords``, ``vertices2landmarks``, ``batch_rodrigues``
(``smplx/lbs.py``), ``rot_mat_to_euler`` and ``to_tensor`` (``smplx/utils.py``), ``VertexJointSelector``
(``smplx/vertex_joint_selector.py``) and ``CoordLoss`` (``fitting/common/nets/loss.py``) is cut out of the files with ``ast``
and exec'd unchanged in a namespace holding torch / nn / np / F and a stub ``smpl_x`` (``kpt``).  ``Tensor.cuda()`` returns a
copy for the duration (this container has no GPU).  The float64 run is the same source on the same numbers with
``torch.FloatTensor`` widened to a float64 constructor.  The five lines that string the functions together in
``SMPLX.forward`` (``body_models.py:1257-1283``) and the tail of ``get_smplx_coord`` (``fitting/main/model.py:97-112``) sit in
methods that cannot be cut out and are restated below, evaluated by torch on the same numbers.  Gradients are autograd's for
recorded random cotangents.
Run from the repo root:  python tests/golden/make_golden_keypoints.py
Nothing here is read at test time on the GPU box -- only the .npz travels.

Sizes: V = 30, F = 120, J = 8, Ls = 4, Ld = 5, E = 3, B = 6 for the layer; B = 6, K = 50 for CoordLoss.  The six items' yaw
angles cover bin 0, a positive bin, a negative bin (> 39), both clamps (39 and 78) and deg in (-0.5, 0); the CoordLoss items
cover the rule firing each way, not firing for a low IoU, not firing because a hand has no valid entry, and a hand with a
single valid point (a zero-area box).  The seeds are searched so that, in the float64 run (asserted below): every deg is at
least 1e-2 away from a half-integer and from 39; every IoU at least 1e-3 from 0.5; the two hand depths differ by more than
1e-4 relative; no ``proj - gt`` lies within 1e-5 relative of 0, the planted exact tie aside.  ``dynamic_lmk_faces_idx[bin, 0]
= bin``, so the reference's selected faces name the bin it chose.
"""
import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import kpt_oracle as ko                 # noqa: E402

SMPLX = '/root/reference/fitting/common/utils/smplx/smplx/'
LOSS = '/root/reference/fitting/common/nets/loss.py'
V, NF, J, LS, LD, E, B = 30, 120, 8, 4, 5, 3, 6
DEGS = [0.3, 12.3, -7.3, 55.0, -50.0, -0.3]
WANT_BINS = [0, 12, 46, 39, 78, 0]
CB, CK = 6, 50


def cut(path, names, ns):
    src = open(path).read()
    lines = src.splitlines()
    for node in ast.parse(src).body:
        if isinstance(node, (ast.ClassDef, ast.FunctionDef)) and node.name in names:
            exec('\n'.join(lines[node.lineno - 1: node.end_lineno]), ns)


lhand, rhand, lwrist, rwrist = ko.HANDS
names = ['K%d' % k for k in range(CK)]
names[lwrist], names[rwrist] = 'L_Wrist', 'R_Wrist'
smpl_x = types.SimpleNamespace(kpt={'part_idx': {'lhand': lhand, 'rhand': rhand}, 'name': names})
ns = {'torch': torch, 'nn': nn, 'np': np, 'F': F, 'smpl_x': smpl_x, 'Tensor': torch.Tensor, 'Tuple': tuple, 'List': list,
      'Union': None, 'Array': np.ndarray}
import typing                                      # noqa: E402
ns.update({'Tuple': typing.Tuple, 'List': typing.List, 'Union': typing.Union})
cut(SMPLX + 'utils.py', ('rot_mat_to_euler', 'to_tensor'), ns)
cut(SMPLX + 'lbs.py', ('find_dynamic_lmk_idx_and_bcoords', 'vertices2landmarks', 'batch_rodrigues'), ns)
cut(SMPLX + 'vertex_joint_selector.py', ('VertexJointSelector',), ns)
cut(LOSS, ('CoordLoss',), ns)


def widen():
    """float64 run: FloatTensor builds float64."""
    saved = torch.FloatTensor
    torch.FloatTensor = lambda a: torch.tensor([float(x) for x in a], dtype=torch.float64)
    return saved


def layer_tail(c, pose, vertices, joints, vjs, dtype):
    """body_models.py:1257-1283 with the cut functions, then model.py:97-112; returns the tensors and the bins."""
    s = c['spec']
    Bn = vertices.shape[0]
    lmk_faces_idx = torch.from_numpy(s['lmk_f']).unsqueeze(dim=0).expand(Bn, -1).contiguous()
    lmk_bary_coords = torch.from_numpy(s['lmk_w']).to(dtype).unsqueeze(dim=0).repeat(Bn, 1, 1)
    dyn_lmk_faces_idx, dyn_lmk_bary_coords = ns['find_dynamic_lmk_idx_and_bcoords'](
        vertices, pose, torch.from_numpy(s['dyn_f']), torch.from_numpy(s['dyn_w']).to(dtype),
        torch.tensor(s['chain'], dtype=torch.long), pose2rot=True)
    lmk_faces_idx = torch.cat([lmk_faces_idx, dyn_lmk_faces_idx], 1)
    lmk_bary_coords = torch.cat([lmk_bary_coords.expand(Bn, -1, -1), dyn_lmk_bary_coords], 1)
    landmarks = ns['vertices2landmarks'](vertices, torch.from_numpy(s['faces']), lmk_faces_idx, lmk_bary_coords)
    full = vjs(vertices, joints)
    full = torch.cat([full, landmarks], dim=1)
    return full, lmk_faces_idx


def coord_tail(full, vertices, c, trans, focal, princpt, root_rel):
    s = c['spec']
    mesh_cam = vertices
    kpt_cam = full[:, torch.from_numpy(s['kpt_idx']), :]
    root_cam = full[:, int(s['root_idx']), :]
    mesh_cam = mesh_cam - root_cam[:, None, :] + trans[:, None, :]
    kpt_cam = kpt_cam - root_cam[:, None, :] + trans[:, None, :]
    x = kpt_cam[:, :, 0] / kpt_cam[:, :, 2] * focal[:, None, 0] + princpt[:, None, 0]
    y = kpt_cam[:, :, 1] / kpt_cam[:, :, 2] * focal[:, None, 1] + princpt[:, None, 1]
    kpt_proj = torch.stack((x, y), 2)
    if root_rel:
        mesh_cam = mesh_cam - trans[:, None, :]
        kpt_cam = kpt_cam - trans[:, None, :]
    return mesh_cam, kpt_cam, root_cam, kpt_proj


def layer_case(seed):
    rs = np.random.RandomState(seed)
    c = ko.kpt_case(seed, B, V, J, 20, LD, root='landmark')
    s = c['spec']
    s['faces'] = ko.faces_of(rs, V, NF)
    s['extra'], s['lmk_f'], s['lmk_w'] = s['extra'][:E], rs.randint(0, NF, LS), s['lmk_w'][:LS]
    s['dyn_f'] = rs.randint(0, NF, (ko.BINS, LD))
    s['dyn_f'][:, 0] = np.arange(ko.BINS)
    s['append'] = s['append'][:0]
    R = J + E + LS + LD
    s['kpt_idx'] = np.concatenate([rs.permutation(R), [J + E + LS, 0]]).astype(np.int64)      # every row, two of them twice
    s['root_idx'] = J + E + 1
    K = s['kpt_idx'].shape[0]
    pose = rs.randn(B, J, 3) * 0.02
    for b in range(B):
        pose[b, s['chain'][0]] = [0.0, -np.deg2rad(DEGS[b]), 0.0]
        pose[b, s['chain'][1:]] = rs.randn(len(s['chain']) - 1, 3) * 0.001
    c['pose'] = ko.f32(pose.reshape(B, J * 3))
    c.update(g_cam=ko.f32(rs.randn(B, K, 3)), g_proj=ko.f32(rs.randn(B, K, 2)))
    return c


def run_layer(c, dtype, root_rel):
    t = lambda a: torch.from_numpy(a).to(dtype)      # noqa: E731
    vertices, joints, trans = (t(c[k]).requires_grad_(True) for k in ('vertices', 'joints', 'trans'))
    vjs = ns['VertexJointSelector'](vertex_ids=VERTEX_IDS, use_hands=False, use_feet_keypoints=False)
    vjs.extra_joints_idxs = torch.from_numpy(c['spec']['extra'])
    full, faces_sel = layer_tail(c, t(c['pose']), vertices, joints, vjs, dtype)
    outs = coord_tail(full, vertices, c, trans, t(c['focal']), t(c['princpt']), root_rel)
    assert all(o.dtype == dtype for o in outs)
    cot = [t(c[k]) for k in ('g_mesh', 'g_cam', 'g_root', 'g_proj')]
    grads = torch.autograd.grad(outs, (vertices, joints, trans), cot)
    rot = ns['batch_rodrigues'](t(c['pose']).view(-1, 3)).view(B, J, 3, 3)
    rel = torch.eye(3, dtype=dtype).repeat(B, 1, 1)
    for j in c['spec']['chain']:
        rel = torch.bmm(rot[:, j], rel)
    deg = -ns['rot_mat_to_euler'](rel) * 180.0 / np.pi
    rec = {'joints_full': full, 'faces_sel': faces_sel, 'mesh_cam': outs[0], 'kpt_cam': outs[1], 'root_cam': outs[2],
           'kpt_proj': outs[3], 'd_vertices': grads[0], 'd_joints': grads[1], 'd_trans': grads[2], 'deg': deg, 'rot': rot}
    return {k: v.detach().numpy() for k, v in rec.items()}


def run_coord(c, dtype):
    t = lambda a: torch.from_numpy(a).to(dtype)      # noqa: E731
    m = ns['CoordLoss']()
    proj = t(c['proj']).requires_grad_(True)
    gt, valid, cam, weight = t(c['gt']), t(c['valid']), t(c['cam']), t(c['weight'])
    captured = []
    ones_like = torch.ones_like
    torch.ones_like = lambda *a, **k: captured.append(ones_like(*a, **k)) or captured[-1]
    try:
        loss = m(proj, gt, valid, cam)
    finally:
        torch.ones_like = ones_like
    assert loss.dtype == dtype
    weighted = loss * weight
    (grad,) = torch.autograd.grad(weighted, proj, t(c['g']))
    ious = np.full(CB, np.nan)
    for i in range(CB):
        vl, vr = valid[i, lhand, :], valid[i, rhand, :]
        if vl.sum() == 0 or vr.sum() == 0:
            continue
        with torch.no_grad():
            ious[i] = float(m.get_iou(m.get_bbox(proj[i, lhand, :], vl), m.get_bbox(proj[i, rhand, :], vr)))
    depths = torch.stack([cam[:, lhand, 2].mean(1), cam[:, rhand, 2].mean(1)], 1)
    return {'loss': loss.detach().numpy(), 'weighted': weighted.detach().numpy(), 'grad': grad.numpy(),
            'hand_w': captured[0][:, :, 0].numpy(), 'iou': ious, 'depths': depths.numpy()}


VERTEX_IDS = {k: 0 for k in ('nose', 'reye', 'leye', 'rear', 'lear')}
_cuda = torch.Tensor.cuda
torch.Tensor.cuda = lambda self, *a, **k: self.clone()
try:
    rec = {}
    for seed in range(500, 700):
        c = layer_case(seed)
        r64 = run_layer(c, torch.float64, False)
        if ko.deg_margin(r64['deg']).min() > 1e-2 and np.abs(r64['kpt_cam'][:, :, 2]).min() > 0.5 and \
                r64['faces_sel'][:, LS].tolist() == WANT_BINS and -0.5 < r64['deg'][5] < 0:
            break
    else:
        raise SystemExit('no clean layer seed')
    assert ko.deg_margin(r64['deg']).min() >= 1e-2, 'every deg at least 1e-2 from a half-integer and from 39'
    assert -0.5 < r64['deg'][5] < 0 and r64['faces_sel'][:, LS].tolist() == WANT_BINS, (r64['deg'], r64['faces_sel'][:, LS])
    r32 = run_layer(c, torch.float32, False)
    assert r32['faces_sel'][:, LS].tolist() == WANT_BINS
    s = c['spec']
    rec.update({'kpt_' + k: np.asarray(v) for k, v in s.items() if k not in ('V', 'J')})
    rec.update(kpt_V=np.int64(V), kpt_J=np.int64(J), kpt_seed=np.int64(seed), kpt_rot=r32['rot'])
    rec.update({'kpt_' + k: c[k] for k in ('vertices', 'joints', 'pose', 'trans', 'focal', 'princpt', 'g_cam', 'g_proj', 'g_root', 'g_mesh')})
    for tag, r in (('32', r32), ('64', r64), ('rel32', run_layer(c, torch.float32, True)), ('rel64', run_layer(c, torch.float64, True))):
        keep = ('kpt_cam', 'mesh_cam', 'd_trans') if tag.startswith('rel') else tuple(k for k in r if k != 'rot')      # root_rel changes these
        rec.update({'kpt_%s_%s' % (k, tag): r[k] for k in keep})
    print('layer: seed %d, deg %s' % (seed, np.round(r64['deg'], 3)))

    for seed in range(700, 900):
        c = ko.coord_case(seed, CB, CK)
        c['gt'][0, 7, 1] = c['proj'][0, 7, 1]                   # the planted exact tie
        saved = widen()
        try:
            q64 = run_coord(c, torch.float64)
        finally:
            torch.FloatTensor = saved
        d = c['proj'].astype(np.float64) - c['gt']
        tie = np.abs(d) <= 1e-5 * np.maximum(np.abs(c['proj']), np.abs(c['gt']))
        fired = q64['hand_w'].min(1) == 0
        ok = np.nanmin(np.abs(q64['iou'] - 0.5)) >= 1e-3 and tie.sum() == 1 and \
            (np.abs(q64['depths'][:, 0] - q64['depths'][:, 1]) > 1e-4 * np.abs(q64['depths']).max(1)).all()
        if ok:
            break
    else:
        raise SystemExit('no clean coord seed')
    assert np.nanmin(np.abs(q64['iou'] - 0.5)) >= 1e-3 and tie.sum() == 1 and tie[0, 7, 1]
    assert (np.abs(q64['depths'][:, 0] - q64['depths'][:, 1]) > 1e-4 * np.abs(q64['depths']).max(1)).all()
    lost_l, lost_r = q64['hand_w'][:, lhand[0]] == 0, q64['hand_w'][:, rhand[0]] == 0
    assert lost_l[0] and lost_r[1] and not fired[2] and q64['iou'][2] < 0.5, 'fires each way, not for a low IoU'
    assert np.isnan(q64['iou'][3]) and not fired[3], 'a hand without a valid entry: skipped'
    assert q64['iou'][4] == 0 and not fired[4], 'a single valid point: a zero-area box'
    q32 = run_coord(c, torch.float32)
    assert np.array_equal(q32['hand_w'], q64['hand_w'])
    rec.update({'coord_' + k: v for k, v in c.items()})
    rec.update(coord_lhand=np.array(lhand), coord_rhand=np.array(rhand), coord_wrists=np.array([lwrist, rwrist]),
               coord_seed=np.int64(seed))
    for tag, q in (('32', q32), ('64', q64)):
        rec.update({'coord_%s_%s' % (k, tag): v for k, v in q.items()})
    print('coord: seed %d, iou %s' % (seed, np.round(q64['iou'], 3)))
finally:
    torch.Tensor.cuda = _cuda

for name in ('kpt_cam', 'kpt_proj', 'mesh_cam', 'd_vertices', 'd_joints', 'd_trans'):
    e = np.abs(rec['kpt_%s_32' % name] - rec['kpt_%s_64' % name]).max()
    print('%-10s reference float32 error %.3e (max |value| %.3e)' % (name, e, np.abs(rec['kpt_%s_64' % name]).max()))
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ref_keypoints.npz')
np.savez_compressed(path, **rec)
print('wrote', path, os.path.getsize(path), 'bytes')
assert os.path.getsize(path) < 100_000
