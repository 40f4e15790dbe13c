"""Generates tests/golden/ref_lossblock_w0.npz and ref_lossblock_w1.npz by EXECUTING the reference's own loss block.

The training branch of ``Model.forward`` (reference ``avatar/main/model.py:191-258``) composes what the HIP loss modules
of this package replace.  ``model.py`` and ``loss.py`` cannot be imported here (lpips, pytorch3d, the training config),
so the classes ``RGBLoss``, ``SSIM``, ``LaplacianReg``, ``JointOffsetSymmetricReg``, ``HandMeanReg``, ``HandRGBReg`` and
``ArmRGBReg`` of ``loss.py``, ``get_arm`` of ``utils/smpl_x.py`` and the body of ``if mode == 'train':`` of
``Model.forward`` are cut out of the files with ``ast`` and exec'd UNCHANGED; the block is re-indented under a ``def``
header of this file that names the variables it reads.  The namespace holds ``torch``, ``F``, ``math``, ``np``, the
``Meshes`` stand-in and stub ``smpl_x`` / ``cfg`` objects; ``self.lpips`` is a stub that returns zeros ``[B, 1, 1, 1]`` and
the two LPIPS terms are dropped (no weights at hand).  ``Tensor.cuda()`` is the identity for the duration.  In the
float64 run ``SSIM.create_window`` is followed by a cast: the window is the reference's float32 window in either run,
as the HIP kernel builds it.

The block runs on the CPU in float64 and in float32 on the case of ``tests/loss_case.py``, for ``cfg.is_warmup`` False
(``_w0``) and True (``_w1``).  Each file holds: every term's ``.mean()`` (train.py:43) and their sum in float64
(``term/NAME``, ``total``), the float32 run's (``#f32``) and the per-element part of the term's rounding scale
(``#elem``, see ``element_errors``); the float64 gradient of the total to every leaf -- of a large one the entries
``loss_case.sample_index`` names -- with the full tensor's norm (``#norm``) and the relative L2 / norm-scaled max error of
the reference's own float32 run over the stored entries (``#rel_l2``, ``#rel_max``, as ``ref_human.npz`` defines them);
the leaves no gradient reaches; the arm masks, ``k``, ``n_valid``, the case's margins and a SHA-256 of every input.
Only results and digests are written -- nothing of the reference's text.

    python tests/golden/make_golden_lossblock.py --reference PATH_TO_EXAVATAR_RELEASE
"""
import argparse
import ast
import math
import os
import sys
import textwrap
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from exavatar_release_amd.p3d_standins import Meshes      # noqa: E402
from tests import loss_case as lc                         # noqa: E402
from tests import reg_oracle as ro                        # noqa: E402

CLASSES = ('RGBLoss', 'SSIM', 'LaplacianReg', 'JointOffsetSymmetricReg', 'HandMeanReg', 'HandRGBReg', 'ArmRGBReg')
HEADER = ('def loss_block(self, data, mode, bg, mesh_neutral_pose, scene_renders, human_renders, scene_human_renders,\n'
          '               human_renders_refined, scene_human_renders_refined, face_renders, face_renders_refined,\n'
          '               human_assets, human_assets_refined, human_offsets):\n')
U = 2.0 ** -24


def _assigns(node, name):
    return isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in node.targets)


def reference_namespace(ref_root):
    """The namespace the cut code runs in, with the cut classes, ``smpl_x.get_arm`` and ``loss_block`` defined."""
    common = os.path.join(ref_root, 'avatar', 'common')
    smpl_x = types.SimpleNamespace(face_upsampled=None, vertex_num_upsampled=lc.V, joint_num=lc.J,
                                   joints_name=lc.JOINTS_NAME, joint_part=lc.JOINT_PART, joint_offset=None)
    cfg = types.SimpleNamespace(rgb_loss_weight=lc.W_RGB, ssim_loss_weight=lc.W_SSIM, lpips_weight=lc.W_LPIPS,
                                fit_pose_to_test=False, is_warmup=False)
    ns = {'torch': torch, 'nn': nn, 'F': F, 'math': math, 'np': np, 'Meshes': Meshes, 'smpl_x': smpl_x, 'cfg': cfg}
    src = open(os.path.join(common, 'nets', 'loss.py')).read()
    lines = src.splitlines()
    found = []
    for node in ast.parse(src).body:
        if isinstance(node, ast.ClassDef) and node.name in CLASSES:
            exec('\n'.join(lines[node.lineno - 1:node.end_lineno]), ns)
            found.append(node.name)
    assert sorted(found) == sorted(CLASSES), found
    # get_arm: a method of class SMPLX
    src = open(os.path.join(common, 'utils', 'smpl_x.py')).read()
    lines = src.splitlines()
    fn = [n for c in ast.parse(src).body if isinstance(c, ast.ClassDef) for n in c.body
          if isinstance(n, ast.FunctionDef) and n.name == 'get_arm']
    assert len(fn) == 1
    exec(textwrap.dedent('\n'.join(lines[fn[0].lineno - 1:fn[0].end_lineno])), ns)
    smpl_x.get_arm = types.MethodType(ns.pop('get_arm'), smpl_x)
    # the training branch of Model.forward that assembles ``loss``
    src = open(os.path.join(ref_root, 'avatar', 'main', 'model.py')).read()
    lines = src.splitlines()
    fwd = [n for c in ast.parse(src).body if isinstance(c, ast.ClassDef) and c.name == 'Model' for n in c.body
           if isinstance(n, ast.FunctionDef) and n.name == 'forward'][0]
    branch = [n for n in ast.walk(fwd) if isinstance(n, ast.If) and isinstance(n.test, ast.Compare)
              and ast.unparse(n.test) == "mode == 'train'" and any(_assigns(s, 'loss') for s in n.body)]
    assert len(branch) == 1
    body = textwrap.dedent('\n'.join(lines[branch[0].body[0].lineno - 1:branch[0].body[-1].end_lineno]))
    exec(HEADER + textwrap.indent(body, '    '), ns)
    return ns


def reference_model(ns, case, dtype):
    """(self, leaves, the keyword arguments of ``loss_block`` but the assets): the case in ``dtype``."""
    t = lambda k: torch.from_numpy(np.array(case[k]))      # noqa: E731
    f = lambda k: t(k).to(dtype)                           # noqa: E731
    smpl_x = ns['smpl_x']
    smpl_x.face_upsampled = np.array(case['face_upsampled'])
    smpl_x.joint_offset = f('joint_offset_ref')
    leaves = {k: f(k).requires_grad_(True) for k in lc.LEAVES}
    consts = {k: f(k) for k in ('face_alpha', 'face_refined_alpha')}

    class SSIM(ns['SSIM']):
        def create_window(self, window_size, feat_dim):
            return super().create_window(window_size, feat_dim).to(dtype)
    B = lc.B
    self = types.SimpleNamespace(
        rgb_loss=ns['RGBLoss'](), ssim=SSIM(), lpips=lambda *a, **k: torch.zeros((B, 1, 1, 1), dtype=dtype),
        lap_reg=ns['LaplacianReg'](lc.V, smpl_x.face_upsampled), joint_offset_sym_reg=ns['JointOffsetSymmetricReg'](),
        hand_mean_reg=ns['HandMeanReg'](), hand_rgb_reg=ns['HandRGBReg'](), arm_rgb_reg=ns['ArmRGBReg'](),
        human_gaussian=types.SimpleNamespace(skinning_weight=f('skinning_weight'), joint_offset=leaves['joint_offset'],
                                             **{k: t(k) for k in lc.MASKS}))
    args = dict(self=self, data={'img': f('img'), 'mask': f('mask'), 'bbox': f('bbox')}, mode='train', bg=f('bg'),
                mesh_neutral_pose=f('mesh_neutral_pose'),
                scene_renders={'img': leaves['scene'], 'mean_2d': [], 'is_vis': torch.zeros(1), 'radius': torch.zeros(1)},
                human_renders={'img': leaves['human']}, scene_human_renders={'img': leaves['scene_human']},
                human_renders_refined={'img': leaves['human_refined']},
                scene_human_renders_refined={'img': leaves['scene_human_refined']},
                face_renders=lc.face_render(leaves, consts, ''), face_renders_refined=lc.face_render(leaves, consts, '_refined'),
                human_offsets={k: leaves[k] for k in ('mean_offset', 'mean_offset_offset', 'scale_offset', 'rgb_offset')})
    return self, leaves, args


def run(ns, case, dtype, is_warmup):
    """One forward + backward of the reference's block: (maps name -> the term before its mean, means, total, gradients
    leaf -> tensor or None, the arm masks)."""
    ns['cfg'].is_warmup = is_warmup
    self, leaves, args = reference_model(ns, case, dtype)
    args['human_assets'], args['human_assets_refined'] = lc.gather_assets(leaves, is_warmup)
    _, maps = ns['loss_block'](**args)
    assert not float(maps['lpips_human'].abs().sum()) and not float(maps['lpips_human_refined'].abs().sum())
    maps = {k: v for k, v in maps.items() if not k.startswith('lpips')}
    assert tuple(maps) == lc.DROPIN_TERMS, tuple(maps)
    means = {k: v.mean() for k, v in maps.items()}                                    # train.py:43
    total = sum(means[k] for k in means)                                              # train.py:46
    grads = torch.autograd.grad(total, list(leaves.values()), allow_unused=True)
    arm = ns['smpl_x'].get_arm(args['mesh_neutral_pose'], self.human_gaussian.skinning_weight)
    return maps, means, total, dict(zip(leaves, grads)), arm


def ssim_error(ns, x, y, mask, crop):
    """Float64 bound on the error a float32 evaluation commits on every element of the SSIM map:
    each of the five statistics is a 121-term convex combination of values (or products) of magnitude <= 1, accumulated
    in float32: 121 products and 121 additions, each rounded at a magnitude <= 1, sqrt(242) < 16 in the root sum square
    (17 with the mask's product in front); the map's own formula propagates them to first order and adds 8 roundings."""
    delta = (17 if mask is not None else 16) * U
    if mask is not None:
        x, y = x * mask, y * mask
    if crop is not None:
        x0, y0, w, h = crop
        x, y = x[:, :, y0:y0 + h, x0:x0 + w], y[:, :, y0:y0 + h, x0:x0 + w]
    win = ns['SSIM']().create_window(11, 3).double()
    conv = lambda a: F.conv2d(a, win, padding=5, groups=3)      # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    s11, s22, s12 = conv(x * x) - mu1 ** 2, conv(y * y) - mu2 ** 2, conv(x * y) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    A1, A2, B1, B2 = 2 * mu1 * mu2 + C1, 2 * s12 + C2, mu1 ** 2 + mu2 ** 2 + C1, s11 + s22 + C2
    s = A1 * A2 / (B1 * B2)
    m = mu1.abs() + mu2.abs()
    ds = 2 * delta * m * (A2.abs() / (B1 * B2) + s.abs() / B1) + 2 * delta * (1 + m) * (A1.abs() / (B1 * B2) + s.abs() / B2)
    return (ds + 8 * U * s.abs()).numpy()


def element_errors(ns, case, maps, is_warmup):
    """name -> float64 array shaped like the term's map: a first-order bound on the error one float32 evaluation commits
    on each element, from the modules' stated arithmetic (``include/exa_raster.h``, ``include/exa_mesh.h``) and the
    float64 values.  DESIGN.md section 8p derives every line."""
    c = {k: torch.from_numpy(np.array(v)).double() for k, v in case.items() if v.dtype == np.float32}
    t = {k: v.detach().abs().numpy() for k, v in maps.items()}
    ones = torch.ones((1, lc.V, 1), dtype=torch.float64)
    wt = {k: v.numpy() for k, v in lc.vertex_weights({k: torch.from_numpy(np.array(case[k])) for k in lc.MASKS}, ones).items()}
    e = {}
    for tag in ('', '_refined'):
        e['rgb_human' + tag] = 2 * U * t['rgb_human' + tag]                       # x - y, * 0.8
        e['rgb_face' + tag] = 2 * U * t['rgb_face' + tag]                         # the composite is exact (is_face is 0 / 1)
        # target = img * mask + (1 - mask) * bg: four roundings at a magnitude <= 1, then x - target
        e['rgb_human%s_rand_bg' % tag] = U * (4 + t['rgb_human%s_rand_bg' % tag])
        e['ssim_human' + tag] = lc.W_SSIM * ssim_error(ns, c['scene_human' + tag], c['img'], None, lc.CROP) \
            + 2 * U * t['ssim_human' + tag]                                       # 1 - s, * 0.2
    # |x - y| (1 - mask) 0.8: three roundings of the product and (1 - mask) rounded at magnitude 1
    e['rgb_scene'] = U * (3 * t['rgb_scene'] + lc.W_RGB * (c['scene'] - c['img']).abs().numpy())
    e['ssim_scene'] = lc.W_SSIM * ssim_error(ns, c['scene'], c['img'], 1 - c['mask'], None) + 2 * U * t['ssim_scene']
    e['gaussian_mean_reg'] = 4 * U * t['gaussian_mean_reg']                       # two squares, one sum, one product
    e['gaussian_scale_reg'] = 4 * U * t['gaussian_scale_reg']
    # two dot products of unit vectors: a float32 vertex normal (about 10 roundings at magnitude 1), the normalised
    # offset (4), three products and two sums (5) each -- at magnitude 1 whatever the dot product is -- and their sum
    e['gaussian_mean_hand_reg'] = U * (2 * 20 + t['gaussian_mean_hand_reg'])
    # t = K w (d1^2 + d2^2): |dt| <= 2 sqrt(2 K w t) dd + 5 U t, with dd the error of one Laplacian difference:
    # lap(x) = x + sum of 10 products, 20 roundings at the magnitude M of x, sqrt(20) < 5 in the root sum square
    mesh_M = c['mesh_neutral_pose'].abs().amax(0) + c['mean_offset'].abs().amax() + c['mean_offset_offset'].abs().amax()
    scale_M = max(float(c['scale_raw'].max()), float(c['scale_refined_raw'].max()))
    for name, K, dd in (('lap_mean', 100000, (8 * U * mesh_M).numpy()[None, None, :]),      # two Laplacians and x = mesh + offsets
                        ('lap_scale', 100000, 5 * U * scale_M), ('lap_rgb', 1, 5 * U * 1.0)):
        e[name] = 2 * np.sqrt(2 * K * wt[name] * t[name]) * dd + 5 * U * t[name]
    # t = 0.01 (dr^2 + dl^2), d = rgb - mean over 301 rows in chunks of 256 (0.5 sqrt(256 / 3) < 5 roundings), the difference 1
    e['hand_rgb_reg'] = 2 * np.sqrt(2 * 0.01 * t['hand_rgb_reg']) * 6 * U + 4 * U * t['hand_rgb_reg']
    # t = 0.1 (d1^2 + d2^2), d = rgb - mean over k = 21 rows summed in order (0.5 sqrt(21 / 3) < 2), the difference 1
    e['arm_rgb_reg'] = 2 * np.sqrt(2 * 0.1 * t['arm_rgb_reg']) * 3 * U + 4 * U * t['arm_rgb_reg']
    e['joint_offset_reg'] = 4 * U * t['joint_offset_reg']                         # difference, square, product (and the weight)
    e['joint_offset_sym_reg'] = 3 * U * t['joint_offset_sym_reg']                 # three |a +- b| and two sums
    assert sorted(e) == sorted(maps)
    return {k: np.broadcast_to(v, maps[k].shape) for k, v in e.items()}


def stored(name, leaf, a64, a32=None):
    a64 = a64.detach().double().numpy()
    s64 = lc.take_sample(leaf, a64)
    out = {name: s64, name + '#norm': np.float64(np.linalg.norm(a64))}
    if a32 is not None:
        err = lc.take_sample(leaf, a32.detach().double().numpy()) - s64
        n = np.linalg.norm(s64)
        out[name + '#rel_l2'] = np.float64(np.linalg.norm(err) / n) if n > 0 else np.float64(0)
        out[name + '#rel_max'] = np.float64(np.abs(err).max() * np.sqrt(err.size) / n) if n > 0 else np.float64(0)
    return out


def record(ref_root, is_warmup, with_float32=True):
    """Every entry of one fixture file (name -> numpy).  ``with_float32=False``: the float64 values alone."""
    ns = reference_namespace(ref_root)
    case = lc.build_case()
    mg = lc.margins(case)
    lc.check_margins(mg)
    out = {}
    threads = torch.get_num_threads()
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.set_num_threads(1)
    try:
        maps, means, total, g64, arm = run(ns, case, torch.float64, is_warmup)
        elem = element_errors(ns, case, maps, is_warmup)
        for k in maps:
            out['term/' + k] = np.float64(means[k].item())
            out['term/%s#elem' % k] = np.float64(np.sqrt((elem[k].astype(np.float64) ** 2).sum()) / elem[k].size)
        out['total'] = np.float64(total.item())
        up, lo = (a.numpy().astype(bool) for a in arm)
        up_np, lo_np = lc.arm_masks(case, lc.normals64(case))
        assert np.array_equal(up, up_np) and np.array_equal(lo, lo_np)
        plan = ro.arm_plan32(case['mesh_neutral_pose'], up, lo)
        assert plan['k'] == lc.K_ARM and (plan['n_valid'].min(), plan['n_valid'].max()) == lc.N_VALID
        out.update({'arm/is_upper': up, 'arm/is_lower': lo, 'arm/k': np.int64(plan['k']),
                    'arm/n_valid': plan['n_valid'].astype(np.int32)})
        g32 = None
        if with_float32:
            _, means32, total32, g32, arm32 = run(ns, case, torch.float32, is_warmup)
            assert all(torch.equal(a, b) for a, b in zip(arm, arm32)), 'the float32 run of the reference finds other arms'
            for k in maps:
                out['term/%s#f32' % k] = np.float64(means32[k].item())
            out['total#f32'] = np.float64(total32.item())
            # the derived scales hold the reference's own float32 run (if not, the derivation is wrong, not the factor)
            for variant, names in (('dropin', lc.DROPIN_TERMS + ('total',)), ('fused', tuple(lc.FUSED_PAIRS))):
                for k in names:
                    got = out['total#f32'] if k == 'total' else sum(out['term/%s#f32' % p] for p in lc.FUSED_PAIRS.get(k, (k,)))
                    want, scale = lc.term_value(out, k), lc.term_scale(out, variant, k)
                    print('w%d %-7s %-28s %.9e  float32 off by %5.2f scales (%.2e)' % (
                        is_warmup, variant, k, want, abs(got - want) / scale, scale))
                    assert abs(got - want) <= lc.FACTOR * scale, (k, got, want, scale)
        unreached = [k for k, g in g64.items() if g is None or not bool(g.any())]
        out['unreached'] = np.array(unreached if unreached else [''])
        for k, g in g64.items():
            if k not in unreached:
                out.update(stored('grad/' + k, k, g, None if g32 is None else g32[k]))
    finally:
        torch.Tensor.cuda = orig_cuda
        torch.set_num_threads(threads)
    for k, v in mg.items():
        out['margin/' + k] = np.float64(v)
    for k, d in lc.digests(case).items():
        out['sha256/' + k] = np.array(d)
    return out


def path_of(is_warmup):
    return os.path.join(HERE, 'ref_lossblock_w%d.npz' % int(is_warmup))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the ExAvatar_RELEASE checkout')
    args = ap.parse_args()
    for is_warmup in (False, True):
        out = record(args.reference, is_warmup)
        np.savez_compressed(path_of(is_warmup), **out)
        size = os.path.getsize(path_of(is_warmup))
        assert size < (1 << 20), size
        worst = max((float(v), k) for k, v in out.items() if k.endswith('#rel_l2'))
        print(path_of(is_warmup), size, 'bytes; unreached %s; largest float32 rel L2 error %.3e (%s)' % (
            [str(s) for s in out['unreached']], worst[0], worst[1]))


if __name__ == '__main__':
    main()
