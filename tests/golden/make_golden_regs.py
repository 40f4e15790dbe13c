"""Generates tests/golden/ref_regs.npz by EXECUTING the reference's own ``ArmRGBReg``, ``HandRGBReg`` and ``HandMeanReg``.

``/root/reference/avatar/common/nets/loss.py`` cannot be imported as a module here (it imports lpips, pytorch3d and the
training config at the top), so the source text of the three classes is cut out of the file with ``ast`` and exec'd
unchanged in a namespace holding torch / nn / F, the ``Meshes`` stand-in and a ``smpl_x`` namespace with
``face_upsampled`` and ``vertex_num_upsampled``; ``Tensor.cuda()`` is a no-op for the duration (this container has no
GPU).  Run from the repo root:  python tests/golden/make_golden_regs.py
Nothing here is read at test time on the GPU box -- only the .npz travels.

Arm cases (tests/reg_oracle.py ``two_tube_arms``; B = 2; every run in float32 and, on the same numbers, in float64):
  a   10 rings x 20: V 437, U 140, L 260, n_l 21 .. 35, so k = 21 < 50.
  b   12 rings x 64: V 1573, U 504, L 1032, n_l 63 .. 105, so k = 50.
  c   case a plus a threshold probe around x = 0: one upper vertex u* at the origin, five lower vertices on the x axis at
      |x| = nextafter(0.01f, 0) (one on either side), nextafter(0.01f, inf) (one on either side) and 0.01f exactly, and
      60 more upper vertices around either side so that the five have partners enough.  u* is the nearest upper vertex
      of all five, so it is in the target exactly where the pair is valid.  The float64 run compares the exact one with
      the DOUBLE 0.01 and so takes u* where the float32 run does not: that row is left out of the float64 comparison.
  d   case b plus three duplicated upper positions with colours of their own, each the 50th neighbour of one lower
      vertex: an exact tie between its k-th and (k+1)-th key, which ``topk`` may break either way.  Those three rows are
      compared with the oracle alone; the script asserts that they are the only rows tied and that every other row of
      every case has its k-th and (k+1)-th float64 distances more than 1e-5 apart, relatively.
Hand case: a bumpy 9 x 11 grid, two disjoint masks of 17 vertices; one offset row exactly 0, one of norm 1e-13, one
pointing against its normal.
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import reg_oracle as ro                                     # noqa: E402
from exavatar_release_amd.p3d_standins import Meshes        # noqa: E402

REF = '/root/reference/avatar/common/nets/loss.py'
src = open(REF).read()
smpl_x = types.SimpleNamespace(face_upsampled=None, vertex_num_upsampled=0)
ns = {'torch': torch, 'nn': nn, 'F': F, 'np': np, 'Meshes': Meshes, 'smpl_x': smpl_x}
lines = src.splitlines()
for node in ast.parse(src).body:
    if isinstance(node, ast.ClassDef) and node.name in ('ArmRGBReg', 'HandRGBReg', 'HandMeanReg'):
        exec('\n'.join(lines[node.lineno - 1: node.end_lineno]), ns)

B = 2


def kth_gap(mesh, is_upper, is_lower, k):
    """Per lower row: (relative gap between the k-th and (k+1)-th valid float64 distance, inf without a (k+1)-th;
    whether their float32 d2 are the same bits)."""
    plan = ro.arm_plan32(mesh, is_upper, is_lower, top_k=k + 1)
    m = mesh.astype(np.float64)
    gaps, tied = [], []
    for row, l in enumerate(plan['lower']):
        a, b = plan['nbr'][row, k - 1], plan['nbr'][row, k]
        if b < 0:
            gaps.append(np.inf)
            tied.append(False)
            continue
        da, db = np.linalg.norm(m[l] - m[a]), np.linalg.norm(m[l] - m[b])
        gaps.append(abs(db - da) / da)
        d32 = [((mesh[l] - mesh[j]) ** 2) for j in (a, b)]
        tied.append(np.float32(np.float32(d32[0][0] + d32[0][1]) + d32[0][2])
                    == np.float32(np.float32(d32[1][0] + d32[1][1]) + d32[1][2]))
    return np.array(gaps), np.array(tied)


def run_arm(mesh, is_upper, is_lower, rgb, G, dtype):
    smpl_x.vertex_num_upsampled = mesh.shape[0]
    x = torch.from_numpy(rgb).to(dtype).requires_grad_(True)
    loss = ns['ArmRGBReg']()(torch.from_numpy(mesh).to(dtype), torch.from_numpy(is_upper), torch.from_numpy(is_lower), x)
    (loss * torch.from_numpy(G).to(dtype)).sum().backward()
    return loss.detach().numpy(), x.grad.numpy()


def arm_case(name, mesh, is_upper, is_lower, seed, rec, f64_skip=(), expect_tied=0):
    rng = np.random.RandomState(seed)
    V, L = mesh.shape[0], int(is_lower.sum())
    rgb = rng.uniform(0, 1, size=(B, V, 3)).astype(np.float32)
    G = rng.standard_normal((B, L, 3)).astype(np.float32)
    plan = ro.arm_plan32(mesh, is_upper, is_lower)
    k = plan['k']
    gaps, tied = kth_gap(mesh, is_upper, is_lower, k)
    tied_rows = np.nonzero(tied)[0]
    assert tied_rows.size == expect_tied, (name, tied_rows)
    assert (gaps[~tied] > 1e-5).all(), (name, gaps[~tied].min())
    loss32, grad32 = run_arm(mesh, is_upper, is_lower, rgb, G, torch.float32)
    loss64, grad64 = run_arm(mesh, is_upper, is_lower, rgb, G, torch.float64)
    # the oracle agrees with the reference's float32 run on every untied row (tests/test_reg_oracle.py repeats this)
    o_loss, o_d = ro.arm_loss32(plan, rgb)
    b64 = ro.arm_forward64(plan, rgb)
    keep = np.ones(L, dtype=bool)
    keep[tied_rows] = False
    err = np.abs(o_loss[:, plan['lower']].astype(np.float64) - loss32)[:, keep]
    assert (err <= 2 * b64['E_loss'][:, keep]).all(), (name, err.max())
    k64 = np.ones(L, dtype=bool)
    k64[tied_rows] = False
    k64[list(f64_skip)] = False
    assert (np.abs(loss32 - loss64)[:, k64] <= b64['E_loss'][:, k64]).all(), name
    rec.update({name + '_mesh': mesh, name + '_is_upper': is_upper, name + '_is_lower': is_lower, name + '_rgb': rgb,
                name + '_G': G, name + '_loss32': loss32, name + '_grad32': grad32, name + '_loss64': loss64,
                name + '_grad64': grad64, name + '_k': np.int64(k), name + '_n_valid': plan['n_valid'],
                name + '_tied_rows': tied_rows.astype(np.int64), name + '_f64_skip': np.array(list(f64_skip), dtype=np.int64)})
    print('%s: V %d U %d L %d n_l %d..%d k %d tied rows %s max |oracle - ref32| %.2e' % (
        name, V, int(is_upper.sum()), L, plan['n_valid'].min(), plan['n_valid'].max(), k, tied_rows.tolist(), err.max()))
    return plan


_cuda = torch.Tensor.cuda
torch.Tensor.cuda = lambda self, *a, **k: self
try:
    rec = {}
    # ---- a, b
    mesh_a, up_a, lo_a = ro.two_tube_arms(10, 20, seed=12)
    plan_a = arm_case('a', mesh_a, up_a, lo_a, 101, rec)
    assert (mesh_a.shape[0], int(up_a.sum()), int(lo_a.sum()), plan_a['k']) == (437, 140, 260, 21)
    assert (plan_a['n_valid'].min(), plan_a['n_valid'].max()) == (21, 35)
    mesh_b, up_b, lo_b = ro.two_tube_arms(12, 64, seed=57)
    plan_b = arm_case('b', mesh_b, up_b, lo_b, 102, rec)
    assert (mesh_b.shape[0], int(up_b.sum()), int(lo_b.sum()), plan_b['k']) == (1573, 504, 1032, 50)
    assert (plan_b['n_valid'].min(), plan_b['n_valid'].max()) == (63, 105)

    # ---- c: the threshold probe
    thr = np.float32(0.01)
    below, above = np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(np.inf))
    assert below < thr < above
    rng = np.random.RandomState(13)
    probes = np.array([[below, 0, 0], [-below, 0, 0], [above, 0, 0], [-above, 0, 0], [thr, 0, 0]], dtype=np.float32)
    ang = rng.uniform(0, 2 * np.pi, 120)
    side = np.repeat([1.0, -1.0], 60)
    cluster = np.stack([side * (0.005 + rng.uniform(-1e-3, 1e-3, 120)), 0.03 * np.sin(ang), 0.03 * np.cos(ang)], 1)
    mesh_c = np.concatenate([mesh_a, np.zeros((1, 3)), cluster, probes]).astype(np.float32)
    n0 = mesh_a.shape[0]
    up_c = np.concatenate([up_a, np.ones(121, dtype=bool), np.zeros(5, dtype=bool)])
    lo_c = np.concatenate([lo_a, np.zeros(121, dtype=bool), np.ones(5, dtype=bool)])
    L_c = int(lo_c.sum())
    probe_rows = np.arange(L_c - 5, L_c)
    plan_c = arm_case('c', mesh_c, up_c, lo_c, 103, rec, f64_skip=[L_c - 1])
    assert plan_c['k'] == 21
    has_ustar = (plan_c['nbr'][probe_rows, :21] == n0).any(1)
    assert plan_c['n_valid'][probe_rows].tolist() == [61, 61, 60, 60, 60] and has_ustar.tolist() == [1, 1, 0, 0, 0]
    assert (plan_c['nbr'][probe_rows[:2], 0] == n0).all(), 'u* is the nearest partner where the pair is valid'
    rec['c_probe_rows'] = probe_rows.astype(np.int64)
    rec['c_ustar'] = np.int64(n0)

    # ---- d: three exact ties at the k-th key
    mesh_d, up_d, lo_d = mesh_b.copy(), up_b.copy(), lo_b.copy()
    k = 50
    chosen = []
    for row in np.random.RandomState(14).permutation(int(lo_b.sum())):
        plan = ro.arm_plan32(mesh_d, up_d, lo_d)
        u_k = plan['nbr'][row, k - 1]
        m2 = np.concatenate([mesh_d, mesh_d[u_k][None]])
        u2, l2 = np.append(up_d, True), np.append(lo_d, False)
        gaps, tied = kth_gap(m2, u2, l2, k)
        if np.nonzero(tied)[0].tolist() == sorted(chosen + [int(row)]) and (gaps[~tied] > 1e-5).all():
            mesh_d, up_d, lo_d = m2, u2, l2
            chosen.append(int(row))
        if len(chosen) == 3:
            break
    assert len(chosen) == 3
    plan_d = arm_case('d', mesh_d, up_d, lo_d, 104, rec, expect_tied=3)
    assert plan_d['k'] == 50 and sorted(rec['d_tied_rows'].tolist()) == sorted(chosen)
    for row in chosen:       # the duplicate is the later index: the oracle takes the original and leaves the duplicate out
        a, b = plan_d['nbr'][row, k - 1], ro.arm_plan32(mesh_d, up_d, lo_d, top_k=k + 1)['nbr'][row, k]
        assert (mesh_d[a] == mesh_d[b]).all() and a < b and not np.array_equal(rec['d_rgb'][:, a], rec['d_rgb'][:, b])

    # ---- the hands
    ROWS, COLS = 9, 11
    V = ROWS * COLS
    rng = np.random.RandomState(15)
    yy, xx = np.meshgrid(np.arange(ROWS), np.arange(COLS), indexing='ij')
    verts = np.stack([xx.reshape(-1) * 0.01, yy.reshape(-1) * 0.01, rng.uniform(-4e-3, 4e-3, V)], 1).astype(np.float32)
    face = ro.grid_faces(ROWS, COLS)
    perm = rng.permutation(V)
    is_r, is_l = np.zeros(V, dtype=bool), np.zeros(V, dtype=bool)
    is_r[perm[:17]] = True
    is_l[perm[17:34]] = True
    smpl_x.face_upsampled, smpl_x.vertex_num_upsampled = face, V
    normal = Meshes(verts=torch.from_numpy(verts)[None], faces=torch.from_numpy(face)[None]).verts_normals_packed().numpy()
    hand = np.nonzero(is_r | is_l)[0]
    offset = (rng.standard_normal((B, V, 3)) * 0.01).astype(np.float32)
    offset[0, hand[3]] = 0.0
    offset[1, hand[5]] = (np.array([0.6, 0.0, 0.8]) * 1e-13).astype(np.float32)
    offset[0, hand[7]] = -0.01 * normal[hand[7]]
    rgb = rng.uniform(0, 1, size=(B, V, 3)).astype(np.float32)
    G_rgb = rng.standard_normal((B, 17, 3)).astype(np.float32)
    G_mean = rng.standard_normal((B, hand.size)).astype(np.float32)
    rec.update(h_verts=verts, h_face=face, h_is_rhand=is_r, h_is_lhand=is_l, h_normal=normal, h_offset=offset, h_rgb=rgb,
               h_G_rgb=G_rgb, h_G_mean=G_mean)
    for tag, dtype in (('32', torch.float32), ('64', torch.float64)):
        x = torch.from_numpy(rgb).to(dtype).requires_grad_(True)
        loss = ns['HandRGBReg']()(x, torch.from_numpy(is_r), torch.from_numpy(is_l))
        (loss * torch.from_numpy(G_rgb).to(dtype)).sum().backward()
        rec['h_rgb_loss' + tag], rec['h_rgb_grad' + tag] = loss.detach().numpy(), x.grad.numpy()
        o = torch.from_numpy(offset).to(dtype).requires_grad_(True)
        loss = ns['HandMeanReg']()(torch.from_numpy(verts).to(dtype), o, torch.from_numpy(is_r), torch.from_numpy(is_l))
        (loss * torch.from_numpy(G_mean).to(dtype)).sum().backward()
        rec['h_mean_loss' + tag], rec['h_mean_grad' + tag] = loss.detach().numpy(), o.grad.numpy()
    j0, j1, j2 = 3, 5, 7
    assert rec['h_mean_loss32'][0, j0] == 0 and np.isfinite(rec['h_mean_grad32']).all()
    assert np.abs(rec['h_mean_grad32'][0, hand[j0]]).max() > 1e10, 'the zero row passes g * n / eps'
    assert rec['h_mean_loss32'][0, j2] == 0 and (rec['h_mean_grad32'][0, hand[j2]] == 0).all(), 'the clamped row'
    assert 0 < np.abs(rec['h_mean_loss32'][1, j1]) < 0.2, 'the 1e-13 row is divided by eps, not by its norm'
finally:
    torch.Tensor.cuda = _cuda
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ref_regs.npz')
np.savez_compressed(path, **rec)
print('wrote', path, os.path.getsize(path), 'bytes')
