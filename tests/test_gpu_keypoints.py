"""The keypoint path on the device: ``BodyKeypoints`` and ``CoordLoss`` against their CPU restatement (tests/kpt_oracle.py) BIT FOR
BIT, values and every gradient, at the sizes where the kernels' work split changes (K around the 64 lanes of a wave and the
256 threads of a workgroup, V around 256); against the reference's expressions run by torch on the same device; against the
reference's own run (tests/golden/ref_keypoints.npz); with every subset of cotangents, empty sizes, unaligned views,
non-finite inputs, repeated, under a poisoned workspace, counted launch by launch and captured into one hipGraph.

Only the yaw bin passes through ``sqrtf`` / ``atan2f``: the cases keep the generator's 1e-2 margin around every rounding tie
and the clamp, and the bin is asserted equal to the oracle's.

Against torch on the device (U = 2^-24, first order): ``kpt_cam``, ``mesh_cam``, ``kpt_proj`` and the loss map are asserted
BIT-EQUAL to the reference's expressions.  A gradient element is a sum of n contributions, n at most ``ko.depth_of`` (the K
sequential additions, SUM2's depth, the longest per-vertex list); each contribution is at most K_Q rounded operations on
either side and the two sides add them in different orders, any order being within (n - 1) U of the exact sum of magnitudes:
|ours - torch| <= (2 K_Q + 2 (n - 1)) U sum |q|, the sum of magnitudes taken from the oracle's float64 magnitude run."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from tests import kpt_oracle as ko

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U = ko.U
module = sys.modules['exavatar_release_amd.keypoints']
K_Q = 12           # per side: tx, qx, the three quotients, two products and their sum, the negation (exact), g + p, w * r: under 12
COTS = ('g_cam', 'g_proj', 'g_root', 'g_mesh')
J = 5


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)                  # (a copy: the cases are read-only)


def _n(t):
    return None if t is None else t.detach().cpu().numpy()


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = (got.view(np.int32) != want.view(np.int32)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), '%s: %d of %d elements differ, first at %s' % (what, bad.sum(), bad.size, np.argwhere(bad)[0])


def offset_view(a):
    """The array as a contiguous device view that starts 4 bytes into its storage (no 16-byte alignment)."""
    if a is None:
        return None
    flat = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
    flat[1:] = _t(a).reshape(-1)
    return flat[1:].view(a.shape)


# ---- running a case on the device -------------------------------------------------------------------------------------------
def run_kpt(c, put=_t, root_rel=False, want_mesh=True, cots=COTS, m=None, zero_cot=False):
    """(outputs, gradients) as dicts of numpy arrays; ``cots`` names the cotangents that are present."""
    m = m if m is not None else exa.BodyKeypoints(**ko.module_args(c['spec']))
    x, jn = put(c['vertices']).requires_grad_(True), put(c['joints']).requires_grad_(True)
    tr = put(c['trans']).requires_grad_(True) if c['trans'] is not None else None
    out = m(x, jn, rot=put(c['rot']), trans=tr, focal=put(c['focal']), princpt=put(c['princpt']), root_rel=root_rel,
            want_mesh=want_mesh)
    pairs = [(y, name) for y, name in zip((out.kpt_cam, out.kpt_proj, out.root_cam, out.mesh_cam), COTS)
             if name in cots and y is not None]
    grads = (None, None, None)
    if pairs:
        wrt = [x, jn] + ([tr] if tr is not None else [])
        grads = torch.autograd.grad([y for y, _ in pairs], wrt, [_t(c[n] * 0 if zero_cot else c[n]) for _, n in pairs])
        grads = tuple(grads) + ((None,) if tr is None else ())
    outs = {k: _n(getattr(out, k)) for k in out._fields}
    return outs, dict(zip(('d_vertices', 'd_joints', 'd_trans'), map(_n, grads)))


def want_kpt(c, root_rel=False, want_mesh=True, cots=COTS, zero_cot=False):
    s = c['spec']
    out = ko.forward(s, c['vertices'], c['joints'], c['rot'], c['trans'], c['focal'], c['princpt'], root_rel, want_mesh)
    present = {n: (c[n] * 0 if zero_cot else c[n]) for n in cots
               if not (n == 'g_proj' and c['focal'] is None) and not (n == 'g_mesh' and not want_mesh)}
    grads = (None, None, None)
    if present:
        grads = ko.backward(s, c['vertices'], c['joints'], out['yaw_bin'], c['trans'], c['focal'], c['princpt'], root_rel, **present)
    return out, dict(zip(('d_vertices', 'd_joints', 'd_trans'), grads))


def check_kpt(c, what='', **kw):
    put = kw.pop('put', _t)
    m = kw.pop('m', None)
    got, ggot = run_kpt(c, put=put, m=m, **kw)
    want, gwant = want_kpt(c, **kw)
    assert got['yaw_bin'].dtype == np.int32 and np.array_equal(got['yaw_bin'], want['yaw_bin']), (what, got['yaw_bin'], want['yaw_bin'])
    for name in ('kpt_cam', 'root_cam', 'kpt_proj', 'mesh_cam'):
        assert (got[name] is None) == (want[name] is None), (what, name)
        if want[name] is not None:
            same_bits(got[name], want[name], '%s %s' % (what, name))
    for name, g in gwant.items():
        assert (ggot[name] is None) == (g is None), (what, name)
        if g is not None:
            same_bits(ggot[name], g, '%s %s' % (what, name))
    return got, ggot


# ---- oracle parity ------------------------------------------------------------------------------------------------------------
KS, VS = (1, 63, 64, 65, 135, 255, 256, 257), (3, 255, 256, 257)
ROOTS = ('joint', 'vertex', 'landmark')


@pytest.mark.parametrize('K,V', list(itertools.product(KS, VS)))
def test_equals_the_oracle(K, V):
    """B in {1, 3} and Ld in {0, 17} alternate so that every K and every V meets both values of each; the root cycles through
    a joint, a vertex and a landmark."""
    i, j = KS.index(K), VS.index(V)
    B, Ld, root = (1, 3)[(i + j) % 2], (0, 17)[(i // 2 + j) % 2], ROOTS[(i + 2 * j) % 3]
    check_kpt(ko.kpt_case(1000 + 10 * i + j, B, V, J, K, Ld, root=root), 'K %d V %d B %d Ld %d root %s' % (K, V, B, Ld, root))


def test_equals_the_oracle_at_the_smplx_size():
    check_kpt(ko.kpt_case(7, 2, 10475, 55, 135, 17, root='joint'), 'V 10475')


@pytest.mark.parametrize('Ld', [0, 17])
@pytest.mark.parametrize('root', ROOTS + ('dynamic',))
def test_every_kind_of_root(root, Ld):
    if root == 'dynamic' and not Ld:
        root = 'landmark'
    check_kpt(ko.kpt_case(21, 3, 257, J, 65, Ld, root=root), 'root %s Ld %d' % (root, Ld))


def test_duplicates_in_kpt_idx_and_a_vertex_shared_across_bins():
    c = ko.kpt_case(31, 3, 300, J, 135, 17, duplicates=True)
    assert len(set(c['spec']['kpt_idx'].tolist())) < 135
    check_kpt(c, 'duplicates')
    c = ko.kpt_case(32, 3, 300, J, 65, 17, shared=True, degs=[3.2, -7.3, 44.0])
    got, _ = check_kpt(c, 'shared')
    assert got['yaw_bin'].tolist() == [3, 46, 39]
    m = exa.BodyKeypoints(**ko.module_args(c['spec']))
    v = int(c['spec']['faces'][0, 0])
    t = m.vrow[v].item()
    ks, bins = (a[m.voff[t]:m.voff[t + 1]].tolist() for a in (m.vent_k, m.vent_bin))
    assert {(0, 3), (1, 46), (2, 39)} <= set(zip(ks, bins)) and -1 in bins, 'one vertex under three keypoints in three bins'


@pytest.mark.parametrize('root_rel,want_mesh', [(True, True), (True, False), (False, False)])
def test_root_rel_and_want_mesh(root_rel, want_mesh):
    check_kpt(ko.kpt_case(41, 3, 257, J, 65, 17, root='landmark'), 'root_rel %s mesh %s' % (root_rel, want_mesh), root_rel=root_rel,
              want_mesh=want_mesh)


def test_without_trans_and_without_a_projection():
    check_kpt(ko.kpt_case(42, 2, 100, J, 30, 17, n_trans=False), 'no trans')
    check_kpt(ko.kpt_case(43, 2, 100, J, 30, 17, proj=False), 'no projection')
    check_kpt(ko.kpt_case(44, 2, 100, J, 30, 0, n_trans=False, proj=False), 'neither', root_rel=True)


# ---- cotangents, empty sizes ------------------------------------------------------------------------------------------------------
def test_every_subset_of_cotangents_and_zero_cotangents():
    c = ko.kpt_case(51, 2, 300, J, 65, 17, root='vertex')
    m = exa.BodyKeypoints(**ko.module_args(c['spec']))
    for n in range(1, 5):
        for cots in itertools.combinations(COTS, n):
            check_kpt(c, 'cotangents %s' % (cots,), cots=cots, m=m)
    _, grads = check_kpt(c, 'zero cotangents', zero_cot=True, m=m)
    assert all(not g.any() for g in grads.values())
    x = _t(c['vertices']).requires_grad_(True)
    out = m(x, _t(c['joints']), rot=_t(c['rot']))
    (g,) = torch.autograd.grad(out.mesh_cam, x, _t(c['g_mesh']))      # only mesh_cam: untouched rows carry g_mesh alone
    untouched = np.flatnonzero(_n(m.vrow) == -1)
    assert untouched.size and np.array_equal(_n(g)[:, untouched], c['g_mesh'][:, untouched])


def test_empty_batch_and_empty_selection():
    c = ko.kpt_case(52, 2, 100, J, 30, 17)
    m = exa.BodyKeypoints(**ko.module_args(c['spec']))
    out = m(torch.empty(0, 100, 3, device=DEV), torch.empty(0, J, 3, device=DEV), rot=torch.empty(0, J, 3, 3, device=DEV),
            trans=torch.empty(0, 3, device=DEV), focal=torch.empty(0, 2, device=DEV), princpt=torch.empty(0, 2, device=DEV))
    assert out.kpt_cam.shape == (0, 30, 3) and out.kpt_proj.shape == (0, 30, 2) and out.mesh_cam.shape == (0, 100, 3)
    assert out.yaw_bin.shape == (0,) and out.yaw_bin.dtype == torch.int32
    c0 = ko.kpt_case(53, 2, 100, J, 0, 17, root='landmark')
    assert c0['spec']['kpt_idx'].size == 0
    got, grads = check_kpt(c0, 'K = 0')
    assert got['kpt_cam'].shape == (2, 0, 3) and got['kpt_proj'].shape == (2, 0, 2)
    loss = exa.CoordLoss(*ko.HANDS)
    e = torch.empty(0, 50, 2, device=DEV)
    assert loss(e, e, torch.empty(0, 50, 1, device=DEV), torch.empty(0, 50, 3, device=DEV)).shape == (0, 50, 2)


# ---- views, non-finite inputs -------------------------------------------------------------------------------------------------
def test_views_at_a_four_byte_offset_give_the_same_bits():
    check_kpt(ko.kpt_case(61, 3, 301, J, 135, 17, root='landmark'), 'offset views', put=offset_view)
    check_coord(ko.coord_case(62, 6, 65), put=offset_view)


def test_a_zero_depth_gives_what_ieee_gives_and_leaves_the_other_rows_alone():
    c = ko.kpt_case(63, 2, 100, J, 30, 17, root='joint')
    c['spec']['kpt_idx'][4] = c['spec']['root_idx']      # cam = (raw - root) + trans = trans exactly
    c['trans'][:, 2] = 0
    got, _ = check_kpt(c, 'Z = 0', cots=())
    assert np.isinf(got['kpt_proj'][:, 4]).all() and (got['kpt_cam'][:, 4, 2] == 0).all()
    others = np.delete(np.arange(30), np.flatnonzero(c['spec']['kpt_idx'] == c['spec']['root_idx']))
    assert np.isfinite(got['kpt_proj'][:, others]).all()
    c['trans'][:, :2] = 0                                                     # 0 / 0
    got, _ = check_kpt(c, '0 / 0', cots=())
    assert np.isnan(got['kpt_proj'][:, 4]).all() and np.isfinite(got['kpt_proj'][:, others]).all()


def test_a_non_finite_rot_gives_bin_zero_and_finite_table_reads():
    c = ko.kpt_case(64, 3, 100, J, 30, 17, root='dynamic')
    c['rot'][0] = np.nan
    c['rot'][1, c['spec']['chain'][1]] = np.inf
    got, _ = check_kpt(c, 'non-finite rot')
    assert got['yaw_bin'][:2].tolist() == [0, 0]
    assert all(np.isfinite(got[k]).all() for k in ('kpt_cam', 'kpt_proj', 'root_cam', 'mesh_cam'))


# ---- reproducibility -----------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_a_poisoned_workspace_changes_nothing():
    c, cc = ko.kpt_case(71, 3, 1000, J, 135, 17), ko.coord_case(72, 12, 135)
    m = exa.BodyKeypoints(**ko.module_args(c['spec']))
    runs = [run_kpt(c, m=m) for _ in range(2)]
    exa.config.poison = True
    runs.append(run_kpt(c, m=m))
    coord = [run_coord(cc) for _ in range(2)]
    for other, name in ((runs[1], 'second call'), (runs[2], 'poisoned workspace')):
        for a, b in zip(runs[0], other):
            for k in a:
                if k == 'yaw_bin':
                    assert np.array_equal(a[k], b[k])
                else:
                    same_bits(a[k], b[k], '%s, %s' % (k, name))
    for a, b in zip(*coord):
        same_bits(a, b, 'coord, second call')
    check_kpt(c, 'poisoned workspace against the oracle', m=m)


def test_launch_counts(monkeypatch):
    calls = []
    real = module.launch

    def counting(abi, name, *args):
        calls.append(name)
        return real(abi, name, *args)
    monkeypatch.setattr(module, 'launch', counting)
    c = ko.kpt_case(73, 2, 300, J, 65, 17)
    run_kpt(c)
    run_kpt(c, want_mesh=False)
    run_coord(ko.coord_case(74, 6, 50))
    assert calls == ['exa_mesh_keypoints_forward', 'exa_mesh_keypoints_backward'] * 2 + \
        ['exa_mesh_coord_loss_forward', 'exa_mesh_coord_loss_backward']
    # one C call each way; the kernels behind them: at most two forward and three backward (csrc/keypoints.hip), one each for the loss
    src = open(os.path.join(os.path.dirname(module.__file__), 'csrc', 'keypoints.hip')).read()
    body = lambda fn: src[src.index('int %s(' % fn):].split('\n}\n')[0]      # noqa: E731
    count = lambda fn: body(fn).count('hipLaunchKernelGGL')      # noqa: E731
    assert count('exa_mesh_keypoints_forward') == 2 and count('exa_mesh_keypoints_backward') == 3
    assert count('exa_mesh_coord_loss_forward') == 1 and count('exa_mesh_coord_loss_backward') == 1


# ---- CoordLoss ----------------------------------------------------------------------------------------------------------------
def run_coord(c, put=_t, weight=True, hands=ko.HANDS, m=None):
    m = m if m is not None else exa.CoordLoss(*hands)
    proj = put(c['proj']).requires_grad_(True)
    loss, hand_w = m(proj, put(c['gt']), put(c['valid']), put(c['cam']), weight=put(c['weight']) if weight else None,
                     return_hand_w=True)
    (g,) = torch.autograd.grad(loss, proj, _t(c['g']))
    return _n(loss), _n(hand_w), _n(g)


def check_coord(c, put=_t, weight=True, hands=ko.HANDS):
    loss, hand_w, grad = run_coord(c, put, weight, hands)
    w = c['weight'] if weight else None
    want, hw = ko.coord_forward(c['proj'], c['gt'], c['valid'], c['cam'], *hands, weight=w)
    assert np.array_equal(hand_w, hw), 'hand_w'
    same_bits(loss, want, 'coord loss')
    same_bits(grad, ko.coord_backward(c['proj'], c['gt'], c['valid'], hw, c['g'], weight=w), 'coord gradient')
    return hand_w


@pytest.mark.parametrize('B,K', [(1, 45), (3, 63), (6, 64), (6, 65), (12, 135), (64, 135), (2, 257)])
@pytest.mark.parametrize('weight', [True, False])
def test_coord_loss_equals_the_oracle(B, K, weight):
    hw = check_coord(ko.coord_case(80 + B + K, B, K), weight=weight)
    if B >= 6:
        lost = (hw == 0).any(1)
        assert lost[:2].all() and not lost[2:5].any(), 'the cases fire on items 0 and 1 and not on 2, 3, 4'


def test_coord_loss_accepts_a_flat_kpt_valid_and_detaches_kpt_cam():
    c = ko.coord_case(91, 6, 50)
    m = exa.CoordLoss(*ko.HANDS)
    proj = _t(c['proj']).requires_grad_(True)
    cam = _t(c['cam']).requires_grad_(True)
    a = m(proj, _t(c['gt']), _t(c['valid']), cam)
    b = m(proj, _t(c['gt']), _t(c['valid'][:, :, 0]), cam.detach())
    same_bits(_n(a), _n(b), 'flat kpt_valid')
    assert torch.autograd.grad(a, cam, torch.ones_like(a), allow_unused=True)[0] is None


# ---- against torch on the device -------------------------------------------------------------------------------------------------
def reference_on_device(c, bins, tr, x, jn, root_rel=False):
    """The reference's expressions (body_models.py:1257-1283 with the faces its ladder selects, model.py:97-112) in torch."""
    s = c['spec']
    B = x.shape[0]
    faces = _t(s['faces'])
    lmk_f = torch.cat([_t(s['lmk_f'])[None].expand(B, -1), _t(s['dyn_f'])[bins.long()]], 1)
    lmk_w = torch.cat([_t(s['lmk_w'])[None].expand(B, -1, -1), _t(s['dyn_w'])[bins.long()]], 1)
    lmk_faces = faces[lmk_f.reshape(-1)].view(B, -1, 3) + torch.arange(B, device=DEV).view(-1, 1, 1) * x.shape[1]
    lmk_vertices = x.reshape(-1, 3)[lmk_faces].view(B, -1, 3, 3)
    landmarks = torch.einsum('blfi,blf->bli', [lmk_vertices, lmk_w])
    full = torch.cat([jn, torch.index_select(x, 1, _t(s['extra'])), landmarks, x[:, _t(s['append'])]], 1)
    kpt_cam = full[:, _t(s['kpt_idx']), :]
    root_cam = full[:, int(s['root_idx']), :]
    mesh_cam = x - root_cam[:, None, :] + tr[:, None, :]
    kpt_cam = kpt_cam - root_cam[:, None, :] + tr[:, None, :]
    focal, princpt = _t(c['focal']), _t(c['princpt'])
    px = kpt_cam[:, :, 0] / kpt_cam[:, :, 2] * focal[:, None, 0] + princpt[:, None, 0]
    py = kpt_cam[:, :, 1] / kpt_cam[:, :, 2] * focal[:, None, 1] + princpt[:, None, 1]
    kpt_proj = torch.stack((px, py), 2)
    if root_rel:
        mesh_cam, kpt_cam = mesh_cam - tr[:, None, :], kpt_cam - tr[:, None, :]
    return kpt_cam, kpt_proj, root_cam, mesh_cam


def reference_bins(c):
    """The reference's ladder (lbs.py:85-98) in torch on the device."""
    rot, chain = _t(c['rot']), c['spec']['chain']
    rel = torch.eye(3, device=DEV).repeat(rot.shape[0], 1, 1)
    for j in chain:
        rel = torch.bmm(rot[:, j], rel)
    sy = torch.sqrt(rel[:, 0, 0] * rel[:, 0, 0] + rel[:, 1, 0] * rel[:, 1, 0])
    y = torch.round(torch.clamp(-torch.atan2(-rel[:, 2, 0], sy) * 180.0 / np.pi, max=39)).to(dtype=torch.long)
    neg_mask, mask = y.lt(0).to(dtype=torch.long), y.lt(-39).to(dtype=torch.long)
    neg_vals = mask * 78 + (1 - mask) * (39 - y)
    return neg_mask * neg_vals + (1 - neg_mask) * y


def within(got, want, bound, what):
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    frac = float((err / np.maximum(bound, 1e-300)).max())
    print('%s: bit-equal to torch on the device: %s; worst error / bound %.3f' % (what, np.array_equal(got, want), frac))
    assert (err <= bound).all(), '%s: worst excess %g' % (what, float((err - bound).max()))


@pytest.mark.parametrize('root_rel', [False, True])
def test_against_the_references_expressions_on_the_device(root_rel):
    """The full selection -- joints, vertices, static and dynamic landmarks, duplicates, a landmark as the root -- against the
    reference's expressions in torch on the device: the four outputs BIT-EQUAL.  The elementwise operations have one possible
    order; a landmark row is defined as the order ``torch.einsum`` takes on the device (the header: a product and two fused
    multiply-adds over the face's corners)."""
    c = ko.kpt_case(101, 3, 1000, J, 135, 17, root='landmark', duplicates=True)
    got, ggot = run_kpt(c, root_rel=root_rel)
    bins = reference_bins(c)
    assert np.array_equal(_n(bins), got['yaw_bin']), 'the reference\'s ladder on the device selects the same bins'
    x, jn, tr = (_t(c[k]).requires_grad_(True) for k in ('vertices', 'joints', 'trans'))
    ref = reference_on_device(c, bins, tr, x, jn, root_rel)
    for name, r in zip(('kpt_cam', 'kpt_proj', 'root_cam', 'mesh_cam'), ref):
        same_bits(got[name], _n(r), name + ' against the reference\'s expressions on the device')
    if root_rel:
        return      # torch's d_trans cancels sums of magnitudes there; the gradients are held in the other run
    grads = torch.autograd.grad(ref, (x, jn, tr), [_t(c[n]) for n in COTS])
    mags = ko.backward(c['spec'], c['vertices'], c['joints'], got['yaw_bin'], c['trans'], c['focal'], c['princpt'], False,
                       *[c[n] for n in COTS], dtype=np.float64, magnitude=True)
    n = ko.depth_of(c['spec'], 1000)
    for name, g, mag in zip(('d_vertices', 'd_joints', 'd_trans'), grads, mags):
        within(ggot[name], _n(g), (2 * K_Q + 2 * (n - 1)) * U * mag, '%s (n = %d)' % (name, n))


@pytest.mark.parametrize('B', [1, 3, 64])
def test_landmark_rows_equal_torchs_einsum_on_the_device_bit_for_bit(B):
    """Every row of the layer with a root joint at the origin and no ``trans``: ``kpt_cam = raw - 0`` is the raw row exactly, so
    the landmark rows are compared with ``torch.einsum('blfi,blf->bli')`` directly, at batch sizes from 1 to the fitting's 64
    (the einsum is a batched product, whose kernel may depend on the batch)."""
    c = ko.kpt_case(103 + B, B, 1000, J, 0, 17, root='joint', n_trans=False, proj=False)
    s = c['spec']
    s['kpt_idx'] = None
    c['joints'][:, s['root_idx']] = 0
    m = exa.BodyKeypoints(**ko.module_args(s))
    x = _t(c['vertices'])
    out = m(x, _t(c['joints']), rot=_t(c['rot']), want_mesh=False)
    bins = out.yaw_bin.long()
    lmk_f = torch.cat([_t(s['lmk_f'])[None].expand(B, -1), _t(s['dyn_f'])[bins]], 1)
    lmk_w = torch.cat([_t(s['lmk_w'])[None].expand(B, -1, -1), _t(s['dyn_w'])[bins]], 1)
    lmk_vertices = x[torch.arange(B, device=DEV)[:, None, None], _t(s['faces'])[lmk_f]]      # [B, L, 3 corners, 3]
    ref = torch.einsum('blfi,blf->bli', [lmk_vertices, lmk_w])
    lo = J + len(s['extra'])
    same_bits(_n(out.kpt_cam)[:, lo:lo + lmk_f.shape[1]], _n(ref), 'landmark rows against torch.einsum on the device')


def test_coord_loss_against_the_references_expressions_on_the_device():
    c = ko.coord_case(102, 12, 135)
    loss, hand_w, grad = run_coord(c)
    proj = _t(c['proj']).requires_grad_(True)
    ref = torch.abs(proj - _t(c['gt'])) * _t(c['valid']) * _t(hand_w)[:, :, None] * _t(c['weight'])
    same_bits(loss, _n(ref), 'coord loss against the reference\'s expression on the device')
    (g,) = torch.autograd.grad(ref, proj, _t(c['g']))
    mag = np.abs(c['g'].astype(np.float64) * c['weight'] * hand_w[:, :, None] * c['valid'])
    within(grad, _n(g), 4 * U * mag, 'coord gradient')      # three products per side, one term


# ---- the golden on the device -------------------------------------------------------------------------------------------------
def test_the_references_own_run_on_the_device(golden_dir):
    from tests import test_kpt_oracle as tko
    g = dict(np.load(os.path.join(golden_dir, 'ref_keypoints.npz')))
    s, x, cot = tko.spec_of(g), tko.layer_inputs(g), tko.cotangents(g)
    c = dict(x, spec=s, **cot)
    Ls = len(s['lmk_f'])
    for root_rel, tag in ((False, ''), (True, 'rel')):
        got, ggot = check_kpt(c, 'golden', root_rel=root_rel)
        assert np.array_equal(got['yaw_bin'], g['kpt_faces_sel_64'][:, Ls]), 'the golden\'s bins on the device'
        res = dict(got, **ggot)
        names = ('kpt_cam', 'mesh_cam', 'd_trans') + (() if root_rel else ('root_cam', 'kpt_proj', 'd_vertices', 'd_joints'))
        for name in names:
            assert tko.meets_the_bar(res[name], g['kpt_%s_%s32' % (name, tag)], g['kpt_%s_%s64' % (name, tag)], name + ' ' + tag)
    hands = (list(g['coord_lhand']), list(g['coord_rhand']), int(g['coord_wrists'][0]), int(g['coord_wrists'][1]))
    cc = {k: g['coord_' + k] for k in ('proj', 'gt', 'valid', 'cam', 'weight', 'g')}
    loss, hand_w, grad = run_coord(cc, hands=hands)
    assert np.array_equal(hand_w, g['coord_hand_w_64']), 'the golden\'s decisions on the device'
    assert tko.meets_the_bar(loss, g['coord_weighted_32'], g['coord_weighted_64'], 'coord loss * weight')
    assert tko.meets_the_bar(grad, g['coord_grad_32'], g['coord_grad_64'], 'coord gradient')
    plain = run_coord(cc, hands=hands, weight=False)[0]
    same_bits(plain, g['coord_loss_32'], 'coord loss against the reference float32 run')


# ---- capture -----------------------------------------------------------------------------------------------------------------
def test_one_captured_graph_replays_the_eager_bits():
    """Forward and backward of BodyKeypoints -> CoordLoss in one hipGraph: nothing in the path reads back."""
    c = ko.kpt_case(111, 4, 1000, J, 135, 17, root='joint')
    cc = ko.coord_case(112, 4, 135)
    m, loss = exa.BodyKeypoints(**ko.module_args(c['spec'])).to(DEV), exa.CoordLoss(*ko.HANDS)
    xs = [_t(c[k]).requires_grad_(True) for k in ('vertices', 'joints', 'trans')]
    const = {k: _t(c[k]) for k in ('rot', 'focal', 'princpt')}
    const.update({k: _t(cc[k]) for k in ('gt', 'valid', 'weight')})
    cot = [_t(cc['g']), _t(c['g_mesh']), _t(c['g_cam'])]

    def step():
        out = m(xs[0], xs[1], rot=const['rot'], trans=xs[2], focal=const['focal'], princpt=const['princpt'])
        term = loss(out.kpt_proj, const['gt'], const['valid'], out.kpt_cam.detach(), weight=const['weight'])
        return (out.kpt_cam, out.kpt_proj, out.root_cam, out.mesh_cam, term) + \
            torch.autograd.grad([term, out.mesh_cam, out.kpt_cam], xs, cot)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    with torch.no_grad():
        xs[0].mul_(1.25)
        xs[1].add_(0.01)
        xs[2].mul_(1.1)
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    for i, (got, want) in enumerate(zip(outs, eager)):
        same_bits(_n(got), _n(want), 'replayed output %d' % i)
    want = ko.forward(c['spec'], _n(xs[0]), _n(xs[1]), c['rot'], _n(xs[2]), c['focal'], c['princpt'])
    same_bits(_n(outs[1]), want['kpt_proj'], 'replayed kpt_proj against the oracle')
