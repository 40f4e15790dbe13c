"""The fitting loss's mesh terms on the device: each term against its CPU restatement (tests/fit_oracle.py) BIT FOR BIT, map and
gradient, at the sizes where the kernels' work split changes; against the reference's expressions run by torch on the
device; against the reference's own run of its classes (tests/golden/ref_fit_terms.npz); repeated, unaligned and captured.

PoseLoss and the device's sinf / cosf: the oracle takes the sine and cosine of the half angles from ``torch.sin`` / ``torch.cos``
ON THE DEVICE (the same device library functions the kernel calls), so that everything around that one step is held bit for
bit; the step itself is held against float64 as the kinematics' is (at most 4x the CPU float32 evaluation's own error).

Against torch on the device (U = 2^-24, first order).  The symmetry map is BIT-EQUAL to the reference's expression (torch
adds its three products in the header's order) and is asserted so; the other maps are held to the bounds of
tests/fit_oracle.py (torch's device sums have an order of their own there, as its CPU sums do).  Gradients: a vertex's (row's) gradient is a sum of n contributions;
each is a handful of rounded operations on either side (K_Q below) and the two sides add them in different orders, any
order being within (n - 1) U of the exact sum of magnitudes: |ours - torch| <= (2 K_Q + 2 (n - 1)) U sum |q|, n the longest
CSR row (two edges per slot for the edge term, plus the row's own term for the symmetry term).  Elements whose sign
decision is within 1e-5 of zero are left out (a flipped sign is not a rounding error), at most 1 %."""
import os
import sys

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import p3d_standins
from tests import fit_oracle as fo

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U = fo.U
module = sys.modules['exavatar_release_amd.fit_terms']
K_Q_EDGE = 16      # per side: two differences, a squared norm of three terms and its root for d_out (4.5) and for d_gt, the
#                    subtraction and its sign (exact), g m, the quotient, the product with the difference (1 + 3): under 16
K_Q_SYM = 2        # per side: sign * g is exact, the product with the weight rounds once
# PoseLoss' gradient against autograd through the stand-in on the device.  With S = sum_q |g_q| of a rotation, |q| <= 1,
# t = 2 / n ~ 2 and (|x| + |y| + |z|) <= sqrt(3) angle, the backward's intermediates are bounded by: h <= 2 |G|; g_r .. g_k <=
# 4 S from their (at most eight) terms plus (2 r) g_n <= 4 S, 8 S in all; g_s <= 14 S angle; g_half <= 8 S + 14 S = 22 S;
# g_angle <= 11 S + 7 S; each output <= 4 S + 18 S = 22 S.  Either side performs fewer than 70 rounded operations (sinf /
# cosf counted at 2 U), each within U of a value of at most 22 S: |ours - torch| <= 2 * 70 * 22 U S.  The count holds for
# angles away from 0 (autograd divides by the angle where the kernel's small-angle branch does not) and below pi (pose_case
# stays there): rows outside POSE_ANGLES are left out, as are those with an ambiguous sign of R_out - R_gt.
POSE_GRAD_K = 2 * 70 * 22
POSE_ANGLES = (1e-3, 3.0)
DEVICE_TRIG = (lambda h: torch.sin(torch.from_numpy(np.ascontiguousarray(h)).to(DEV)).cpu().numpy(),
               lambda h: torch.cos(torch.from_numpy(np.ascontiguousarray(h)).to(DEV)).cpu().numpy())


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # (a copy: the cases are read-only)


def _n(t):
    return t.detach().cpu().numpy()


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = (got.view(np.int32) != want.view(np.int32)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), '%s: %d of %d elements differ, first at %s' % (what, bad.sum(), bad.size, np.argwhere(bad)[0])


def offset_view(a):
    """The array as a contiguous device view that starts 4 bytes into its storage (no 16-byte alignment)."""
    flat = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
    flat[1:] = _t(a).reshape(-1)
    return flat[1:].view(a.shape)


def grad_of(y, x, g):
    return _n(torch.autograd.grad(y, x, g)[0])


# ---- running a case on the device: (loss, gradient) as numpy ----------------------------------------------------------------
def run_edge(c, put=_t, module_=None):
    m = module_ or exa.EdgeLengthLoss(c['face'])
    x = put(c['out']).requires_grad_(True)
    y = m(x, put(c['gt']), put(c['valid']))
    return _n(y), grad_of(y, x, put(c['g'])) if y.requires_grad else None


def want_edge(c):
    a = (c['out'], c['gt'], fo.valid_rows(c), c['face'])
    return fo.edge_forward(*a), fo.edge_backward(*a, c['g'])


def check_edge(c, put=_t):
    got, want = run_edge(c, put), want_edge(c)
    same_bits(got[0], want[0], 'edge map')
    same_bits(got[1], want[1], 'edge dL/dcoord_out')
    return got


def sym_module(c):
    return exa.FaceOffsetSymmetricReg(int(c['vertex_num']), c['face_vertex_idx'], c['closest_faces'], c['bc'])


def run_sym(c, put=_t, m=None):
    m = m or sym_module(c)
    x = put(c['p']).requires_grad_(True)
    y = m(x)
    return _n(y), grad_of(y, x, put(c['g']))


def want_sym(c):
    taps, w, _, _ = fo.flip_plan(int(c['vertex_num']), c['face_vertex_idx'], c['closest_faces'], c['bc'])
    return fo.sym_forward(c['p'], taps, w), fo.sym_backward(c['p'], taps, w, c['g'])


def check_sym(c, put=_t):
    got, want = run_sym(c, put), want_sym(c)
    same_bits(got[0], want[0], 'symmetry map')
    same_bits(got[1], want[1], 'symmetry dL/dface_offset')


def run_pose(c, put=_t, shape=None):
    shape = shape or c['out'].shape
    x = put(c['out'].reshape(shape)).requires_grad_(True)
    y = exa.PoseLoss()(x, put(c['gt'].reshape(shape)))
    return _n(y), grad_of(y, x, put(c['g'].reshape(tuple(y.shape))))


def check_pose(c, put=_t, shape=None):
    loss, grad = run_pose(c, put, shape)
    same_bits(loss.reshape(-1, 9), fo.pose_forward(c['out'], c['gt'], trig=DEVICE_TRIG), 'pose map')
    same_bits(grad.reshape(-1, 3), fo.pose_backward(c['out'], c['gt'], c['g'], trig=DEVICE_TRIG), 'pose dL/dpose_out')
    return loss, grad


def run_v2v(c, put=_t, scale=10.0):
    x = put(c['out']).requires_grad_(True)
    y = exa.centered_v2v_loss(x, put(c['target']), put(c['weight']), scale)
    means = _n(y.grad_fn.saved_tensors[3]) if c['out'].size else None
    return _n(y), grad_of(y, x, put(c['g'])), means


def check_v2v(c, put=_t, scale=10.0):
    loss, grad, means = run_v2v(c, put, scale)
    same_bits(loss, fo.v2v_forward(c['out'], c['target'], c['weight'], scale), 'centred map')
    same_bits(grad, fo.v2v_backward(c['out'], c['target'], c['weight'], c['g'], scale), 'centred dL/dout')
    return means


# ---- edge length -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,V,F', [(1, 3, 1), (1, 300, 255), (1, 300, 256), (2, 300, 257), (3, 1000, 1990), (2, 5023, 9976)])
def test_edge_equals_the_oracle(B, V, F):
    check_edge(fo.edge_case(1000 + F, B, V, F))


def test_edge_a_fan_whose_hub_lies_in_300_faces_and_an_isolated_vertex():
    face = [[0, i, i + 1] for i in range(1, 301)]
    c = fo.edge_case(11, 2, 303, 0, face=face)                    # vertex 302 is in no face
    loss, grad = check_edge(c)
    same_bits(grad[:, 302], np.zeros((2, 3), np.float32), 'the isolated vertex: +0.0')


def test_edge_degenerate_edges_give_a_finite_zero_gradient():
    """Face 1 repeats vertex 3; vertices 6 and 7 coincide exactly and lie only in face 3, whose three edges all have length
    0; vertices 2 and 5 coincide and share the edge (2, 5) of face 2."""
    c = fo.edge_case(12, 2, 8, 0, face=[[0, 1, 2], [3, 3, 4], [2, 4, 5], [6, 7, 6]])
    c['out'][:, 7] = c['out'][:, 6]
    c['out'][:, 5] = c['out'][:, 2]
    c['valid'][:] = 1
    loss, grad = check_edge(c)
    assert np.isfinite(grad).all()
    same_bits(grad[:, 6:8], np.zeros((2, 2, 3), np.float32), 'vertices with zero-length edges only: +0.0')
    assert (loss[:, 1, 0] == 0).all(), 'edge (3, 3) of face 1: |0 - 0|'


@pytest.mark.parametrize('valid_shape,gt_batch', [('1V1', None), ('BV1', None), ('V', None), ('BV1', 1), ('1V1', 1)])
def test_edge_every_accepted_shape_of_valid_and_coord_gt(valid_shape, gt_batch):
    check_edge(fo.edge_case(13, 3, 77, 130, valid_shape=valid_shape, gt_batch=gt_batch))


def test_edge_empty_sizes_and_missing_or_zero_cotangents():
    c = fo.edge_case(14, 0, 9, 5)
    loss, _ = run_edge(c)
    assert loss.shape == (0, 15, 1)
    c = fo.edge_case(15, 2, 9, 0)
    loss, grad = run_edge(c)
    assert loss.shape == (2, 0, 1)
    same_bits(grad, np.zeros((2, 9, 3), np.float32), 'no faces: +0.0 everywhere')
    c = fo.edge_case(16, 2, 300, 257)
    c['g'][:] = 0
    check_edge(c)
    x = _t(c['out']).requires_grad_(True)
    y = exa.EdgeLengthLoss(c['face'])(x, _t(c['gt']), _t(c['valid']))
    other = _t(c['out']).requires_grad_(True)
    assert torch.autograd.grad((y * 0).sum() + other.sum(), [x, other])[0].abs().max() == 0
    assert torch.autograd.grad(other.sum() * 2, [x, other], allow_unused=True)[0] is None


# ---- flip symmetry ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Vf', [1, 255, 256, 257])
def test_symmetry_equals_the_oracle(Vf):
    c = fo.sym_case(2000 + Vf, 2, Vf + 40, Vf, hub=min(Vf - 1, 70))
    taps, _, offsets, _ = fo.flip_plan(c['vertex_num'], c['face_vertex_idx'], c['closest_faces'], c['bc'])
    if Vf > 1:
        rows = np.diff(offsets)
        assert rows.max() > 64 and (rows == 0).any() and (taps == -1).any() and taps[2, 1] == 2, \
            'a row named by more than 64 taps, one named by none, taps of -1 and a self-tap'
    check_sym(c)


def test_symmetry_at_full_size_and_empty():
    check_sym(fo.sym_case(21, 2, 10475, 5023, hub=100))
    c = fo.sym_case(22, 0, 60, 25)
    x = _t(c['p']).requires_grad_(True)
    assert sym_module(c)(x).shape == (0, 25)
    c = fo.sym_case(23, 2, 60, 25)
    c['g'][:] = 0
    check_sym(c)


# ---- pose ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 63, 64, 65, 64 * 55])
def test_pose_equals_the_oracle_given_the_devices_sine_and_cosine(N):
    c = fo.pose_case(3000 + N, N)
    check_pose(c, shape=(1, N * 3))
    if N == 64 * 55:
        loss, grad = check_pose(c, shape=(64, 55, 3))
        assert loss.shape == (64, 55, 3, 3) and np.isfinite(grad).all()
        g = grad.reshape(-1, 3)
        assert not g[6].any() and not g[7].any(), 'out == gt rows (a zero row among them): gradient 0'
        assert not loss.reshape(-1, 9)[6].any()


def test_pose_both_layouts_mixed_and_the_trigonometric_step_against_float64():
    c = fo.pose_case(31, 2 * 55)
    x = _t(c['out'].reshape(2, 165)).requires_grad_(True)
    y = exa.PoseLoss()(x, _t(c['gt'].reshape(2, 55, 3)))
    assert y.shape == (2, 55, 3, 3)
    want = fo.pose_forward(c['out'], c['gt'], trig=DEVICE_TRIG)
    same_bits(_n(y).reshape(-1, 9), want, 'mixed layouts')
    exact = fo.pose_forward(c['out'], c['gt'], np.float64)
    cpu32 = fo.pose_forward(c['out'], c['gt'])
    err_dev, err_cpu = np.abs(_n(y).reshape(-1, 9) - exact).max(), np.abs(cpu32 - exact).max()
    print('pose map: device max error %.3e, CPU float32 max error %.3e, ratio %.2f' % (err_dev, err_cpu, err_dev / err_cpu))
    assert err_cpu > 0 and err_dev <= 4 * err_cpu
    keep = ~fo.pose_ambiguous(c['out'], c['gt'])
    assert keep.mean() >= 0.99
    grad = grad_of(y, x, _t(c['g'].reshape(2, 55, 3, 3))).reshape(-1, 3)
    g64 = fo.pose_backward(c['out'], c['gt'], c['g'], np.float64)
    g32 = fo.pose_backward(c['out'], c['gt'], c['g'])
    gerr_dev, gerr_cpu = np.abs(grad - g64)[keep].max(), np.abs(g32 - g64)[keep].max()
    print('pose gradient: device max error %.3e, CPU float32 max error %.3e, ratio %.2f' % (gerr_dev, gerr_cpu, gerr_dev / gerr_cpu))
    assert np.isfinite(grad).all() and gerr_cpu > 0 and gerr_dev <= 4 * gerr_cpu


# ---- the centred term ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', [1, 255, 256, 257, 5023, 65537])
def test_centred_term_equals_the_oracle_and_its_means_stay_within_the_depth_bound(V):
    c = fo.v2v_case(4000 + V, 3, V)
    means = check_v2v(c)
    same_bits(means, fo.v2v_means(c['out'], c['target']), 'means')
    m64 = np.concatenate([c['out'].astype(np.float64).mean(1), c['target'].astype(np.float64).mean(1)], 1)
    mag = np.concatenate([np.abs(c['out']).astype(np.float64).mean(1), np.abs(c['target']).astype(np.float64).mean(1)], 1)
    frac = np.abs(means.astype(np.float64) - m64) / ((fo.v2v_depth(V) + 2) * U * mag)
    print('V = %d: depth %d, worst mean error / bound %.3f' % (V, fo.v2v_depth(V), frac.max()))
    assert (frac <= 1).all()


def test_centred_term_zero_weight_other_scale_and_empty():
    check_v2v(fo.v2v_case(41, 3, 300, zero_weight=True))
    check_v2v(fo.v2v_case(42, 2, 300), scale=0.5)
    c = fo.v2v_case(43, 0, 7)
    assert exa.centered_v2v_loss(_t(c['out']), _t(c['target']), _t(c['weight'])).shape == (0, 7, 3)
    c = fo.v2v_case(44, 2, 300)
    c['g'][:] = 0
    check_v2v(c)
    for shape in ((300,), (300, 1)):
        same_bits(_n(exa.centered_v2v_loss(_t(c['out']), _t(c['target']), _t(c['weight'].reshape(shape)))),
                  fo.v2v_forward(c['out'], c['target'], c['weight']), 'weight as %s' % (shape,))


def test_centred_term_under_a_poisoned_workspace():
    exa.config.poison = True
    check_v2v(fo.v2v_case(45, 3, 777))


# ---- unaligned inputs, repeatability, launches ---------------------------------------------------------------------------
def test_views_at_a_four_byte_offset_give_the_same_bits():
    check_edge(fo.edge_case(51, 2, 301, 555), put=offset_view)
    check_sym(fo.sym_case(52, 2, 333, 257, hub=10), put=offset_view)
    check_pose(fo.pose_case(53, 65), put=offset_view)
    check_v2v(fo.v2v_case(54, 2, 1001), put=offset_view)


def test_two_calls_give_the_same_bits():
    ce, cs, cp, cv = fo.edge_case(61, 3, 1000, 1990), fo.sym_case(62, 2, 600, 300, hub=80), fo.pose_case(63, 64 * 55), \
        fo.v2v_case(64, 3, 5023)
    me, ms = exa.EdgeLengthLoss(ce['face']), sym_module(cs)
    runs = [[run_edge(ce, module_=me), run_sym(cs, m=ms), run_pose(cp), run_v2v(cv)[:2]] for _ in range(2)]
    for (a, b), name in zip(zip(*runs), ('edge', 'symmetry', 'pose', 'centred')):
        same_bits(a[0], b[0], name + ' map, second call')
        same_bits(a[1], b[1], name + ' gradient, second call')


def test_one_launch_each_way_and_two_for_the_centred_term(monkeypatch):
    calls = []
    real = module.launch

    def counting(abi, name, *args):
        calls.append(name)
        return real(abi, name, *args)
    monkeypatch.setattr(module, 'launch', counting)
    run_edge(fo.edge_case(71, 2, 300, 257))
    run_sym(fo.sym_case(72, 2, 60, 25))
    run_pose(fo.pose_case(73, 65))
    run_v2v(fo.v2v_case(74, 2, 300))
    assert calls == ['exa_mesh_edge_length_forward', 'exa_mesh_edge_length_backward', 'exa_mesh_flip_symmetry_forward',
                     'exa_mesh_flip_symmetry_backward', 'exa_mesh_pose_loss_forward', 'exa_mesh_pose_loss_backward',
                     'exa_mesh_centered_v2v_forward', 'exa_mesh_centered_v2v_backward']      # (two kernels each, the last two)


# ---- against torch on the device -------------------------------------------------------------------------------------------
def within(got, want, bound, keep, what):
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert keep.mean() >= 0.99, '%s: share of ambiguous elements %.4f' % (what, 1 - keep.mean())
    frac = float((err / np.maximum(bound, 1e-300))[keep].max()) if keep.any() else 0.0
    print('%s: bit-equal to torch on the device: %s; worst error / bound %.3f' % (what, np.array_equal(got, want), frac))
    assert (err <= bound)[keep].all(), '%s: worst excess %g' % (what, float((err - bound)[keep].max()))


def test_against_the_references_expressions_on_the_device():
    # edge: the reference's lines with a device face tensor
    c = fo.edge_case(81, 3, 1000, 1990)
    got = run_edge(c)
    x, gt, valid, f = _t(c['out']).requires_grad_(True), _t(c['gt']), _t(c['valid']), _t(c['face'])
    pairs = ((0, 1), (0, 2), (1, 2))
    d = [[torch.sqrt(torch.sum((y[:, f[:, a], :] - y[:, f[:, b], :]) ** 2, 2, keepdim=True)) for a, b in pairs] for y in (x, gt)]
    ref = torch.cat([torch.abs(d[0][k] - d[1][k]) * (valid[:, f[:, a], :] * valid[:, f[:, b], :])
                     for k, (a, b) in enumerate(pairs)], 1)
    args = (c['out'], c['gt'], fo.valid_rows(c), c['face'])
    within(got[0], _n(ref), fo.edge_bound(*args), np.ones(got[0].shape, bool), 'edge map')
    n = 2 * int(np.diff(fo.transpose(c['face'], 1000)[0]).max())
    mag = fo.edge_backward(*args, c['g'], dtype=np.float64, magnitude=True)
    keep = np.broadcast_to(~fo.edge_ambiguous(c['out'], c['gt'], c['face'])[..., None], mag.shape)
    within(got[1], grad_of(ref, x, _t(c['g'])), (2 * K_Q_EDGE + 2 * (n - 1)) * U * mag, keep, 'edge gradient (longest row %d)' % n)

    # symmetry: the reference's padded gather
    c = fo.sym_case(82, 2, 600, 300, hub=80)
    got = run_sym(c)
    p = _t(c['p']).requires_grad_(True)
    full = torch.zeros((2, 600, 3), device=DEV)
    full[:, _t(c['face_vertex_idx']), :] = p
    flip = torch.sum(full[:, _t(c['closest_faces']).view(-1), :].view(2, 600, 3, 3) * _t(c['bc']).view(1, 600, 3, 1), 2)
    ref = (torch.abs(full[:, :, 0] + flip[:, :, 0]) + torch.abs(full[:, :, 1] - flip[:, :, 1])
           + torch.abs(full[:, :, 2] - flip[:, :, 2]))[:, _t(c['face_vertex_idx'])]
    taps, w, offsets, _ = fo.flip_plan(600, c['face_vertex_idx'], c['closest_faces'], c['bc'])
    same_bits(got[0], _n(ref), 'symmetry map against torch on the device (its three products are added in the header\'s order)')
    n = 1 + int(np.diff(offsets).max())
    mag = fo.sym_backward(c['p'], taps, w, c['g'], np.float64, magnitude=True)
    keep = np.broadcast_to(~fo.sym_ambiguous(c['p'], taps, w)[..., None], mag.shape)
    within(got[1], grad_of(ref, p, _t(c['g'])), (2 * K_Q_SYM + 2 * (n - 1)) * U * mag, keep, 'symmetry gradient (longest row %d)' % n)

    # pose: the stand-in's quaternion route on the device
    c = fo.pose_case(83, 64 * 55, special=False)
    got = run_pose(c)
    x = _t(c['out']).requires_grad_(True)
    ref = torch.abs(p3d_standins.axis_angle_to_matrix(x) - p3d_standins.axis_angle_to_matrix(_t(c['gt'])))
    within(got[0].reshape(-1, 9), _n(ref).reshape(-1, 9), np.full((64 * 55, 9), fo.POSE_K * U), np.ones((64 * 55, 9), bool), 'pose map')
    angle = np.linalg.norm(c['out'].astype(np.float64), axis=1)
    keep = ~fo.pose_ambiguous(c['out'], c['gt']) & (angle > POSE_ANGLES[0]) & (angle < POSE_ANGLES[1])
    bound = POSE_GRAD_K * U * np.abs(c['g'].astype(np.float64)).sum(1, keepdims=True)
    within(got[1].reshape(-1, 3), grad_of(ref, x, _t(c['g'].reshape(-1, 3, 3))), np.broadcast_to(bound, (64 * 55, 3)),
           np.broadcast_to(keep[:, None], (64 * 55, 3)), 'pose gradient')

    # the centred term: model.py:235-237
    c = fo.v2v_case(84, 3, 5023)
    got = run_v2v(c)
    a, t, w = _t(c['out']).requires_grad_(True), _t(c['target']), _t(c['weight'])
    ref = torch.abs((a - a.mean(1)[:, None, :]) - (t - t.mean(1)[:, None, :]).detach()) * w * 10
    within(got[0], _n(ref), fo.v2v_bound(c['out'], c['target'], c['weight']), np.ones(got[0].shape, bool), 'centred map')
    # the gradient: s is exact products of one rounding each (2 per side), its mean a sum of V terms in two orders
    s_mag = np.abs(c['g'].astype(np.float64) * c['weight'].astype(np.float64) * 10)
    bound = U * (4 * s_mag + (5023 + fo.v2v_depth(5023) + 2) * s_mag.mean(1, keepdims=True))
    # the ambiguous elements are left out one by one; a flipped sign among them still moves S of its whole (b, c) column
    # by 2 |s|, so every element's bound carries 2 sum_ambiguous |s| / V
    amb = fo.v2v_ambiguous(c['out'], c['target'])
    keep = ~amb
    bound = bound + 2 * np.where(amb, s_mag, 0).sum(1, keepdims=True) / 5023
    within(got[1], grad_of(ref, a, _t(c['g'])), bound, keep, 'centred gradient')


# ---- capture -----------------------------------------------------------------------------------------------------------------
def test_one_captured_graph_replays_the_eager_bits():
    ce, cs, cp, cv = fo.edge_case(91, 2, 1000, 1990), fo.sym_case(92, 2, 600, 300, hub=80), fo.pose_case(93, 2 * 55), \
        fo.v2v_case(94, 2, 5023)
    me, ms, mp = exa.EdgeLengthLoss(ce['face']), sym_module(cs).to(DEV), exa.PoseLoss()
    xs = [_t(ce['out']), _t(cs['p']), _t(cp['out']), _t(cv['out'])]
    for x in xs:
        x.requires_grad_(True)
    const = {'gt': _t(ce['gt']), 'valid': _t(ce['valid']), 'pose_gt': _t(cp['gt']), 'target': _t(cv['target']),
             'weight': _t(cv['weight'])}
    cot = [_t(ce['g']), _t(cs['g']), _t(cp['g'].reshape(1, -1, 3, 3)), _t(cv['g'])]

    def step():
        ys = [me(xs[0], const['gt'], const['valid']), ms(xs[1]), mp(xs[2][None], const['pose_gt'][None]),
              exa.centered_v2v_loss(xs[3], const['target'], const['weight'])]
        return tuple(ys) + torch.autograd.grad(ys, xs, cot)

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
        xs[1].add_(0.001)
        xs[2].copy_(xs[2].flip(0))
        xs[3].mul_(-0.5)
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    for i, (got, want) in enumerate(zip(outs, eager)):
        same_bits(_n(got), _n(want), 'replayed output %d' % i)
    same_bits(_n(outs[0]), fo.edge_forward(_n(xs[0]), ce['gt'], fo.valid_rows(ce), ce['face']), 'replayed edge map against the oracle')


# ---- the golden on the device ------------------------------------------------------------------------------------------------
def test_the_references_own_run_on_the_device(golden_dir):
    from tests import test_fit_oracle as tfo
    g = dict(np.load(os.path.join(golden_dir, 'ref_fit_terms.npz')))
    c = lambda name: {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + '_')}      # noqa: E731
    pc = c('pose')
    results = {'edge': run_edge(c('edge')), 'sym': run_sym(c('sym')), 'pose': run_pose(pc), 'v2v': run_v2v(c('v2v'))[:2]}
    for name, (loss, grad) in results.items():
        ref32, ref64, gref32, gref64 = (g[name + k] for k in ('_loss32', '_loss64', '_grad32', '_grad64'))
        _, _, bound, amb = tfo.oracle(name, g, np.float32)
        loss, grad = loss.reshape(ref32.shape), grad.reshape(gref32.shape)
        diff = np.abs(loss.astype(np.float64) - ref32)
        assert (diff <= bound).all(), '%s map: worst excess over the derived bound %g' % (name, float((diff - bound).max()))
        e, e_ref = np.abs(loss - ref64).max(), np.abs(ref32 - ref64).max()
        keep = ~amb
        ge, ge_ref = np.abs(grad - gref64)[keep].max(), np.abs(gref32 - gref64)[keep].max()
        print('%s: map error / reference error %.2f, gradient %.2f' % (name, e / max(e_ref, 1e-300), ge / max(ge_ref, 1e-300)))
        if name in tfo.BIT_EQUAL_MAPS:
            same_bits(loss, ref32, name + ' map against the reference float32 run')
        assert tfo.meets_the_bar(e, e_ref) and tfo.meets_the_bar(ge, ge_ref), (name, e, e_ref, ge, ge_ref)
