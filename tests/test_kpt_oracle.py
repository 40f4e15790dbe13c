"""The keypoint oracle (tests/kpt_oracle.py) against the reference's own run (tests/golden/ref_keypoints.npz, written by
tests/golden/make_golden_keypoints.py from the reference's functions and ``CoordLoss`` executed on the CPU in float32 and in
float64): the discrete decisions -- yaw bins, selected faces, ``hand_w`` -- EXACTLY, the values and gradients within 4x the
reference's own float32-against-float64 error, floored at 2^-24 of the norm (the project's standing bar; the measured ratios
are printed and recorded in DESIGN.md section 8y).  The golden's margins and its coverage are asserted again here, from the
file's own numbers, so that every decision the tests hold is the reference's and none was left out."""
import os

import numpy as np
import pytest

from tests import kpt_oracle as ko

FACTOR = 4.0
U = ko.U


@pytest.fixture(scope='module')
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, 'ref_keypoints.npz')))


def spec_of(g):
    s = {k: g['kpt_' + k] for k in ('faces', 'extra', 'lmk_f', 'lmk_w', 'dyn_f', 'dyn_w', 'chain', 'append', 'kpt_idx')}
    s.update(V=int(g['kpt_V']), J=int(g['kpt_J']), root_idx=int(g['kpt_root_idx']), chain=[int(j) for j in g['kpt_chain']])
    return s


def layer_inputs(g):
    return {k: g['kpt_' + k] for k in ('vertices', 'joints', 'rot', 'trans', 'focal', 'princpt')}


def cotangents(g):
    return {k: g['kpt_' + k] for k in ('g_cam', 'g_proj', 'g_root', 'g_mesh')}


def meets_the_bar(got, ref32, ref64, what):
    """max |got - ref64| <= max(4 max |ref32 - ref64|, 2^-24 max |ref64|); prints the ratio to the reference's own error."""
    e, e_ref, norm = np.abs(got - ref64).max(), np.abs(ref32 - ref64).max(), np.abs(ref64).max()
    print('%s: error %.3e, reference float32 error %.3e (ratio %.2f), floor %.3e' % (what, e, e_ref, e / max(e_ref, 1e-300), U * norm))
    return e <= max(FACTOR * e_ref, U * norm)


def test_the_goldens_margins_and_coverage(golden):
    g = golden
    deg = g['kpt_deg_64']
    assert ko.deg_margin(deg).min() >= 1e-2
    Ls = g['kpt_lmk_f'].shape[0]
    bins = g['kpt_faces_sel_64'][:, Ls]             # dynamic_lmk_faces_idx[bin, 0] == bin
    assert np.array_equal(g['kpt_dyn_f'][:, 0], np.arange(ko.BINS)) and np.array_equal(bins, g['kpt_faces_sel_32'][:, Ls])
    assert 0 in bins and ((bins > 0) & (bins < 39)).any() and ((bins > 39) & (bins < 78)).any() and 39 in bins and 78 in bins
    assert ((deg > -0.5) & (deg < 0)).any() and (deg > 39.5).any() and (deg < -39.5).any()
    iou, depths, hw = g['coord_iou_64'], g['coord_depths_64'], g['coord_hand_w_64']
    lhand, rhand = g['coord_lhand'], g['coord_rhand']
    assert np.nanmin(np.abs(iou - 0.5)) >= 1e-3
    assert (np.abs(depths[:, 0] - depths[:, 1]) > 1e-4 * np.abs(depths).max(1)).all()
    d = g['coord_proj'].astype(np.float64) - g['coord_gt']
    tie = np.abs(d) <= 1e-5 * np.maximum(np.abs(g['coord_proj']), np.abs(g['coord_gt']))
    assert tie.sum() == 1 and d[tie][0] == 0, 'the planted exact tie and no other'
    lost_l, lost_r = hw[:, lhand[0]] == 0, hw[:, rhand[0]] == 0
    valid = g['coord_valid'][:, :, 0]
    assert lost_l.any() and lost_r.any() and not (lost_l & lost_r).any()
    quiet = ~(lost_l | lost_r)
    assert (quiet & (iou < 0.5)).any(), 'not firing for a low IoU'
    assert (quiet & ((valid[:, lhand].sum(1) == 0) | (valid[:, rhand].sum(1) == 0))).any(), 'a hand without a valid entry'
    assert (quiet & ((valid[:, lhand] > 0).sum(1) == 1) & (iou == 0)).any(), 'a single valid point: a zero-area box'
    assert np.array_equal(hw, g['coord_hand_w_32'])


def test_the_oracle_reproduces_the_references_bins_and_faces_exactly(golden):
    s, x = spec_of(golden), layer_inputs(golden)
    Ls = len(s['lmk_f'])
    for dtype in (np.float32, np.float64):
        bins = ko.yaw_bins(s, x['rot'], x['rot'].shape[0], dtype)
        assert np.array_equal(bins, golden['kpt_faces_sel_64'][:, Ls])
        assert np.array_equal(ko.selected_faces(s, bins), golden['kpt_faces_sel_64'])
    assert np.abs(ko.yaw_deg(x['rot'], s['chain'], np.float64) - golden['kpt_deg_64']).max() < 1e-4      # rot is the float32 run's


@pytest.mark.parametrize('root_rel', [False, True])
def test_the_oracle_meets_the_references_own_run(golden, root_rel):
    g, s, x, cot = golden, spec_of(golden), layer_inputs(golden), cotangents(golden)
    tag = 'rel' if root_rel else ''
    out = ko.forward(s, x['vertices'], x['joints'], x['rot'], x['trans'], x['focal'], x['princpt'], root_rel=root_rel)
    grads = ko.backward(s, x['vertices'], x['joints'], out['yaw_bin'], x['trans'], x['focal'], x['princpt'], root_rel, **cot)
    got = {'kpt_cam': out['kpt_cam'], 'mesh_cam': out['mesh_cam'], 'd_trans': grads[2]}
    if not root_rel:
        got.update(root_cam=out['root_cam'], kpt_proj=out['kpt_proj'], d_vertices=grads[0], d_joints=grads[1])
        full = ko.forward(dict(s, kpt_idx=None), x['vertices'], x['joints'], x['rot'], want_mesh=False)
        root = full['root_cam'][:, None, :]
        # joints_full: the raw rows (cam = raw - root without trans; the oracle's rows are copies or the stated landmark sum)
        assert meets_the_bar(full['kpt_cam'], g['kpt_joints_full_32'] - root, g['kpt_joints_full_64'] - root, 'joints_full')
    for name, v in got.items():
        assert v.dtype == np.float32
        assert meets_the_bar(v, g['kpt_%s_%s32' % (name, tag)], g['kpt_%s_%s64' % (name, tag)], name + (' (root_rel)' if root_rel else '')), name


def test_the_coord_oracle_reproduces_hand_w_exactly_and_meets_the_references_run(golden):
    g = golden
    hands = (list(g['coord_lhand']), list(g['coord_rhand']), int(g['coord_wrists'][0]), int(g['coord_wrists'][1]))
    c = {k: g['coord_' + k] for k in ('proj', 'gt', 'valid', 'cam', 'weight', 'g')}
    for dtype in (np.float32, np.float64):
        loss, hw = ko.coord_forward(c['proj'], c['gt'], c['valid'], c['cam'], *hands, dtype=dtype)
        assert np.array_equal(hw, g['coord_hand_w_64']), 'hand_w in %s' % dtype
    assert meets_the_bar(loss := ko.coord_forward(c['proj'], c['gt'], c['valid'], c['cam'], *hands)[0], g['coord_loss_32'],
                         g['coord_loss_64'], 'coord loss')
    print('coord loss bit-equal to the reference float32 run:', np.array_equal(loss, g['coord_loss_32']))
    weighted, hw = ko.coord_forward(c['proj'], c['gt'], c['valid'], c['cam'], *hands, weight=c['weight'])
    assert meets_the_bar(weighted, g['coord_weighted_32'], g['coord_weighted_64'], 'coord loss * weight')
    grad = ko.coord_backward(c['proj'], c['gt'], c['valid'], hw, c['g'], weight=c['weight'])
    assert meets_the_bar(grad, g['coord_grad_32'], g['coord_grad_64'], 'coord gradient')
    assert grad[0, 7, 1] == 0, 'sign(0) = 0 at the planted tie'
    lose, iou, depths = ko.coord_rule(c['proj'], c['valid'], c['cam'], hands[0], hands[1], np.float64)
    fired = ~np.isnan(g['coord_iou_64'])
    assert np.array_equal(np.isnan(iou), ~fired) and np.abs(iou[fired] - g['coord_iou_64'][fired]).max() < 1e-9
    assert np.abs(depths - g['coord_depths_64']).max() < 1e-12


def test_the_bin_rule_at_its_edges():
    deg = np.array([-0.5, -1.5, 39.5, -39.4, -39.6, -40.5, 0.5, 1.5, 38.5, 39.0, 200.0, -200.0, np.nan, np.inf, -np.inf, -0.0,
                    -38.5, -39.5], np.float32)
    assert ko.bin_of(deg).tolist() == [0, 41, 39, 78, 78, 78, 0, 2, 38, 39, 39, 78, 0, 0, 0, 0, 77, 78]
