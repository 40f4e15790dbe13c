"""Developer check (CPU, numpy float32): the row-interval footprint arithmetic of csrc/binning.hip (rows_mask; the model is
tests/footprint_oracle.py model_cell_masks) against the per-pixel alpha rule evaluated by brute force on one 64x64 cell -- no
reached sub-tile may be missed ("bad" must be 0); "kept" vs "exact(pixel)" shows how tight the test is, "box" what the bounding
rect alone keeps.  python tools/footprint_check.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import footprint_oracle as fo                                                # noqa: E402

rng = np.random.default_rng(0)
f32 = np.float32
LOG2E = f32(1.4426950408889634)
def run(N, big):
    recs = []; truths = []; what = []
    for it in range(N):
        # random covariance (with the 0.3 low-pass), opacity, centre
        s1 = np.exp(rng.uniform(np.log(0.3), np.log(60.0 if big else 6.0))); s2 = np.exp(rng.uniform(np.log(0.3), np.log(60.0 if big else 6.0)))
        th = rng.uniform(0, np.pi)
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        cov = R @ np.diag([s1 * s1, s2 * s2]) @ R.T + 0.3 * np.eye(2)
        a, b, c = cov[0, 0], cov[0, 1], cov[1, 1]
        det = a * c - b * b
        ca, cb, cc = c / det, -b / det, a / det
        op = rng.uniform(0.01, 1.0) if rng.uniform() < 0.5 else 1.0
        if 255 * op < 1: continue
        px, py = rng.uniform(0, 64, 2)
        A = f32(-0.5) * LOG2E * f32(ca); B = -LOG2E * f32(cb); C = f32(-0.5) * LOG2E * f32(cc)
        px = f32(px); py = f32(py)
        # brute force per pixel (float32, same formula as the kernels), over an 8x8 grid of sub-tiles = one cell
        X = np.arange(64, dtype=np.float32); Y = np.arange(64, dtype=np.float32)
        dx = (px - X)[None, :]; dy = (py - Y)[:, None]
        p2 = (A * dx) * dx + ((C * dy) * dy + (B * dx) * dy)
        alpha = np.minimum(f32(0.99), f32(op) * np.exp2(p2.astype(np.float32)))
        ok = (alpha >= f32(1 / 255.)) & (p2 <= 0)
        truth = ok.reshape(8, 8, 8, 8).any(axis=(1, 3))        # [sub y, sub x]
        # bounding box (what preprocess gives), in sub-tiles, clipped to the cell
        tau2 = 2 * np.log(255 * op) + 1e-3
        ex = np.sqrt(tau2 * a) * 1.001 + 0.01; ey = np.sqrt(tau2 * c) * 1.001 + 0.01
        x0 = max(int(np.floor((px - ex) / 8)), 0); x1 = min(int(np.floor(np.ceil(px + ex) / 8)) + 1, 8)
        y0 = max(int(np.floor((py - ey) / 8)), 0); y1 = min(int(np.floor(np.ceil(py + ey) / 8)) + 1, 8)
        if x1 <= x0 or y1 <= y0: continue
        recs.append((px, py, 1, A, B, C, f32(op), x0, x1, y0, y1)); truths.append(truth); what.append((it, s1, s2, th, op, px, py))
    # ---- row-interval method in float32: the model of make_footprint / footprint_band / rows_mask, one cell at the origin ----
    rec = fo.pack(*(np.array(col) for col in zip(*recs)))
    g = np.arange(len(rec)); zero = np.zeros(len(rec), np.int64)
    masks = fo.model_cell_masks(rec, g, zero, zero)
    r = fo.unpack(rec)
    bad = 0
    for k in range(len(rec)):
        miss = truths[k] & ~masks[k]
        # truth outside the rect cannot happen if the rect is right
        if miss.any(): bad += 1; print('MISS', *what[k], np.argwhere(miss)[:3])
    kept = masks.sum(); exact = np.sum(truths); box = r['n_inst'].sum()
    print('N', N, 'big', big, 'bad', bad, 'box', box, 'kept', kept, 'exact(pixel)', exact)
run(4000, False)
run(3000, True)
