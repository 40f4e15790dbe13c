"""Which (Gaussian, 8x8 sub-tile) pairs MUST, MAY and MUST NOT enter a sub-tile list: the per-pixel alpha rule in float64.

THIS IS TEST INFRASTRUCTURE (numpy only: no torch device, no library), like tests/decision_oracle.py.  The binning chain
(csrc/preprocess_fwd.hip: sub-tile rect; csrc/common.h make_footprint / footprint_band and csrc/binning.hip rows_mask: exact
footprint) decides membership with hardware reciprocals, square roots and hand-picked relaxations.  The rule it has to imply
is "a sub-tile is dropped only if none of its 64 pixel centres passes alpha >= 1/255".  Here that rule is evaluated per pixel,
in float64, on the float32 words of the 64-byte ``Splat`` records the kernels themselves read (a (P, 16) uint32 array:
px, py, flags, radius | ca, cb, cc, opacity | r, g, b, depth | sub_x, sub_y, n_inst, inst_off), so that nothing of the
float32 preprocess can excuse a difference.

    power2 = ca dx^2 + cb dx dy + cc dy^2      (conic pre-scaled by log2 e;  dx, dy = integer pixel centre - (px, py))
    alpha  = opacity * 2^power2
    mag    = |ca| dx^2 + |cb| |dx dy| + |cc| dy^2

Classes of a pair (``classify``), over every sub-tile of upstream's 16x16-tile rect of the splat (raster_oracle.preprocess step
7, from the record's radius and centre) that holds an image pixel; ``in_rect`` says which of them the record's rect holds:

MUST      some pixel of the sub-tile, inside the image and inside upstream's tile rect, has power2 <= 0 and
          alpha >= (1 + d) / 255 with d = 1e-6 (1 + mag).  Derivation of d: the kernels evaluate power2 in float32 as three
          products and two fmas (common.h gauss_power2), at most about 4 ulp of mag = 2.4e-7 mag absolute in the log2 domain,
          which is ln 2 * 2.4e-7 mag = 1.7e-7 mag relative in alpha; exp2 and the opacity product add about 2e-7 relative.
          d is a little over four times the sum 2e-7 + 1.7e-7 mag.  A pixel that passes by more than d passes in every
          legitimate float32 evaluation, so the pair has to be listed.
BAND      not MUST, but some such pixel has alpha >= (1 - d) / 255: either decision is legitimate float32 rounding.  (d is the
          linearisation of a log2-domain error of 1.44e-6 (1 + mag); where mag exceeds 1e6 -- a pixel thousands of px along a
          needle -- 1 - d is negative and BAND says nothing.  MUST_NOT, whose own relaxation 2e-5 mag_cell >= 2e-5 mag is above
          that log2-domain error, takes precedence over BAND.)
MUST_NOT  (inside the rect only; only for splats the kernel tests at all: ca < 0, cc < 0, ca - cb^2 / (4 cc) < 0, all
          finite -- every other splat has none.)  The sub-tile's pixel-centre hull [x0, x0 + 7] x [y0, y0 + 7] relative to the
          centre, widened in x by 2e-3 (1 + Xf) where Xf is the half extent in x of the relaxed ellipse (it bounds |xa| and
          |xb| of rows_mask), holds no point with power2 >= -log2(255 o) - 2 (1e-3 + 1e-5 mag_cell): the maximum of the
          concave quadratic over that box (closed form: 0 if the box holds the centre, otherwise the best of the four
          edges) is below that threshold.  mag_cell is make_footprint's own ``mag`` for the pair's cell (xm, ym from the rect
          clipped to the cell, as rows_mask does it).  This is TWICE the kernel's documented relaxations (1e-3 + 1e-5 mag
          on the threshold, 1e-3 (1 + |x|) px on the interval): a pair the device lists although it is MUST_NOT was kept
          by something other than those relaxations.
MAY       everything else inside the rect (the ellipse cuts the hull between pixel centres, or only the relaxations reach).

``model_mask`` is a float32 numpy re-statement of make_footprint, footprint_band and rows_mask (one mask per (splat, cell)),
the designed arithmetic without the hardware's approximate reciprocal / square root / log2.  tools/footprint_check.py runs it
against a brute-force per-pixel rule; tests/test_footprint_oracle.py checks MUST <= model_mask and model_mask & MUST_NOT = 0.
"""
import numpy as np

SUB, CELL_SUBS, TILE = 8, 8, 16
MAY, MUST, BAND, MUST_NOT = 0, 1, 2, 3
CLASS_NAMES = ('MAY', 'MUST', 'BAND', 'MUST_NOT')
f32 = np.float32


def unpack(rec):
    """Fields of (P, 16) uint32 records."""
    rec = np.ascontiguousarray(rec, dtype=np.uint32).reshape(-1, 16)
    fl = rec.view(np.float32)
    return dict(px=fl[:, 0], py=fl[:, 1], radius=rec[:, 3].view(np.int32), ca=fl[:, 4], cb=fl[:, 5], cc=fl[:, 6], op=fl[:, 7],
                sx0=(rec[:, 12] & 0xffff).astype(np.int64), sx1=(rec[:, 12] >> 16).astype(np.int64),
                sy0=(rec[:, 13] & 0xffff).astype(np.int64), sy1=(rec[:, 13] >> 16).astype(np.int64),
                n_inst=rec[:, 14].astype(np.int64))


def pack(px, py, radius, ca, cb, cc, op, sx0, sx1, sy0, sy1, depth=None):
    """(P, 16) uint32 records from their fields (what preprocess_fwd.hip stores; colour and flags zero)."""
    P = len(px)
    rec = np.zeros((P, 16), np.uint32)
    fl = rec.view(np.float32)
    fl[:, 0], fl[:, 1], fl[:, 4], fl[:, 5], fl[:, 6], fl[:, 7] = px, py, ca, cb, cc, op
    if depth is not None:
        fl[:, 11] = depth
    rec[:, 3] = np.asarray(radius, np.int64).astype(np.int32).view(np.uint32)
    sx0, sx1, sy0, sy1 = (np.asarray(v, np.int64) for v in (sx0, sx1, sy0, sy1))
    rec[:, 12] = (sx0 | (sx1 << 16)).astype(np.uint32)
    rec[:, 13] = (sy0 | (sy1 << 16)).astype(np.uint32)
    rec[:, 14] = ((sx1 - sx0) * (sy1 - sy0)).astype(np.uint32)
    return rec


def grid(H, W):
    return dict(gx=(W + 15) // 16, gy=(H + 15) // 16, sx=(W + 7) // 8, sy=(H + 7) // 8, cx=(W + 63) // 64, cy=(H + 63) // 64)


def pair_key(g, sx, sy, H, W):
    """One integer per (Gaussian, sub-tile) pair; sub-tile coordinates over the padded grid of whole cells."""
    gr = grid(H, W)
    return (np.asarray(g, np.int64) * (gr['cy'] * 8) + np.asarray(sy, np.int64)) * (gr['cx'] * 8) + np.asarray(sx, np.int64)


def _boxes(lo_x, hi_x, lo_y, hi_y):
    """All (g, x, y) with lo_x[g] <= x < hi_x[g], lo_y[g] <= y < hi_y[g]: g ascending, then y, then x."""
    nx, ny = np.maximum(hi_x - lo_x, 0), np.maximum(hi_y - lo_y, 0)
    n = nx * ny
    g = np.repeat(np.arange(len(n)), n)
    k = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
    nxg = np.maximum(nx[g], 1)
    return g, lo_x[g] + k % nxg, lo_y[g] + k // nxg


def rect_pairs(rec, H, W):
    """The pairs of the records' sub-tile rects (g, sx, sy), Gaussian-major, rows of the rect, then columns."""
    r = unpack(rec)
    live = r['n_inst'] > 0
    z = np.zeros_like(r['sx0'])
    return _boxes(np.where(live, r['sx0'], z), np.where(live, r['sx1'], z), np.where(live, r['sy0'], z), np.where(live, r['sy1'], z))


def tile_rect(rec, H, W):
    """Upstream's 16x16-tile rect (x0, x1, y0, y1; exclusive upper) from the record's radius and centre: float32, C
    truncation, clamped to the grid (raster_oracle.preprocess step 7).  Empty for radius <= 0."""
    r, gr = unpack(rec), grid(H, W)
    rf = r['radius'].astype(f32)
    big = f32(1 << 20)

    def tr(t, hi):
        with np.errstate(invalid='ignore'):
            t = np.where(np.isnan(t), f32(0), np.clip(t, -big, big))
        return np.clip(np.trunc(t).astype(np.int64), 0, hi)
    with np.errstate(invalid='ignore', over='ignore'):
        x0, x1 = tr((r['px'] - rf) / f32(TILE), gr['gx']), tr(((r['px'] + rf) + f32(TILE - 1)) / f32(TILE), gr['gx'])
        y0, y1 = tr((r['py'] - rf) / f32(TILE), gr['gy']), tr(((r['py'] + rf) + f32(TILE - 1)) / f32(TILE), gr['gy'])
    dead = (r['radius'] <= 0) | (x1 <= x0) | (y1 <= y0)
    z = np.zeros_like(x0)
    return np.where(dead, z, x0), np.where(dead, z, x1), np.where(dead, z, y0), np.where(dead, z, y1)


def _quad_max(A, B, C, xl, xh, yl, yh):
    """Maximum of the concave A x^2 + B x y + C y^2 (A, C < 0, 4AC > B^2) over the box: 0 at the centre if the box holds it,
    otherwise on the boundary -- per edge the 1-D parabola's vertex clamped to the edge."""
    q = lambda x, y: A * x * x + B * x * y + C * y * y                                   # noqa: E731
    best = np.full(A.shape, -np.inf)
    for c in (xl, xh):
        best = np.maximum(best, q(c, np.clip(-B * c / (2 * C), yl, yh)))
    for c in (yl, yh):
        best = np.maximum(best, q(np.clip(-B * c / (2 * A), xl, xh), c))
    inside = (xl <= 0) & (xh >= 0) & (yl <= 0) & (yh >= 0)
    return np.where(inside, 0.0, best)


def _cell_mag(r, g, sx, sy, f=np.float64):
    """make_footprint's ``mag`` for the cell of pair (g, sx, sy): xm, ym from the rect clipped to the cell (rows_mask)."""
    out = []
    for s, lo, hi, c in ((sx, r['sx0'], r['sx1'], r['px']), (sy, r['sy0'], r['sy1'], r['py'])):
        c0 = (s // CELL_SUBS) * CELL_SUBS
        a0, a1 = np.maximum(lo[g] - c0, 0), np.minimum(hi[g] - c0, CELL_SUBS)
        l0 = ((c0 + a0) * SUB).astype(f) - c[g].astype(f)
        out.append(np.maximum(np.abs(l0), np.abs(l0 + ((a1 - a0) * SUB).astype(f))))
    xm, ym = out
    A, B, C = (np.abs(r[k][g].astype(f)) for k in ('ca', 'cb', 'cc'))
    return A * xm * xm + B * xm * ym + C * ym * ym


def classify(rec, H, W, chunk=1 << 16):
    """Classes of every pair of the splats' upstream tile rects (see the module docstring).

    Returns a dict of equally long arrays: g, sx, sy, key (``pair_key``), in_rect (bool: inside the record's sub-tile rect) and
    cls (MAY / MUST / BAND / MUST_NOT; outside the rect only MUST and BAND mean anything -- MAY stands for "not reached")."""
    r, gr = unpack(rec), grid(H, W)
    tx0, tx1, ty0, ty1 = tile_rect(rec, H, W)
    g, sx, sy = _boxes(2 * tx0, np.minimum(2 * tx1, gr['sx']), 2 * ty0, np.minimum(2 * ty1, gr['sy']))
    live = r['n_inst'][g] > 0
    in_rect = live & (sx >= r['sx0'][g]) & (sx < r['sx1'][g]) & (sy >= r['sy0'][g]) & (sy < r['sy1'][g])
    # the record's rect lies inside the tile rect by construction; if a record says otherwise, its pairs are judged too
    rg_, rsx, rsy = rect_pairs(rec, H, W)
    extra = ~np.isin(pair_key(rg_, rsx, rsy, H, W), pair_key(g, sx, sy, H, W)[in_rect])
    g, sx, sy = np.concatenate([g, rg_[extra]]), np.concatenate([sx, rsx[extra]]), np.concatenate([sy, rsy[extra]])
    in_rect = np.concatenate([in_rect, np.ones(int(extra.sum()), bool)])
    N = len(g)
    cls = np.zeros(N, np.int8)
    d64 = lambda k, i: r[k][i].astype(np.float64)                                       # noqa: E731
    off = np.arange(SUB, dtype=np.int64)
    with np.errstate(all='ignore'):
        for b in range(0, N, chunk):
            i = g[b:b + chunk]
            X = (sx[b:b + chunk] * SUB)[:, None, None] + off[None, None, :]
            Y = (sy[b:b + chunk] * SUB)[:, None, None] + off[None, :, None]
            ok = ((X < W) & (Y < H) & (X >= TILE * tx0[i][:, None, None]) & (X < TILE * tx1[i][:, None, None])
                  & (Y >= TILE * ty0[i][:, None, None]) & (Y < TILE * ty1[i][:, None, None]))
            dx, dy = X - d64('px', i)[:, None, None], Y - d64('py', i)[:, None, None]
            A, B, C = (d64(k, i)[:, None, None] for k in ('ca', 'cb', 'cc'))
            p2 = A * dx * dx + B * dx * dy + C * dy * dy
            mag = np.abs(A) * dx * dx + np.abs(B) * np.abs(dx * dy) + np.abs(C) * dy * dy
            alpha = d64('op', i)[:, None, None] * np.exp2(p2)
            d = 1e-6 * (1.0 + mag)
            ok = ok & (p2 <= 0)
            must = (ok & (alpha >= (1 + d) / 255)).any((1, 2))
            band = (ok & (alpha >= (1 - d) / 255)).any((1, 2)) & ~must
            cls[b:b + chunk] = np.where(must, MUST, np.where(band, BAND, MAY))
        # MUST_NOT: inside the rect, tested splats only
        A, B, C, o = d64('ca', g), d64('cb', g), d64('cc', g), d64('op', g)
        As = A - B * B / (4 * C)
        tested = np.isfinite(A) & np.isfinite(B) & np.isfinite(C) & np.isfinite(o) & (A < 0) & (C < 0) & (As < 0) & np.isfinite(As)
        thr = -np.log2(255.0 * o) - 2 * (1e-3 + 1e-5 * _cell_mag(r, g, sx, sy))
        Xf = np.sqrt(np.maximum(thr / As, 0.0))
        wide = 2e-3 * (1.0 + Xf)
        xl, yl = sx * SUB - d64('px', g), sy * SUB - d64('py', g)
        qmax = _quad_max(A, B, C, xl - wide, xl + (SUB - 1) + wide, yl, yl + (SUB - 1))
        must_not = in_rect & tested & np.isfinite(thr) & (qmax < thr)
    assert not (must_not & (cls == MUST)).any(), 'a pair is both reached and unreachable: the bounds of this oracle cross'
    cls[must_not] = MUST_NOT                                     # (over BAND: see the module docstring)
    return dict(g=g, sx=sx, sy=sy, key=pair_key(g, sx, sy, H, W), in_rect=in_rect, cls=cls)


def counts(c):
    """rect, MUST, BAND, MAY, MUST_NOT (inside the rect) and the reached pairs outside it."""
    r = c['in_rect']
    out = {'rect': int(r.sum())}
    for k, name in enumerate(CLASS_NAMES):
        out[name] = int((r & (c['cls'] == k)).sum())
    out['reached_outside_rect'] = int((~r & (c['cls'] == MUST)).sum())
    return out


# ---- float32 model of make_footprint / footprint_band / rows_mask ----

def _clampf(v, lo, hi):
    return np.minimum(np.maximum(v, lo), hi)


def cell_entries(rec, H, W):
    """(g, cx, cy) of every cell a live rect overlaps."""
    r = unpack(rec)
    live = r['n_inst'] > 0
    z = np.zeros_like(r['sx0'])
    c = lambda lo, hi: (np.where(live, lo // CELL_SUBS, z), np.where(live, (hi - 1) // CELL_SUBS + 1, z))   # noqa: E731
    (cx0, cx1), (cy0, cy1) = c(r['sx0'], r['sx1']), c(r['sy0'], r['sy1'])
    return _boxes(cx0, cx1, cy0, cy1)


def model_cell_masks(rec, g, cx, cy, footprint=True):
    """rows_mask for entries (g, cell cx, cy): bool (E, 8, 8) [row y, column x of the cell], float32 operation by operation."""
    r = unpack(rec)
    csx0, csy0 = cx * CELL_SUBS, cy * CELL_SUBS
    x0, x1 = np.maximum(r['sx0'][g] - csx0, 0), np.minimum(r['sx1'][g] - csx0, CELL_SUBS)
    y0, y1 = np.maximum(r['sy0'][g] - csy0, 0), np.minimum(r['sy1'][g] - csy0, CELL_SUBS)
    cols, rows = np.arange(CELL_SUBS)[None, None, :], np.arange(CELL_SUBS)[None, :, None]
    in_rows = (rows >= y0[:, None, None]) & (rows < y1[:, None, None])
    whole = in_rows & (cols >= x0[:, None, None]) & (cols < x1[:, None, None])
    if not footprint:
        return whole
    with np.errstate(all='ignore'):
        A, B, C, op = r['ca'][g], r['cb'][g], r['cc'][g], r['op'][g]
        xl0 = ((csx0 + x0) * SUB).astype(f32) - r['px'][g]
        yl0 = ((csy0 + y0) * SUB).astype(f32) - r['py'][g]
        xm = np.maximum(np.abs(xl0), np.abs(xl0 + ((x1 - x0) * SUB).astype(f32)))
        ym = np.maximum(np.abs(yl0), np.abs(yl0 + ((y1 - y0) * SUB).astype(f32)))
        # make_footprint
        rA, rC = f32(1) / A, f32(1) / C
        As = A - f32(0.25) * B * B * rC
        test = (A < 0) & (C < 0) & (As < 0)
        mag = np.abs(A) * xm * xm + np.abs(B) * xm * ym + np.abs(C) * ym * ym
        thr = -np.log2(f32(255.0) * op) - f32(1e-3) - f32(1e-5) * mag
        kA = f32(-0.5) * B * rA
        ysr = f32(-0.5) * B * rC * np.sqrt(thr * (f32(1) / As))
        X2 = thr * rA
        D4 = C * As * rA * rA
        # footprint_band, per row of sub-tiles
        e = lambda v: v[:, None]                                                        # noqa: E731
        yl = e(yl0) + ((np.arange(CELL_SUBS)[None, :] - e(y0)) * SUB).astype(f32)
        yh = yl + f32(SUB - 1)
        yR, yL = _clampf(e(ysr), yl, yh), _clampf(-e(ysr), yl, yh)
        hR2, hL2 = e(X2) - e(D4) * yR * yR, e(X2) - e(D4) * yL * yL
        miss = (hR2 < 0) | (hL2 < 0)
        xb, xa = e(kA) * yR + np.sqrt(hR2), e(kA) * yL - np.sqrt(hL2)
        # rows_mask
        ordered = xa <= xb                                                              # (NaN: keep the row)
        m = f32(1e-3) * (f32(1) + np.maximum(np.abs(xa), np.abs(xb)))
        lo = _clampf((xa - m - f32(SUB - 1) - e(xl0)) * f32(1.0 / SUB), f32(-1.0e6), f32(1.0e6))
        hi = _clampf((xb + m - e(xl0)) * f32(1.0 / SUB), f32(-1.0e6), f32(1.0e6))
        c0 = np.where(ordered, np.maximum(e(x0), e(x0) + np.ceil(np.where(ordered, lo, 0)).astype(np.int64)), e(x0))
        c1 = np.where(ordered, np.minimum(e(x1) - 1, e(x0) + np.floor(np.where(ordered, hi, 0)).astype(np.int64)), e(x1) - 1)
    tested = in_rows & ~miss[:, :, None] & (cols >= c0[:, :, None]) & (cols <= c1[:, :, None])
    return np.where(test[:, None, None], tested, whole)


def model_mask(rec, H, W, footprint=True):
    """bool per pair of ``rect_pairs``: the pairs the designed float32 arithmetic keeps."""
    gr = grid(H, W)
    g, cx, cy = cell_entries(rec, H, W)
    masks = model_cell_masks(rec, g, cx, cy, footprint)
    ekey = (g * gr['cy'] + cy) * gr['cx'] + cx                       # ascending in g; look pairs up by (g, cell)
    order = np.argsort(ekey, kind='stable')
    pg, sx, sy = rect_pairs(rec, H, W)
    e = order[np.searchsorted(ekey[order], (pg * gr['cy'] + sy // CELL_SUBS) * gr['cx'] + sx // CELL_SUBS)]
    return masks[e, sy % CELL_SUBS, sx % CELL_SUBS]


# ---- judging lists: assertions on plain arrays (a list is the set of keys of its pairs: pair_key), shared by the GPU test,
# which feeds them the device's lists, and the CPU test, which feeds them the model's and deliberately broken models' ----

def listed_pairs(rg, ids, H, W):
    """(g, sx, sy) of every list entry, from the cell-major ranges and the concatenated sorted ids."""
    gcx = grid(H, W)['cx']
    n = np.maximum(rg[:, 1].astype(np.int64) - rg[:, 0], 0)
    st = np.repeat(np.arange(len(rg)), n)
    cell, local = st // 64, st % 64
    return ids.astype(np.int64), (cell % gcx) * 8 + (local & 7), (cell // gcx) * 8 + (local >> 3)


def assert_well_formed(rec, rg, ids, cap, H, W):
    r, gr = unpack(rec), grid(H, W)
    assert len(rg) == gr['cx'] * gr['cy'] * 64
    b, e = rg[:, 0].astype(np.int64), rg[:, 1].astype(np.int64)
    assert (e >= b).all()
    full = e > b
    assert (b[full] % 64 == 0).all() and (e[full] <= cap).all()
    o = np.argsort(b[full], kind='stable')
    assert (b[full][o][1:] >= e[full][o][:-1]).all(), 'ranges overlap'
    st = np.arange(len(rg))
    sx, sy = ((st // 64) % gr['cx']) * 8 + (st & 7), ((st // 64) // gr['cx']) * 8 + ((st & 63) >> 3)
    assert not full[(sx * 8 >= W) | (sy * 8 >= H)].any(), 'a padding sub-tile has a list'
    g, lx, ly = listed_pairs(rg, ids, H, W)
    assert len(g) == (e - b).sum()
    assert (g < len(rec)).all()
    key = pair_key(g, lx, ly, H, W)
    assert len(np.unique(key)) == len(key), 'an id occurs twice in a list'
    assert (r['radius'][g] > 0).all() and (r['n_inst'][g] > 0).all()
    assert ((lx >= r['sx0'][g]) & (lx < r['sx1'][g]) & (ly >= r['sy0'][g]) & (ly < r['sy1'][g])).all(), 'a listed pair lies outside its rect'
    return key


def _show(cl, m):
    return [(int(cl['g'][i]), int(cl['sx'][i]), int(cl['sy'][i])) for i in np.flatnonzero(m)[:8]]


def assert_nothing_reached_is_missing(cl, key):
    missing = (cl['cls'] == MUST) & ~np.isin(cl['key'], key)
    assert not missing.any(), '%d reached pairs (Gaussian, sub-tile x, y) are in no list: %s' % (missing.sum(), _show(cl, missing))


def assert_no_unreachable_pair_is_listed(cl, key):
    wrong = (cl['cls'] == MUST_NOT) & np.isin(cl['key'], key)
    assert not wrong.any(), '%d listed pairs (Gaussian, sub-tile x, y) are beyond twice the relaxations: %s' % (wrong.sum(), _show(cl, wrong))


def assert_lists_are_the_rects(rec, key, H, W):
    g, sx, sy = rect_pairs(rec, H, W)
    assert len(key) == unpack(rec)['n_inst'].sum() == len(g)
    assert np.array_equal(np.sort(key), np.sort(pair_key(g, sx, sy, H, W)))
