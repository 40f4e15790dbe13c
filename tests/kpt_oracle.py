"""CPU restatement of the keypoint path (include/exa_mesh.h, "KEYPOINTS" and "COORD LOSS"; csrc/keypoints.hip), operation by
operation in numpy: forward and backward of ``BodyKeypoints`` and ``CoordLoss``, plus the case generators the tests share.

A ``spec`` is a dict of the source arrays, as the module's constructor takes them: ``V``, ``J``, ``faces [F, 3]``, ``extra``,
``lmk_f [Ls]``, ``lmk_w [Ls, 3]``, ``dyn_f [79, Ld]``, ``dyn_w [79, Ld, 3]``, ``chain``, ``kpt_idx``, ``root_idx``, ``append``.
Nothing here reads the module's compiled tables: the rows are resolved from the source arrays again, and the backward adds
keypoint by keypoint in ascending (k, corner), which gives every vertex and joint the header's order.  Every function takes
``dtype``: float32 restates the kernels bit for bit (only the bin passes through ``sqrt`` / ``arctan2``, which the cases keep
a margin around; a landmark row's two fused multiply-adds are evaluated exactly, ``fma32``), float64 is the same
arithmetic for error measurements.
"""
import numpy as np

from tests import fit_oracle

F32 = np.float32
BINS = 79
U = 2.0 ** -24


def sign(x):
    return (x > 0).astype(x.dtype) - (x < 0).astype(x.dtype)


# ---- rows ---------------------------------------------------------------------------------------------------------------
def rows_of(spec):
    """The full list's rows as ('j', joint) / ('v', vertex) / ('s', lmk) / ('d', slot), then the selection + the root."""
    rows = [('j', j) for j in range(spec['J'])] + [('v', int(v)) for v in spec['extra']]
    rows += [('s', i) for i in range(len(spec['lmk_f']))] + [('d', s) for s in range(spec['dyn_f'].shape[1])]
    rows += [('v', int(v)) for v in spec['append']]
    idx = range(len(rows)) if spec['kpt_idx'] is None else spec['kpt_idx']
    return [rows[int(i)] for i in idx], rows[int(spec['root_idx'])]


def corners(spec, row, b_bin):
    """(vertices, weights) of a landmark row under yaw bin ``b_bin``."""
    kind, i = row
    if kind == 's':
        return spec['faces'][spec['lmk_f'][i]], spec['lmk_w'][i]
    return spec['faces'][spec['dyn_f'][b_bin, i]], spec['dyn_w'][b_bin, i]


def fma32(a, b, c):
    """``fmaf(a, b, c)`` of float32 arrays, exactly: the product is exact in float64, the sum's rounding error is recovered
    (two-sum) and folded in by rounding to odd, after which the rounding to float32 is the correct one."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(all='ignore'):
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        odd = (s.view(np.int64) & 1) == 1
        fix = (e != 0) & ~odd & np.isfinite(s) & np.isfinite(e)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def raw_row(spec, row, x, joints, b, b_bin, dt):
    kind, i = row
    if kind == 'j':
        return joints[b, i].copy()
    if kind == 'v':
        return x[b, i].copy()
    v, w = corners(spec, row, b_bin)
    w = w.astype(dt)
    if dt is np.float32:      # the header's row: one rounded product, two fused multiply-adds
        return fma32(x[b, v[2]], w[2], fma32(x[b, v[1]], w[1], x[b, v[0]] * w[0]))
    return (x[b, v[0]] * w[0] + x[b, v[1]] * w[1]) + x[b, v[2]] * w[2]


def yaw_deg(rot, chain, dtype=F32):
    """[B]: the header's deg."""
    dt = np.dtype(dtype).type
    rot = np.asarray(rot, dtype=dt)
    B = rot.shape[0]
    rel = np.tile(np.eye(3, dtype=dt), (B, 1, 1))
    with np.errstate(all='ignore'):
        for j in chain:
            R, new = rot[:, int(j)], np.zeros_like(rel)
            for r in range(3):
                for c in range(3):
                    new[:, r, c] = (R[:, r, 0] * rel[:, 0, c] + R[:, r, 1] * rel[:, 1, c]) + R[:, r, 2] * rel[:, 2, c]
            rel = new
        sy = np.sqrt(rel[:, 0, 0] * rel[:, 0, 0] + rel[:, 1, 0] * rel[:, 1, 0])
        a = np.arctan2(-rel[:, 2, 0], sy)
        pi = dt(np.float32(np.pi)) if dt is np.float32 else dt(np.pi)
        return (((-a) * dt(180.0)) / pi).astype(dt)


def bin_of(deg):
    """The header's bin rule, [B] int32."""
    out = np.zeros(deg.shape[0], np.int32)
    for b, d in enumerate(deg):
        if not np.isfinite(d):
            continue
        y = np.rint(min(d, type(d)(39)))
        n = int(y) if y >= 0 else (39 - int(y) if y >= -39 else 78)
        out[b] = min(max(n, 0), BINS - 1)
    return out


def yaw_bins(spec, rot, B, dtype=F32):
    if spec['dyn_f'].shape[1] == 0:
        return np.zeros(B, np.int32)
    return bin_of(yaw_deg(rot, spec['chain'], dtype))


def selected_faces(spec, bins):
    """[B, Ls + Ld]: the face of every landmark, as the reference's ``lmk_faces_idx`` after the ``cat``."""
    return np.stack([np.concatenate([spec['lmk_f'], spec['dyn_f'][b]]) for b in bins]).astype(np.int64)


# ---- BodyKeypoints ------------------------------------------------------------------------------------------------------
def _cam(spec, sel, root_row, x, joints, trans, b, b_bin, dt):
    root = raw_row(spec, root_row, x, joints, b, b_bin, dt)
    cam = np.zeros((len(sel), 3), dt)
    for k, row in enumerate(sel):
        cam[k] = raw_row(spec, row, x, joints, b, b_bin, dt) - root
        if trans is not None:
            cam[k] = cam[k] + trans[b]
    return root, cam


def forward(spec, vertices, joints, rot=None, trans=None, focal=None, princpt=None, root_rel=False, want_mesh=True, dtype=F32,
            bins=None):
    dt = np.dtype(dtype).type
    cast = lambda a: None if a is None else np.asarray(a, dtype=dt)      # noqa: E731
    x, joints, trans, focal, princpt = cast(vertices), cast(joints), cast(trans), cast(focal), cast(princpt)
    B = x.shape[0]
    sel, root_row = rows_of(spec)
    K = len(sel)
    bins = yaw_bins(spec, rot, B, dtype) if bins is None else bins
    out = {'kpt_cam': np.zeros((B, K, 3), dt), 'root_cam': np.zeros((B, 3), dt), 'yaw_bin': bins,
           'kpt_proj': None if focal is None else np.zeros((B, K, 2), dt), 'mesh_cam': None}
    if want_mesh:
        out['mesh_cam'] = np.zeros_like(x)
    with np.errstate(all='ignore'):
        for b in range(B):
            root, cam = _cam(spec, sel, root_row, x, joints, trans, b, bins[b], dt)
            out['root_cam'][b] = root
            if focal is not None:
                out['kpt_proj'][b] = ((cam[:, :2] / cam[:, 2:3]) * focal[b]) + princpt[b]
            out['kpt_cam'][b] = cam - trans[b] if root_rel and trans is not None else cam
            if want_mesh:
                m = x[b] - root
                if trans is not None:
                    m = m + trans[b]
                    if root_rel:
                        m = m - trans[b]
                out['mesh_cam'][b] = m
    return out


def backward(spec, vertices, joints, bins, trans=None, focal=None, princpt=None, root_rel=False, g_cam=None, g_proj=None,
             g_root=None, g_mesh=None, dtype=F32, magnitude=False):
    """(d_vertices, d_joints, d_trans or None).  ``magnitude``: every term by its absolute value (for error bounds)."""
    dt = np.dtype(dtype).type
    cast = lambda a: None if a is None else np.asarray(a, dtype=dt)      # noqa: E731
    x, joints, trans, focal, princpt = cast(vertices), cast(joints), cast(trans), cast(focal), cast(princpt)
    g_cam, g_proj, g_root, g_mesh = cast(g_cam), cast(g_proj), cast(g_root), cast(g_mesh)
    mag = np.abs if magnitude else (lambda a: a)
    B, V, J = x.shape[0], x.shape[1], joints.shape[1]
    sel, root_row = rows_of(spec)
    K = len(sel)
    dv = mag(g_mesh).copy() if g_mesh is not None else np.zeros_like(x)
    dj = np.zeros_like(joints)
    d_trans = None if trans is None else np.zeros((B, 3), dt)
    Sm = fit_oracle.sum2(mag(g_mesh)) if g_mesh is not None and V > 0 else np.zeros((B, 3), dt)
    with np.errstate(all='ignore'):
        for b in range(B):
            _, cam = _cam(spec, sel, root_row, x, joints, trans, b, bins[b], dt)
            p = np.zeros((K, 3), dt)
            if g_proj is not None:
                t = g_proj[b] * focal[b]
                q = cam[:, :2] / cam[:, 2:3]
                p[:, 0] = mag(t[:, 0] / cam[:, 2])
                p[:, 1] = mag(t[:, 1] / cam[:, 2])
                if magnitude:
                    p[:, 2] = np.abs((np.abs(t[:, 0] * q[:, 0]) + np.abs(t[:, 1] * q[:, 1])) / cam[:, 2])
                else:
                    p[:, 2] = -((t[:, 0] * q[:, 0] + t[:, 1] * q[:, 1]) / cam[:, 2])
            c = p if g_cam is None else (mag(g_cam[b]) + p if g_proj is not None else mag(g_cam[b]).copy())
            Sc, Sp = np.zeros(3, dt), np.zeros(3, dt)
            for k in range(K):
                Sc = Sc + c[k]
                Sp = Sp + p[k]
            g = mag(g_root[b]) if g_root is not None else np.zeros(3, dt)
            r_root = (g + Sc) + Sm[b] if magnitude else (g - Sc) - Sm[b]
            if d_trans is not None:
                d_trans[b] = Sp if root_rel else Sc + Sm[b]
            for k, row in enumerate(sel + [root_row]):
                r = c[k] if k < K else r_root
                if row[0] == 'j':
                    dj[b, row[1]] = dj[b, row[1]] + r
                elif row[0] == 'v':
                    dv[b, row[1]] = dv[b, row[1]] + dt(1.0) * r
                else:
                    v, w = corners(spec, row, bins[b])
                    for corner in range(3):
                        dv[b, v[corner]] = dv[b, v[corner]] + mag(dt(w[corner])) * r
    return dv, dj, d_trans


def depth_of(spec, V):
    """The additions a cotangent may pass through on its way into one output element: the K sequential ones, SUM2's, and the
    longest per-vertex / per-joint list (at most K + 1 records of three corners)."""
    K = len(rows_of(spec)[0])
    return K + fit_oracle.v2v_depth(max(V, 1)) + 3 * (K + 1) + 8


# ---- CoordLoss ----------------------------------------------------------------------------------------------------------
def _nmax(p, q):
    return p.dtype.type(np.nan) if (p != p or q != q) else (p if p > q else q)


def _nmin(p, q):
    return p.dtype.type(np.nan) if (p != p or q != q) else (p if p < q else q)


def _extend(lo_in, hi_in, dt):
    centre, width = (lo_in + hi_in) / dt(2.0), hi_in - lo_in
    half = (dt(0.5) * width) * dt(1.2)
    lo, hi = centre - half, centre + half
    return lo, hi - lo


def _hand(proj, valid, cam, idx, dt):
    s, z, count = dt(0.0), dt(0.0), 0
    lo, hi = [dt(0.0), dt(0.0)], [dt(0.0), dt(0.0)]
    for k in idx:
        s = s + valid[k]
        z = z + cam[k, 2]
        if valid[k] > 0:
            for c in range(2):
                lo[c] = proj[k, c] if count == 0 else _nmin(lo[c], proj[k, c])
                hi[c] = proj[k, c] if count == 0 else _nmax(hi[c], proj[k, c])
            count += 1
    x, w = _extend(lo[0], hi[0], dt)
    y, h = _extend(lo[1], hi[1], dt)
    return s, z / dt(len(idx)), count, (x, y, w, h)


def coord_rule(proj, valid, cam, lhand, rhand, dtype=F32):
    """Per item: (lose: 0 none / 1 left / 2 right, iou or nan when skipped, the two depths)."""
    dt = np.dtype(dtype).type
    proj, valid, cam = (np.asarray(a, dtype=dt) for a in (proj, valid, cam))
    B = proj.shape[0]
    valid = valid.reshape(B, -1)
    lose, ious, depths = np.zeros(B, np.int32), np.full(B, np.nan), np.zeros((B, 2))
    with np.errstate(all='ignore'):
        for b in range(B):
            sl, dl, nl, L = _hand(proj[b], valid[b], cam[b], lhand, dt)
            sr, dr, nr, R = _hand(proj[b], valid[b], cam[b], rhand, dt)
            depths[b] = dl, dr
            if sl == 0 or sr == 0 or nl == 0 or nr == 0:
                continue
            lx2, ly2, rx2, ry2 = L[2] + L[0], L[3] + L[1], R[2] + R[0], R[3] + R[1]
            xmin, ymin = _nmax(L[0], R[0]), _nmax(L[1], R[1])
            xmax, ymax = _nmin(lx2, rx2), _nmin(ly2, ry2)
            inter = _nmax(dt(0.0), xmax - xmin) * _nmax(dt(0.0), ymax - ymin)
            area_l, area_r = (lx2 - L[0]) * (ly2 - L[1]), (rx2 - R[0]) * (ry2 - R[1])
            iou = inter / (((area_l + area_r) - inter) + dt(1e-5))
            ious[b] = iou
            if iou > dt(0.5):
                lose[b] = 1 if dl > dr else 2
    return lose, ious, depths


def hand_weights(lose, K, lhand, rhand, lwrist, rwrist, dtype=F32):
    hw = np.ones((lose.shape[0], K), dtype)
    for b, n in enumerate(lose):
        if n == 1:
            hw[b, list(lhand) + [lwrist]] = 0
        elif n == 2:
            hw[b, list(rhand) + [rwrist]] = 0
    return hw


def coord_forward(proj, gt, valid, cam, lhand, rhand, lwrist, rwrist, weight=None, dtype=F32):
    """(loss [B, K, 2], hand_w [B, K])."""
    dt = np.dtype(dtype).type
    proj, gt, valid = (np.asarray(a, dtype=dt) for a in (proj, gt, valid))
    B, K = proj.shape[:2]
    lose, _, _ = coord_rule(proj, valid, cam, lhand, rhand, dtype)
    hw = hand_weights(lose, K, lhand, rhand, lwrist, rwrist, dt)
    loss = (np.abs(proj - gt) * valid.reshape(B, K, 1)) * hw[:, :, None]
    if weight is not None:
        loss = loss * np.asarray(weight, dtype=dt)
    return loss, hw


def coord_backward(proj, gt, valid, hand_w, g, weight=None, dtype=F32):
    dt = np.dtype(dtype).type
    proj, gt, valid, hand_w, g = (np.asarray(a, dtype=dt) for a in (proj, gt, valid, hand_w, g))
    B, K = proj.shape[:2]
    if weight is not None:
        g = g * np.asarray(weight, dtype=dt)
    return ((g * hand_w[:, :, None]) * valid.reshape(B, K, 1)) * sign(proj - gt)


# ---- cases --------------------------------------------------------------------------------------------------------------
def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def rot_y(theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def small_rotation(rs, scale=0.05):
    a = rs.randn(3) * scale
    angle = np.linalg.norm(a) + 1e-12
    k = a / angle
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def deg_margin(deg):
    """Distance of every deg to the nearest rounding tie (a half-integer) and to the clamp at 39."""
    return np.minimum(np.abs(deg - np.floor(deg) - 0.5), np.abs(deg - 39.0))


def rotations(rs, B, J, chain, degs=None):
    """rot [B, J, 3, 3] float32 whose chain gives a yaw ``deg`` near ``degs`` (drawn when None) with the 1e-2 margin in both
    float32 and float64; every matrix is a rotation."""
    for _ in range(1000):
        want = rs.uniform(-60, 60, B) if degs is None else np.asarray(degs, float)
        rot = np.stack([np.stack([small_rotation(rs) for _ in range(J)]) for _ in range(B)])
        if len(chain):
            for b in range(B):
                rot[b, chain[0]] = rot_y(-np.deg2rad(want[b]))
                for j in chain[1:]:
                    rot[b, j] = small_rotation(rs, 0.001)
        rot = f32(rot)
        if not len(chain):
            return rot
        if min(deg_margin(yaw_deg(rot, chain, np.float64)).min(), deg_margin(yaw_deg(rot, chain, F32).astype(np.float64)).min()) > 1e-2:
            return rot
    raise RuntimeError('no rotations with the margin')


def faces_of(rs, V, F):
    faces = np.stack([rs.choice(V, 3, replace=False) for _ in range(F)]).astype(np.int64)
    return faces


def kpt_case(seed, B, V, J, K, Ld=17, root='joint', duplicates=False, shared=False, degs=None, proj=True, n_trans=True):
    """A synthetic layer and its inputs.  The full list: J joints, E = min(4, V) extra vertices, Ls = 6 static landmarks, Ld
    dynamic ones, A = 2 appended vertices; ``kpt_idx`` draws K rows so that every kind occurs when K allows."""
    rs = np.random.RandomState(seed)
    F = max(2, min(3 * V, 600))
    faces = faces_of(rs, V, F)
    E, Ls, A = min(4, V), 6, 2
    chain = [J - 2, 1, 0] if Ld else []
    spec = {'V': V, 'J': J, 'faces': faces, 'extra': rs.randint(0, V, E), 'lmk_f': rs.randint(0, F, Ls),
            'lmk_w': f32(rs.dirichlet(np.ones(3), Ls)), 'dyn_f': rs.randint(0, F, (BINS, Ld)),
            'dyn_w': f32(rs.dirichlet(np.ones(3), (BINS, Ld))), 'chain': chain, 'append': rs.randint(0, V, A)}
    R = J + E + Ls + Ld + A
    rot = rotations(rs, B, J, chain, degs)
    if shared and Ld:      # one vertex under three dynamic keypoints in different bins, a static one and a vertex row
        bins = bin_of(yaw_deg(rot, chain))
        for i, b in enumerate(list(bins) + [5, 40, 78]):
            spec['dyn_f'][b, i % Ld] = 0
        spec['lmk_f'][0] = 0
        spec['extra'][0] = faces[0, 1]
    idx = rs.randint(0, R, K) if K > R or duplicates else rs.permutation(R)[:K]
    if duplicates and K > 2:
        idx[K // 2] = idx[0]
        idx[-1] = idx[0]
    if shared and Ld and K >= 6:
        idx[:5] = [J + E + Ls, J + E + Ls + 1, J + E + Ls + 2, J + E, J]
    spec['kpt_idx'] = idx.astype(np.int64)
    spec['root_idx'] = {'joint': min(1, J - 1), 'vertex': J, 'landmark': J + E + 1, 'dynamic': J + E + Ls}[root]
    c = {'spec': spec, 'vertices': f32(rs.randn(B, V, 3) * 0.3), 'joints': f32(rs.randn(B, J, 3) * 0.3), 'rot': rot,
         'trans': f32(rs.randn(B, 3) * 0.1 + [0, 0, 3.0]) if n_trans else None,
         'focal': f32(rs.uniform(900, 1100, (B, 2))) if proj else None, 'princpt': f32(rs.uniform(200, 300, (B, 2))) if proj else None,
         'g_cam': f32(rs.randn(B, K, 3)), 'g_proj': f32(rs.randn(B, K, 2)), 'g_root': f32(rs.randn(B, 3)),
         'g_mesh': f32(rs.randn(B, V, 3))}
    return c


def module_args(spec):
    """The constructor arguments of ``BodyKeypoints`` for a spec."""
    Ld = spec['dyn_f'].shape[1]
    return dict(num_vertices=spec['V'], num_joints=spec['J'], faces=spec['faces'], extra_vertices=spec['extra'],
                lmk_faces_idx=spec['lmk_f'], lmk_bary_coords=spec['lmk_w'], dynamic_lmk_faces_idx=spec['dyn_f'] if Ld else None,
                dynamic_lmk_bary_coords=spec['dyn_w'] if Ld else None, neck_kin_chain=spec['chain'], kpt_idx=spec['kpt_idx'],
                root_idx=spec['root_idx'], append_vertices=spec['append'])


HANDS = (list(range(3, 23)), list(range(25, 45)), 1, 2)      # lhand, rhand, lwrist, rwrist of the coord cases (K >= 45)


def coord_case(seed, B, K=50, hands=HANDS):
    """Items cycle through: boxes overlapping with the left hand deeper, with the right deeper, far apart, a hand without a
    valid entry, a hand with a single valid entry (zero-area box), plain random."""
    rs = np.random.RandomState(seed)
    lhand, rhand = hands[0], hands[1]
    proj = rs.uniform(0, 500, (B, K, 2))
    cam = rs.randn(B, K, 3) * 0.1 + [0, 0, 3.0]
    valid = (rs.rand(B, K) > 0.2).astype(np.float64)
    for b in range(B):
        kind = b % 6
        valid[b, lhand[0]] = valid[b, rhand[0]] = valid[b, lhand[1]] = valid[b, rhand[1]] = 1
        if kind in (0, 1, 3, 4):       # overlapping boxes
            proj[b, lhand] = rs.uniform(100, 200, (len(lhand), 2))
            proj[b, rhand] = proj[b, lhand][:len(rhand)] + rs.uniform(-3, 3, (len(rhand), 2))
            cam[b, lhand, 2] += 0.5 if kind != 1 else -0.5
        elif kind == 2:                # far apart
            proj[b, lhand] = rs.uniform(0, 100, (len(lhand), 2))
            proj[b, rhand] = rs.uniform(300, 400, (len(rhand), 2))
        if kind == 3:
            valid[b, rhand] = 0
        if kind == 4:
            valid[b, lhand] = 0
            valid[b, lhand[3]] = 1
    gt = proj + rs.randn(B, K, 2) * 5
    return {'proj': f32(proj), 'gt': f32(gt), 'valid': f32(valid).reshape(B, K, 1), 'cam': f32(cam),
            'weight': f32(rs.uniform(0, 2, (B, K, 2))), 'g': f32(rs.randn(B, K, 2))}
