"""One deterministic small case for the composed training loss block (``Model.forward``, reference
``avatar/main/model.py:195-258``), and that block written with the HIP modules.

* ``build_case()`` -- every input of the block as numpy arrays, drawn with ``numpy.random.RandomState`` only and rounded
  to float32, so that the float64 run of the reference (``tests/golden/make_golden_lossblock.py``) and the HIP run read
  the same numbers.  Nothing is stored: the fixture keeps a SHA-256 of every array.  The arrays are read-only.
* ``margins(case)`` -- the float64 distances of the case from every decision two float32 evaluations need not share.
* ``HipLoss(case, device)`` -- what ``Model.__init__`` holds: the loss modules, the buffers,
  the constant weights of the fused form, and ``leaves`` (name -> the tensor that requires grad).
* ``wire_losses(m, variant, is_warmup)`` -- the block, twice: ``'dropin'`` as INTEGRATION.md's drop-in lines give it,
  ``'fused'`` with everything INTEGRATION.md offers.  Returns name -> scalar: every term's ``.mean()`` (reference
  ``train.py:43``) and ``'total'``, their sum.

The five Gaussian renders and the two face renders enter as leaves: upstream's rasterizer is not in the reference tree,
and that is the cut at which the block can be run by the reference's own code.  The LPIPS terms are left out on both
sides (no weights at hand).

Mesh: a closed surface of revolution about x, 160 rings of 20 vertices (ring spacing 0.004, radius
``0.04 + 0.008 cos(25 x)``), one pole vertex 0.02 beyond either end, every coordinate jittered by +-5e-4; two triangles
per quad and the two pole fans: V = 3202, F = 6400.  The poles have 20 neighbours, so ``LaplacianReg``'s
``neighbor_max_num = 10`` truncation is on the path; each hand (15 rings and a pole: 301 vertices) exceeds one 256-row
chunk; the arm bands (rings 25..54 and 105..134) give U = 420 upper-arm and L = 780 lower-arm vertices with 21..35
partners within 0.01 along x, so k = 21.
"""
import functools
import hashlib

import numpy as np
import torch

from exavatar_release_amd import p3d_standins as p3d

RINGS, PER_RING = 160, 20
V, N_FACES = RINGS * PER_RING + 2, (RINGS - 1) * PER_RING * 2 + 2 * PER_RING
POLE_R, POLE_L = RINGS * PER_RING, RINGS * PER_RING + 1
RING_DX, POLE_DX, JITTER = 0.004, 0.02, 5e-4
JITTER_SEED, LEAF_SEED = 4269, 606                             # the first seeds from 4242 / 606 that meet check_margins
B, H, W = 2, 48, 72
BBOX = (-5, 7, 60, 50)                                         # clamped by the reference to x 0..60, y 7..48
CROP = (0, 7, 60, 41)                                          # (x0, y0, w, h) of that clamp
BAND = 6                                                       # pixels kept either side of a crop edge inside the image
SAMPLE = 2048                                                  # entries the fixture keeps of a large gradient elsewhere
J = 55
JOINTS_NAME = ('Pelvis', 'L_Hip', 'R_Hip', 'Spine_1', 'L_Knee', 'R_Knee', 'Spine_2', 'L_Ankle', 'R_Ankle', 'Spine_3',
               'L_Foot', 'R_Foot', 'Neck', 'L_Collar', 'R_Collar', 'Head', 'L_Shoulder', 'R_Shoulder', 'L_Elbow',
               'R_Elbow', 'L_Wrist', 'R_Wrist', 'Jaw', 'L_Eye', 'R_Eye') + \
    tuple('%s_%s_%d' % (s, f, i) for s in 'LR' for f in ('Index', 'Middle', 'Pinky', 'Ring', 'Thumb') for i in (1, 2, 3))
JOINT_PART = {'body': range(0, 22), 'face': range(22, 25), 'lhand': range(25, 40), 'rhand': range(40, 55)}
ARM_JOINTS = ('R_Shoulder', 'R_Elbow', 'L_Shoulder', 'L_Elbow')
ARM_RINGS = {'R_Elbow': (25, 40), 'R_Shoulder': (40, 55), 'L_Shoulder': (105, 120), 'L_Elbow': (120, 135)}
W_RGB, W_SSIM, W_LPIPS = 0.8, 0.2, 0.2                         # config.py:35-37
SCALE_MAX = 0.001                                              # model.py:94
# the conditions the generator asserts (float64)
ARM_NORMAL_MARGIN, ARM_DX_MARGIN, ARM_KTH_GAP = 1e-3, 1e-4, 1e-5
L1_KINK, HAND_DOT, SCALE_CLAMP = 1e-6, 1e-4, 1e-6
U_ARM, L_ARM, K_ARM, N_VALID = 420, 780, 21, (21, 35)

RENDERS = ('scene', 'human', 'scene_human', 'human_refined', 'scene_human_refined')
IMAGE_LEAVES = RENDERS + ('face', 'face_refined')
VERTEX_LEAVES = {'rgb': 3, 'rgb_refined': 3, 'scale_raw': 1, 'scale_refined_raw': 1, 'mean_offset': 3,
                 'mean_offset_offset': 3, 'scale_offset': 1, 'rgb_offset': 3}
LEAVES = IMAGE_LEAVES + tuple(VERTEX_LEAVES) + ('joint_offset',)
MASKS = ('is_rhand', 'is_lhand', 'is_face', 'is_face_expr', 'is_cavity')
# name -> the terms of the drop-in block it stands for
FUSED_PAIRS = {'rgb+ssim_human': ('rgb_human', 'ssim_human'),
               'rgb+ssim_human_refined': ('rgb_human_refined', 'ssim_human_refined'),
               'rgb+ssim_scene': ('rgb_scene', 'ssim_scene')}
DROPIN_TERMS = ('rgb_human', 'ssim_human', 'rgb_face', 'rgb_human_rand_bg', 'rgb_human_refined', 'ssim_human_refined',
                'rgb_face_refined', 'rgb_human_refined_rand_bg', 'rgb_scene', 'ssim_scene', 'gaussian_mean_reg',
                'gaussian_mean_hand_reg', 'gaussian_scale_reg', 'lap_mean', 'lap_scale', 'lap_rgb', 'hand_rgb_reg',
                'arm_rgb_reg', 'joint_offset_reg', 'joint_offset_sym_reg')
FUSED_TERMS = ('rgb+ssim_human', 'rgb_face', 'rgb_human_rand_bg', 'rgb+ssim_human_refined', 'rgb_face_refined',
               'rgb_human_refined_rand_bg', 'rgb+ssim_scene') + DROPIN_TERMS[10:]


def _f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32))


def ring_of():
    """[V] the ring index of every vertex, -1 for the two poles."""
    r = np.repeat(np.arange(RINGS), PER_RING)
    return np.concatenate([r, [-1, -1]])


def _mesh():
    x = np.arange(RINGS) * RING_DX
    rad = 0.04 + 0.008 * np.cos(25 * x)
    th = 2 * np.pi * np.arange(PER_RING) / PER_RING
    body = np.stack([np.repeat(x, PER_RING), (rad[:, None] * np.cos(th)[None]).reshape(-1),
                     (rad[:, None] * np.sin(th)[None]).reshape(-1)], 1)
    verts = np.concatenate([body, [[-POLE_DX, 0, 0], [x[-1] + POLE_DX, 0, 0]]])
    r, j = np.meshgrid(np.arange(RINGS - 1), np.arange(PER_RING), indexing='ij')
    a, b = r * PER_RING + j, r * PER_RING + (j + 1) % PER_RING
    c, d = a + PER_RING, b + PER_RING
    quads = np.stack([np.stack([a, b, c], -1), np.stack([b, d, c], -1)], 2).reshape(-1, 3)      # outward
    j = np.arange(PER_RING)
    last = (RINGS - 1) * PER_RING
    fan_r = np.stack([np.full(PER_RING, POLE_R), (j + 1) % PER_RING, j], 1)
    fan_l = np.stack([np.full(PER_RING, POLE_L), last + j, last + (j + 1) % PER_RING], 1)
    return verts, np.concatenate([quads, fan_r, fan_l]).astype(np.int64)


def _blob(cx, cy, rx, ry):
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    return np.sqrt(((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2)


@functools.lru_cache(maxsize=None)
def build_case():
    """dict name -> numpy array: every input of the block (float32 unless a mask or an index), read-only."""
    c = {}
    verts, face = _mesh()
    assert verts.shape == (V, 3) and face.shape == (N_FACES, 3)
    c['mesh_neutral_pose'] = _f32(verts + np.random.RandomState(JITTER_SEED).uniform(-JITTER, JITTER, (V, 3)))
    c['face_upsampled'] = np.ascontiguousarray(face)
    # ---- masks, by ring index (the z > 0 half is decided on the unjittered surface) ------------------------------------
    ring = ring_of()
    slot = np.concatenate([np.tile(np.arange(PER_RING), RINGS), [-1, -1]])
    c['is_rhand'] = ((ring >= 0) & (ring < 15)) | (np.arange(V) == POLE_R)
    c['is_lhand'] = (ring >= 145) | (np.arange(V) == POLE_L)
    c['is_face'] = (ring >= 70) & (ring < 90)
    c['is_face_expr'] = c['is_face'] & (slot >= 1) & (slot <= 9)
    c['is_cavity'] = c['is_face_expr'] & (((ring >= 77) & (ring < 80)) | ((ring == 80) & (slot <= 3)))
    rs = np.random.RandomState(LEAF_SEED)
    # ---- skinning: <= 4 non-zeros per row, the argmax of the arm bands on the four arm joints and of no other row --------
    arm_idx = [JOINTS_NAME.index(n) for n in ARM_JOINTS]
    other = np.array([j for j in range(J) if j not in arm_idx])
    main = other[rs.randint(0, len(other), V)]
    for name, (r0, r1) in ARM_RINGS.items():
        main[(ring >= r0) & (ring < r1)] = JOINTS_NAME.index(name)
    Wt = np.zeros((V, J))
    for v in range(V):
        k = rs.randint(1, 5)
        rest = rs.permutation(np.array([j for j in range(J) if j != main[v]]))[:k - 1]
        w = np.sort(rs.uniform(0.05, 1.05, k))[::-1]
        w[0] += 0.05                                                              # a strict argmax after rounding
        Wt[v, np.concatenate([[main[v]], rest]).astype(np.int64)] = w / w.sum()
    c['skinning_weight'] = _f32(Wt)
    # ---- data ----------------------------------------------------------------------------------------------------------
    c['img'] = _f32(rs.uniform(0.02, 0.98, (B, 3, H, W)))
    mask = np.stack([np.clip(1.6 - _blob(30 + 6 * b, 26 - 3 * b, 16, 13), 0, 1) for b in range(B)])[:, None]
    c['mask'] = _f32(mask)                                                       # exact 0 / 1 regions and a soft rim
    c['bbox'] = _f32([BBOX] * B)
    c['bg'] = _f32(rs.uniform(0.05, 0.95, 3))
    c['joint_offset_ref'] = _f32(0.01 * rs.randn(J, 3))                          # smpl_x.joint_offset, model.py:256
    # ---- leaves --------------------------------------------------------------------------------------------------------
    for k in RENDERS:
        c[k] = _f32(rs.uniform(0.02, 0.98, (B, 3, H, W)))
    for n, k in enumerate(('face', 'face_refined')):
        d = np.stack([_blob(50 - 2 * b - n, 20 + 3 * b + n, 14, 10) for b in range(B)])[:, None]
        rgb = rs.uniform(0.02, 0.98, (B, 3, H, W))
        rgb = np.where(d < 1, rgb, -1.0)
        for b in range(B):                       # a few pixels of the core with one channel at exactly -1 (per-channel test)
            rgb[b, 1, 20 + 3 * b, 44:48] = -1.0
        c[k] = _f32(rgb)
        c[k + '_alpha'] = _f32(np.where(d < 0.8, 1.0, np.where(d < 1, 0.5, 0.0)))
    for k, ch in VERTEX_LEAVES.items():
        if k.startswith('rgb') and k != 'rgb_offset':
            a = rs.uniform(0.02, 0.98, (B, V, ch))
        elif k.startswith('scale') and k != 'scale_offset':
            a = rs.uniform(0.0005, 0.0015, (B, V, ch))
            a = np.where(np.abs(a - SCALE_MAX) < 4e-6, a + 1e-5, a)
        elif k == 'scale_offset':
            a = 0.1 * rs.randn(B, V, ch)
        else:
            a = 0.01 * rs.randn(B, V, ch)
        c[k] = _f32(a)
    c['joint_offset'] = _f32(c['joint_offset_ref'] + 0.005 * rs.randn(J, 3))
    for a in c.values():
        a.setflags(write=False)
    return c


def digests(case):
    """name -> SHA-256 of the array's bytes (dtype and shape included)."""
    return {k: hashlib.sha256(('%s%s' % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()
            for k, a in case.items()}


# ---- what the fixture keeps of a gradient -------------------------------------------------------------------------------
def sample_index(name, shape):
    """The sorted flat entries of a gradient the fixture keeps, or None (all of it): a function of the leaf's name and
    shape alone.  Of a [B, C, H, W] gradient of a cropped render: every pixel within ``BAND`` of a crop edge that lies
    inside the image (where a bbox error shows), and ``SAMPLE`` fixed entries; of another large tensor ``SAMPLE`` fixed
    entries."""
    n = int(np.prod(shape))
    if n <= 4096:
        return None
    rs = np.random.RandomState(int(hashlib.sha256(name.encode()).hexdigest()[:8], 16))
    keep = np.zeros(n, dtype=bool)
    keep[rs.permutation(n)[:SAMPLE]] = True
    if len(shape) == 4 and name != 'scene':
        x1, y0 = CROP[0] + CROP[2], CROP[1]
        band = np.zeros(shape, dtype=bool)
        band[:, :, max(y0 - BAND, 0):y0 + BAND, :] = True
        band[:, :, :, x1 - BAND:min(x1 + BAND, shape[3])] = True
        keep |= band.reshape(-1)
    return np.nonzero(keep)[0]


def take_sample(name, a):
    idx = sample_index(name, a.shape)
    return a if idx is None else a.reshape(-1)[idx]


# ---- the case's distances from every decision ---------------------------------------------------------------------------
def normals64(case):
    """Float64 vertex normals of the ``Meshes`` stand-in, [V, 3]."""
    m = p3d.Meshes(verts=torch.from_numpy(np.array(case['mesh_neutral_pose'])).double()[None],
                   faces=torch.from_numpy(np.array(case['face_upsampled']))[None])
    return m.verts_normals_packed().numpy()


def arm_masks(case, normal):
    """``smpl_x.get_arm`` (smpl_x.py:139-148) on numpy arrays: (is_upper_arm, is_lower_arm)."""
    label = case['skinning_weight'].argmax(1)
    is_arm = np.isin(label, [JOINTS_NAME.index(n) for n in ARM_JOINTS])
    return is_arm & (normal[:, 1] > 0.5), is_arm & (normal[:, 1] <= 0.5)


def l1_maps(case):
    """name -> float64 ``x - target`` of the seven L1 maps of the block (model.py:197-214), uncropped."""
    c = {k: case[k].astype(np.float64) for k in IMAGE_LEAVES + ('img', 'mask', 'bg', 'face_alpha', 'face_refined_alpha')}
    target = c['img'] * c['mask'] + (1 - c['mask']) * c['bg'][None, :, None, None]
    out = {'rgb_scene': c['scene'] - c['img']}
    for tag in ('', '_refined'):
        f = ((c['face' + tag] != -1) & (c['face%s_alpha' % tag] == 1)).astype(np.float64)
        sh = c['scene_human' + tag]
        out['rgb_human' + tag] = sh - c['img']
        out['rgb_face' + tag] = sh * (1 - f) + c['face' + tag] * f - c['img']
        out['rgb_human%s_rand_bg' % tag] = c['human' + tag] - target
    return out


def margins(case):
    """name -> float64 figure; the generator asserts every one against its constant above."""
    mesh = case['mesh_neutral_pose'].astype(np.float64)
    normal = normals64(case)
    n32 = normal.astype(np.float32)
    up, lo = arm_masks(case, normal)
    up32, lo32 = arm_masks(case, n32)
    out = {'arm/float32_masks_equal': float(np.array_equal(up, up32) and np.array_equal(lo, lo32)),
           'arm/U': float(up.sum()), 'arm/L': float(lo.sum()),
           'arm/normal_margin': float(np.abs(normal[up | lo, 1] - 0.5).min())}
    dx = np.abs(mesh[lo][:, None, 0] - mesh[up][None, :, 0])
    dx32 = np.abs(case['mesh_neutral_pose'][lo][:, None, 0] - case['mesh_neutral_pose'][up][None, :, 0])
    valid = dx32 < np.float32(0.01)
    assert np.array_equal(valid, dx < 0.01)
    n_valid = valid.sum(1)
    k = min(50, int(n_valid.min()))
    d = np.sqrt(((mesh[lo][:, None] - mesh[up][None]) ** 2).sum(2))
    d = np.sort(np.where(valid, d, np.inf), 1)
    gap = np.where(np.isfinite(d[:, k]), (d[:, k] - d[:, k - 1]) / d[:, k - 1], np.inf)
    out.update({'arm/dx_margin': float(np.abs(dx - 0.01).min()), 'arm/k': float(k), 'arm/n_valid_min': float(n_valid.min()),
                'arm/n_valid_max': float(n_valid.max()), 'arm/kth_gap': float(gap.min())})
    x0, y0, w, h = CROP
    for name, m in l1_maps(case).items():
        if name != 'rgb_scene':
            m = m[:, :, y0:y0 + h, x0:x0 + w]
        out['l1_kink/' + name] = float(np.abs(m).min())
    hand = case['is_rhand'] | case['is_lhand']
    for k_ in ('mean_offset', 'mean_offset_offset'):
        o = case[k_].astype(np.float64)
        norm = np.linalg.norm(o, axis=2)
        dot = (normal[None] * o / norm[:, :, None]).sum(2)[:, hand]
        out['hand_dot/' + k_] = float(np.abs(dot).min())
        out['offset_norm/' + k_] = float(norm.min())
    for k_ in ('scale_raw', 'scale_refined_raw'):
        out['scale_clamp/' + k_] = float(np.abs(case[k_].astype(np.float64) - SCALE_MAX).min())
    return out


def check_margins(mg):
    """Raises AssertionError where the case is too near a decision (choose another seed)."""
    assert mg['arm/float32_masks_equal'] == 1.0
    assert (mg['arm/U'], mg['arm/L'], mg['arm/k']) == (U_ARM, L_ARM, K_ARM), mg
    assert (mg['arm/n_valid_min'], mg['arm/n_valid_max']) == N_VALID, mg
    assert mg['arm/normal_margin'] > ARM_NORMAL_MARGIN and mg['arm/dx_margin'] > ARM_DX_MARGIN, mg
    assert mg['arm/kth_gap'] > ARM_KTH_GAP, mg['arm/kth_gap']
    for k, v in mg.items():
        if k.startswith('l1_kink/'):
            assert v > L1_KINK, (k, v)
        if k.startswith('hand_dot/'):
            assert v >= HAND_DOT, (k, v)
        if k.startswith('offset_norm/'):
            assert v > 0, (k, v)
        if k.startswith('scale_clamp/'):
            assert v > SCALE_CLAMP, (k, v)


# ---- the scale of a scalar term -----------------------------------------------------------------------------------------
FACTOR = 4.0
U24 = 2.0 ** -24


def term_value(g, name):
    """The float64 value of a term of either variant from the fixture ``g``: a fused pair is the sum of its two terms."""
    if name == 'total':
        return float(g['total'])
    return sum(float(g['term/' + p]) for p in FUSED_PAIRS.get(name, (name,)))


def term_scale(g, variant, name):
    """The rounding scale of one scalar term.  A term's own float32 error is one draw and no
    scale, so it is derived: ``elem`` is the root sum square over the elements of the first-order error one float32
    evaluation commits on each (``make_golden_lossblock.element_errors``, stored as ``#elem`` = sqrt(sum e_i^2) / N);
    to it come the roundings made at the magnitude of the reduced scalar m, ``r 2^-24 |m|``: the reduction tree
    (partial sums s with sum s^2 <= 2 m^2 N^2 for terms of one sign) and the division by N give sqrt(3) < r = 2 for a
    ``.mean()``; ``PhotometricLoss`` reduces two sums and forms ``w1 l1 + w2 (1 - ssim)`` from them, nine roundings in
    all, r = 4 > 3; the arm term of the ``plan.count`` formula has one more product than a mean, r = 3.  The total adds n
    terms of one sign in order: ``sqrt(n) 2^-24 |total|`` on top of the root sum square of its terms' scales."""
    if name == 'total':
        names = FUSED_TERMS if variant == 'fused' else DROPIN_TERMS
        return float(np.sqrt(sum(term_scale(g, variant, k) ** 2 for k in names))
                     + U24 * np.sqrt(len(names)) * abs(float(g['total'])))
    parts = FUSED_PAIRS.get(name, (name,))
    elem = float(np.sqrt(sum(float(g['term/%s#elem' % p]) ** 2 for p in parts)))
    r = 4 if len(parts) == 2 else (3 if (variant == 'fused' and name == 'arm_rgb_reg') else 2)
    return elem + r * U24 * abs(term_value(g, name))


# ---- the constants of the block -----------------------------------------------------------------------------------------
def vertex_weights(masks, ones):
    """The six per-vertex weights of model.py:217-247, ``[1, V, 1]`` each: ``ones`` is a ``[1, V, 1]`` tensor of ones on
    the masks' device; name -> weight.  (Boolean-mask assignment reads the mask back on the host: the fused form builds them once.)"""
    r, l, f, fe, cav = (masks[k] for k in MASKS)

    def make(base, *rules):
        w = ones * base
        for m, value in rules:
            w[:, m, :] = value
        return w
    return {'gaussian_mean_reg': make(10, (r, 1000), (l, 1000), (f, 1), (fe, 10)),
            'gaussian_scale_reg': make(1, (r, 1000), (l, 1000), (fe, 10), (cav, 0)),
            'lap_mean': make(1, (fe, 50), (cav, 0.1)),
            'lap_scale': make(10, (r, 10), (l, 10), (fe, 0)),
            'lap_rgb': make(0.1, (r, 100), (l, 100))}


def joint_weight(ones):
    """model.py:253-255: ``ones`` [J, 3] -> the weight of ``joint_offset_reg``."""
    w = ones.clone()
    w[list(JOINT_PART['lhand']), :] = 10
    w[list(JOINT_PART['rhand']), :] = 10
    return w


def gather_assets(leaves, is_warmup):
    """``human_assets`` / ``human_assets_refined`` as model.py:91-106 gathers them from the leaves, in plain torch on both
    sides: ``scale`` is the raw [B, V, 1] scale repeated to three columns (module.py:531-534) and, in the warm-up, clamped
    at 0.001 with ``scale_wo_clamp`` its clone."""
    out = []
    for tag in ('', '_refined'):
        a = {'rgb': leaves['rgb' + tag], 'scale': leaves['scale%s_raw' % tag].repeat(1, 1, 3)}
        if is_warmup:
            a['scale_wo_clamp'] = a['scale'].clone()
            a['scale'] = torch.clamp(a['scale'], max=SCALE_MAX)
        out.append(a)
    return out


def face_render(leaves, consts, tag):
    """The [B, 4, H, W] face render: the differentiable colour channels and the constant coverage channel."""
    return torch.cat((leaves['face' + tag], consts['face%s_alpha' % tag]), 1)


# ---- the block with the HIP modules ------------------------------------------------------------------------------------
class HipLoss:
    """What ``Model.__init__`` holds of the loss block, built from the case on ``device``."""

    def __init__(self, case, device):
        import exavatar_release_amd as exa
        c, dev = case, torch.device(device)
        t = lambda k: torch.from_numpy(np.array(c[k])).to(dev)      # noqa: E731
        self.device = dev
        self.leaves = {k: t(k).requires_grad_(True) for k in LEAVES}
        self.consts = {k: t(k) for k in ('face_alpha', 'face_refined_alpha')}
        self.data = {'img': t('img'), 'mask': t('mask'), 'bbox': torch.from_numpy(np.array(c['bbox']))}    # bbox: on the host
        self.bg = t('bg')
        self.mesh_neutral_pose = t('mesh_neutral_pose')
        self.masks = {k: t(k) for k in MASKS}
        self.skinning_weight = t('skinning_weight')
        self.joint_offset_ref = t('joint_offset_ref')
        self.face_upsampled = np.array(c['face_upsampled'])          # smpl_x.face_upsampled: a host array, one object
        # Model.__init__ (model.py:27-35)
        self.rgb_loss, self.ssim = exa.RGBLoss(), exa.SSIM()
        self.crit = exa.PhotometricLoss(W_RGB, W_SSIM)
        self.lap_reg = exa.LaplacianReg(V, self.face_upsampled)
        self.hand_mean_reg = exa.HandMeanReg(self.face_upsampled)
        self.hand_rgb_reg, self.arm_rgb_reg = exa.HandRGBReg(), exa.ArmRGBReg()
        self.arm_joint_idx = [JOINTS_NAME.index(n) for n in ARM_JOINTS]
        self.sym_right = [j for j in range(J) if JOINTS_NAME[j][:2] == 'R_']
        self.sym_left = [JOINTS_NAME.index('L_' + JOINTS_NAME[j][2:]) for j in self.sym_right]
        # the constants of the fused form, built once
        self.weights = vertex_weights(self.masks, torch.ones((1, V, 1), device=dev))
        self.joint_weight = joint_weight(torch.ones((J, 3), device=dev))
        self.sym_right_idx, self.sym_left_idx = (torch.tensor(i, dtype=torch.int64, device=dev)
                                                 for i in (self.sym_right, self.sym_left))
        self.plan = None                                             # what arm_neighbors returned last
        self.arm = None                                              # what get_arm returned last


def joint_offset_sym(m, joint_offset, fused):
    """``JointOffsetSymmetricReg`` (loss.py:133-146; no HIP replacement): |x_R + x_L| + |y_R - y_L| + |z_R - z_L| per pair.
    The reference indexes with two Python lists it rebuilds on every call, a host-to-device copy each; the fused form
    selects with the same lists held as device tensors."""
    if fused:
        r, l = joint_offset.index_select(0, m.sym_right_idx), joint_offset.index_select(0, m.sym_left_idx)
    else:
        r, l = joint_offset[m.sym_right], joint_offset[m.sym_left]
    return torch.abs(r[:, 0] + l[:, 0]) + torch.abs(r[:, 1] - l[:, 1]) + torch.abs(r[:, 2] - l[:, 2])


def wire_losses(m, variant, is_warmup):
    """The block of model.py:195-258 with the HIP modules; name -> 0-dim tensor, ``'total'`` last."""
    import exavatar_release_amd as exa
    assert variant in ('dropin', 'fused'), variant
    fused = variant == 'fused'
    L, data, bg, masks = m.leaves, m.data, m.bg, m.masks
    mesh_neutral_pose = m.mesh_neutral_pose
    is_rhand, is_lhand = masks['is_rhand'], masks['is_lhand']
    human_assets, human_assets_refined = gather_assets(L, is_warmup)
    human_offsets = {k: L[k] for k in ('mean_offset', 'mean_offset_offset', 'scale_offset', 'rgb_offset')}
    scene_renders, human_renders, scene_human_renders = {'img': L['scene']}, {'img': L['human']}, {'img': L['scene_human']}
    human_renders_refined, scene_human_renders_refined = {'img': L['human_refined']}, {'img': L['scene_human_refined']}
    face_renders, face_renders_refined = face_render(L, m.consts, ''), face_render(L, m.consts, '_refined')

    loss = {}
    if fused:
        loss['rgb+ssim_human'] = m.crit(scene_human_renders['img'], data['img'], bbox=data['bbox'])
    else:
        loss['rgb_human'] = m.rgb_loss(scene_human_renders['img'], data['img'], bbox=data['bbox']) * W_RGB
        loss['ssim_human'] = (1 - m.ssim(scene_human_renders['img'], data['img'], bbox=data['bbox'])) * W_SSIM
    is_face = ((face_renders[:, :3] != -1) * (face_renders[:, 3:] == 1)).float()
    loss['rgb_face'] = m.rgb_loss(scene_human_renders['img'] * (1 - is_face) + face_renders[:, :3] * is_face, data['img'],
                                  bbox=data['bbox']) * W_RGB
    loss['rgb_human_rand_bg'] = m.rgb_loss(human_renders['img'], data['img'], bbox=data['bbox'], mask=data['mask'],
                                           bg=bg[None])
    if fused:
        loss['rgb+ssim_human_refined'] = m.crit(scene_human_renders_refined['img'], data['img'], bbox=data['bbox'])
    else:
        loss['rgb_human_refined'] = m.rgb_loss(scene_human_renders_refined['img'], data['img'], bbox=data['bbox']) * W_RGB
        loss['ssim_human_refined'] = (1 - m.ssim(scene_human_renders_refined['img'], data['img'],
                                                 bbox=data['bbox'])) * W_SSIM
    is_face = ((face_renders_refined[:, :3] != -1) * (face_renders_refined[:, 3:] == 1)).float()
    loss['rgb_face_refined'] = m.rgb_loss(scene_human_renders_refined['img'] * (1 - is_face)
                                          + face_renders_refined[:, :3] * is_face, data['img'], bbox=data['bbox']) * W_RGB
    loss['rgb_human_refined_rand_bg'] = m.rgb_loss(human_renders_refined['img'], data['img'], bbox=data['bbox'],
                                                   mask=data['mask'], bg=bg[None])
    if fused:
        loss['rgb+ssim_scene'] = m.crit(scene_renders['img'], data['img'], l1_weight=1 - data['mask'],
                                        ssim_mask=1 - data['mask'])
    else:
        loss['rgb_scene'] = m.rgb_loss(scene_renders['img'], data['img']) * (1 - data['mask']) * W_RGB
        loss['ssim_scene'] = (1 - m.ssim(scene_renders['img'], data['img'], mask=1 - data['mask'])) * W_SSIM

    # the per-vertex weights: the fused form holds them as constants, the drop-in builds them as model.py:217-247 does
    wt = m.weights if fused else vertex_weights(masks, torch.ones((1, V, 1), device=m.device))
    normal = exa.vertex_normals(mesh_neutral_pose.detach(), m.face_upsampled)          # once per iteration, [1, V, 3]
    loss['gaussian_mean_reg'] = (human_offsets['mean_offset'] ** 2 + human_offsets['mean_offset_offset'] ** 2) \
        * wt['gaussian_mean_reg']
    loss['gaussian_mean_hand_reg'] = \
        m.hand_mean_reg(mesh_neutral_pose, human_offsets['mean_offset'], is_lhand, is_rhand, normal=normal) \
        + m.hand_mean_reg(mesh_neutral_pose, human_offsets['mean_offset_offset'], is_lhand, is_rhand, normal=normal)
    if is_warmup:
        loss['gaussian_scale_reg'] = (human_assets['scale_wo_clamp'] ** 2 + human_offsets['scale_offset'] ** 2) \
            * wt['gaussian_scale_reg']
    else:
        loss['gaussian_scale_reg'] = (human_assets['scale'] ** 2 + human_offsets['scale_offset'] ** 2) \
            * wt['gaussian_scale_reg']
    neutral = mesh_neutral_pose[None, :, :].detach()
    a = neutral + human_offsets['mean_offset']
    b = neutral + human_offsets['mean_offset'] + human_offsets['mean_offset_offset']
    if fused:
        w = wt['lap_mean']
        loss['lap_mean'] = (m.lap_reg(a, neutral, w) + m.lap_reg(b, neutral, w)) * 100000
        w = wt['lap_scale']
        loss['lap_scale'] = (m.lap_reg(human_assets['scale'], None, w)
                             + m.lap_reg(human_assets_refined['scale'], None, w)) * 100000
        w = wt['lap_rgb']
        loss['lap_rgb'] = m.lap_reg(human_assets['rgb'], None, w) + m.lap_reg(human_assets_refined['rgb'], None, w)
    else:
        loss['lap_mean'] = (m.lap_reg(a, neutral) + m.lap_reg(b, neutral)) * 100000 * wt['lap_mean']
        loss['lap_scale'] = (m.lap_reg(human_assets['scale'], None)
                             + m.lap_reg(human_assets_refined['scale'], None)) * 100000 * wt['lap_scale']
        loss['lap_rgb'] = (m.lap_reg(human_assets['rgb'], None) + m.lap_reg(human_assets_refined['rgb'], None)) \
            * wt['lap_rgb']

    loss['hand_rgb_reg'] = (m.hand_rgb_reg(human_assets['rgb'], is_rhand, is_lhand)
                            + m.hand_rgb_reg(human_assets_refined['rgb'], is_rhand, is_lhand)) * 0.01
    m.arm = exa.get_arm(mesh_neutral_pose, m.skinning_weight, m.face_upsampled, m.arm_joint_idx, normal=normal)
    is_upper_arm, is_lower_arm = m.arm
    if fused:
        plan = m.plan = exa.arm_neighbors(mesh_neutral_pose, is_upper_arm, is_lower_arm)      # once per iteration
        dense = exa.arm_rgb_loss(plan, human_assets['rgb']) + exa.arm_rgb_loss(plan, human_assets_refined['rgb'])
        loss['arm_rgb_reg'] = dense.sum() / (3 * dense.shape[0] * plan.count) * 0.1
    else:
        loss['arm_rgb_reg'] = (m.arm_rgb_reg(mesh_neutral_pose, is_upper_arm, is_lower_arm, human_assets['rgb'])
                               + m.arm_rgb_reg(mesh_neutral_pose, is_upper_arm, is_lower_arm,
                                               human_assets_refined['rgb'])) * 0.1

    jw = m.joint_weight if fused else joint_weight(torch.ones((J, 3), device=m.device))
    loss['joint_offset_reg'] = (L['joint_offset'] - m.joint_offset_ref) ** 2 * jw
    loss['joint_offset_sym_reg'] = joint_offset_sym(m, L['joint_offset'], fused)

    loss = {k: v.mean() for k, v in loss.items()}                                      # train.py:43
    assert tuple(loss) == (FUSED_TERMS if fused else DROPIN_TERMS), tuple(loss)
    loss['total'] = sum(loss[k] for k in loss)                                         # train.py:46
    return loss
