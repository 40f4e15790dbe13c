"""One deterministic small avatar for the composed ``HumanGaussian.forward`` (reference
``avatar/common/nets/module.py:516-586``), and that forward written with the HIP modules.

* ``build_case()`` -- every input of the forward as float32 numpy arrays, drawn with ``numpy.random.RandomState`` only
  (its stream is frozen across NumPy versions) and rounded to float32, so that the float64 run of the reference
  (``tests/golden/make_golden_human.py``) and the HIP run read the same numbers.  Nothing is stored: the fixture keeps a
  SHA-256 of every array.
* ``HipHuman(case, device)`` -- what ``HumanGaussian.init()`` builds once per model: the
  triplane plan, the four ``FusedMLP`` s over the modules' own Parameters, the blend-shape tables, the parents list; and
  the leaves the gradients are taken to.
* ``wire_hip(model, is_world_coord)`` -- the forward exactly as the INTEGRATION.md section 5 snippets wire it; returns
  ``(assets, assets_refined, offsets)`` with the reference's keys.

Sizes (the smallest at which every module leaves its trivial path): a closed mesh of 162 vertices (a stretched level-2
icosphere) subdivided twice with the ``SubdivideMeshes`` stand-in to V = 2562 vertices and 5120 faces, the low-resolution
vertices first -- 2562 = 5 * 512 + 2 (a two-row last MLP chunk) = 10 * 256 + 2 (a two-vertex last skinning chunk), more
than one blend chunk of 1024 compact columns; J = 55 with the SMPL-X tree; triplanes (32, 16, 16); the four nets at
their real widths; Ke = 50, Kp = 486.
"""
import functools
import hashlib

import numpy as np
import torch
import torch.nn as nn

from exavatar_release_amd import lbs, p3d_standins as p3d

V_LR, V, N_FACES = 162, 2562, 5120
J, KE, KP = 55, 50, 486
PARENTS = tuple(lbs.SMPLX_PARENTS)
JOINT_PART = {'body': 22, 'lhand': 15, 'rhand': 15}           # module.py:283 reads len(smpl_x.joint_part['body'])
TRIPLANE_SHAPE = (32, 16, 16)
TRIPLANE_SHAPE_3D = (2.0, 2.0, 2.0)
TRIPLANE_FACE_SHAPE_3D = (0.4, 0.3, 0.3)                       # narrower than the face: rows land in the zero padding
RADII = (0.35, 0.8, 0.25)                                      # the stretch of the icosphere (x: arms, y: up, z: front)
JITTER, JITTER_SEED = 0.006, 5                                 # fixed jitter of the upsampled mesh (the knn condition)
KNN_GAP = 1e-4
RELU_MARGIN, RELU_BAND = 5e-5, 1e-2                            # a pre-ReLU activation nearer to 0 makes its row ambiguous
IMG_SHAPE = (96, 128)                                          # (H, W) of the render test
# module.py:279-287: name -> (widths, relu_final, use_gn)
NETS = {
    'geo_net': ([96, 128, 128, 128], True, True),
    'mean_offset_net': ([128, 3], False, False),
    'scale_net': ([128, 1], False, False),
    'geo_offset_net': ([96 + 126, 128, 128, 128], True, True),
    'mean_offset_offset_net': ([128, 3], False, False),
    'scale_offset_net': ([128, 1], False, False),
    'rgb_net': ([96, 128, 128, 128, 3], False, True),
    'rgb_offset_net': ([96 + 126 + 3, 128, 128, 128, 3], False, True),
}
POSE_LEAVES = ('root_pose', 'body_pose', 'jaw_pose', 'lhand_pose', 'rhand_pose')
DATA_LEAVES = ('triplane', 'triplane_face') + POSE_LEAVES + ('expr', 'trans', 'joint_zero_pose',
                                                             'transform_mat_neutral_pose', 'mesh_neutral_pose')
ASSET_KEYS = ('mean_3d', 'opacity', 'scale', 'rotation', 'rgb')
OFFSET_KEYS = ('mean_offset', 'mean_offset_offset', 'scale_offset', 'rgb_offset')
# the tensors that get a cotangent: the three differentiable assets of both sets and the four offsets
OUTPUTS = tuple('%s/%s' % (s, k) for s in ('assets', 'assets_refined') for k in ('mean_3d', 'scale', 'rgb')) + \
    tuple('offsets/' + k for k in OFFSET_KEYS)
ROW_SAMPLE, ENTRY_SAMPLE = 640, 384                            # what the fixture keeps of a [V, c] tensor / a large gradient


def _icosphere(level):
    """Unit icosphere: (verts [n, 3] float64, faces [f, 3] int64); level 2 has 162 vertices and 320 faces."""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
             (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    verts = [np.asarray(v, dtype=np.float64) / np.linalg.norm(v) for v in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
             (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
             (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, out = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                v = verts[a] + verts[b]
                verts.append(v / np.linalg.norm(v))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in faces:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return np.stack(verts), np.asarray(faces, dtype=np.int64)


def _rotation(aa):
    """Rodrigues' formula in float64: axis-angle [3] -> [3, 3]."""
    th = np.linalg.norm(aa)
    k = aa / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def _f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32))


def net_keys(name):
    """The ``state_dict`` keys of a ``make_linear_layers`` Sequential and their shapes, in order."""
    dims, relu_final, use_gn = NETS[name]
    keys, at = [], 0
    for i in range(len(dims) - 1):
        keys += [('%d.weight' % at, (dims[i + 1], dims[i])), ('%d.bias' % at, (dims[i + 1],))]
        at += 1
        if i < len(dims) - 2 or relu_final:
            if use_gn:
                keys += [('%d.weight' % at, (dims[i + 1],)), ('%d.bias' % at, (dims[i + 1],))]
                at += 1
            at += 1                                              # the ReLU
    return keys


def linear_layers(name):
    """The Sequential ``make_linear_layers`` builds for this net: Linear [-> GroupNorm(4)] -> ReLU per hidden layer."""
    dims, relu_final, use_gn = NETS[name]
    mods = []
    for i in range(len(dims) - 1):
        mods.append(nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2 or relu_final:
            if use_gn:
                mods.append(nn.GroupNorm(4, dims[i + 1]))
            mods.append(nn.ReLU(inplace=True))
    return nn.Sequential(*mods)


@functools.lru_cache(maxsize=None)
def build_case():
    """dict name -> numpy array: every input of the forward (float32 unless a mask or an index)."""
    rs = np.random.RandomState(20240)
    c = {}
    # ---- mesh: 162 -> 642 -> 2562 vertices, the low-resolution ones first --------------------------------------------
    sphere, faces = _icosphere(2)
    lr = _f32(sphere * np.asarray(RADII))
    mesh = p3d.Meshes(torch.from_numpy(lr)[None], torch.from_numpy(faces)[None])
    for _ in range(2):
        mesh = p3d.SubdivideMeshes()(mesh)
    hr = mesh.verts_packed().numpy().astype(np.float64)
    face_hr = mesh.faces_packed().numpy()
    assert lr.shape == (V_LR, 3) and hr.shape == (V, 3) and face_hr.shape == (N_FACES, 3)
    assert np.array_equal(hr[:V_LR].astype(np.float32), lr)
    c['mesh_lr'] = lr                                                             # mesh_neutral_pose_wo_upsample
    c['face_upsampled'] = np.ascontiguousarray(face_hr.astype(np.int64))
    jitter = np.random.RandomState(JITTER_SEED).uniform(-JITTER, JITTER, (V, 3))
    c['mesh_neutral_pose'] = _f32(hr + jitter)
    c['pos_enc_mesh'] = _f32(hr * np.asarray((1.05, 0.95, 1.1)) + rs.uniform(-0.003, 0.003, (V, 3)))
    # ---- masks, carved by coordinate ---------------------------------------------------------------------------------
    x, y, z = hr[:, 0], hr[:, 1], hr[:, 2]
    c['is_rhand'] = x < -0.28
    c['is_lhand'] = x > 0.28
    c['is_face'] = y > 0.6
    c['is_face_expr'] = (y > 0.6) & (z > 0.02)
    c['is_cavity'] = (y > 0.66) & (y < 0.74) & (z > 0.08)
    # ---- skeleton ----------------------------------------------------------------------------------------------------
    c['joint_zero_pose'] = _f32(rs.uniform(-1, 1, (J, 3)) * np.asarray(RADII) * 0.8)
    T = np.zeros((J, 4, 4))
    for j in range(J):
        T[j, :3, :3] = _rotation(0.25 * rs.randn(3))
        T[j, :3, 3] = 0.05 * rs.randn(3)
    T[:, 3, 3] = 1.0
    c['transform_mat_neutral_pose'] = _f32(T)                                     # rigid, not the identity
    W = np.zeros((V, J))
    for v in range(V):                                                            # <= 4 non-zeros per row, summing to 1
        k = rs.randint(1, 5)
        cols = rs.permutation(J)[:k]
        w = rs.uniform(0.05, 1.05, k)
        W[v, cols] = w / w.sum()
    c['skinning_weight'] = _f32(W)
    c['root_pose'] = _f32(0.3 * rs.randn(3))
    c['body_pose'] = _f32(0.3 * rs.randn(JOINT_PART['body'] - 1, 3))
    c['jaw_pose'] = _f32(0.2 * rs.randn(3))
    c['leye_pose'] = np.zeros(3, dtype=np.float32)                                # exactly 0: the finite-gradient path
    c['reye_pose'] = np.zeros(3, dtype=np.float32)
    c['lhand_pose'] = _f32(0.3 * rs.randn(JOINT_PART['lhand'], 3))
    c['rhand_pose'] = _f32(0.3 * rs.randn(JOINT_PART['rhand'], 3))
    c['expr'] = _f32(0.5 * rs.randn(KE))
    c['trans'] = _f32((0.1, -0.15, 3.0))
    # ---- blend shapes ------------------------------------------------------------------------------------------------
    c['pose_dirs'] = _f32(0.004 * rs.randn(KP, 3 * V))
    expr_dirs = 0.004 * rs.randn(V, 3, KE)
    expr_dirs[~c['is_face_expr']] = 0.0
    c['expr_dirs'] = _f32(expr_dirs)
    # ---- triplanes and nets ------------------------------------------------------------------------------------------
    c['triplane'] = _f32(0.5 * rs.randn(3, *TRIPLANE_SHAPE))
    c['triplane_face'] = _f32(0.5 * rs.randn(3, *TRIPLANE_SHAPE))
    for name in NETS:
        dims = NETS[name][0]
        for key, shape in net_keys(name):
            li = int(key.split('.')[0])
            if len(shape) == 2:
                a = rs.uniform(-1, 1, shape) / np.sqrt(shape[1])
            elif key.endswith('bias'):
                a = rs.uniform(-0.2, 0.2, shape)
            else:
                a = rs.uniform(0.5, 1.5, shape)                                   # GroupNorm weights
            last = li == max(int(k.split('.')[0]) for k, _ in net_keys(name))
            if last and name in ('mean_offset_net', 'mean_offset_offset_net'):
                a = a * 0.004                                                      # offsets of a few millimetres
            if last and name in ('scale_net', 'scale_offset_net'):
                a = a * 0.1 - (4.0 if name == 'scale_net' and len(shape) == 1 else 0.0)      # exp(scale) ~ 0.02
            c['%s.%s' % (name, key)] = _f32(a)
        assert dims[0] in (96, 128, 222, 225)
    # ---- camera ------------------------------------------------------------------------------------------------------
    c['cam_R'] = _f32(_rotation(np.asarray((0.12, -0.2, 0.08))))
    c['cam_t'] = _f32((0.05, -0.04, 0.3))
    c['cam_focal'] = _f32((150.0, 150.0))
    c['cam_princpt'] = _f32((IMG_SHAPE[1] / 2.0, IMG_SHAPE[0] / 2.0))
    for a in c.values():
        a.setflags(write=False)
    return c


def digests(case):
    """name -> SHA-256 of the array's bytes (dtype and shape included)."""
    return {k: hashlib.sha256(('%s%s' % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()
            for k, a in case.items()}


def leaf_names():
    """Every leaf the gradients are taken to, in a fixed order."""
    return DATA_LEAVES + tuple('%s.%s' % (n, k) for n in NETS for k, _ in net_keys(n))


def hand_face_mask(case):
    return case['is_rhand'] | case['is_lhand'] | case['is_face']


def face_coords(case):
    """The normalised face-plane coordinates of the face rows (module.py:442-446), float64 [n_face, 3]."""
    xyz = case['pos_enc_mesh'].astype(np.float64)[case['is_face']]
    return (xyz - xyz.mean(0)) / (np.asarray(TRIPLANE_FACE_SHAPE_3D) / 2)


def knn_gaps(case, mean_offset):
    """Float64 relative gap ``(d2 - d1) / d2`` between the nearest and the second-nearest low-resolution vertex of every
    Gaussian centre ``mesh_neutral_pose + mean_offset + expression offset`` (module.py:528-543), for the vertices
    outside the hand / face mask; and the float64 nearest index of every vertex after the overwrite of module.py:546."""
    c = case
    mean = c['mesh_neutral_pose'].astype(np.float64) + np.asarray(mean_offset, dtype=np.float64) + \
        (c['expr'].astype(np.float64)[None, None, :] * c['expr_dirs'].astype(np.float64)).sum(2)
    d = np.sqrt(((mean[:, None, :] - c['mesh_lr'].astype(np.float64)[None]) ** 2).sum(2))
    order = np.argsort(d, axis=1, kind='stable')
    d1 = np.take_along_axis(d, order[:, :1], 1)[:, 0]
    d2 = np.take_along_axis(d, order[:, 1:2], 1)[:, 0]
    mask = hand_face_mask(c)
    idx = np.where(mask, np.arange(V), order[:, 0])
    return ((d2 - d1) / d2)[~mask], idx


def sample_index(name, shape):
    """Which entries of a stored tensor the fixture keeps: None (all of it), a sorted set of rows of a [V, c] tensor, or
    a sorted set of flat entries of a large gradient.  A function of the name and the shape alone."""
    n = int(np.prod(shape))
    rs = np.random.RandomState(int(hashlib.sha256(name.encode()).hexdigest()[:8], 16))
    if len(shape) == 2 and shape[0] == V:
        return 'rows', np.sort(rs.permutation(V)[:ROW_SAMPLE])
    if n > 2048:
        return 'flat', np.sort(rs.permutation(n)[:ENTRY_SAMPLE])
    return None, None


def take_sample(name, a):
    """The entries of ``a`` (numpy) the fixture keeps, as ``sample_index`` names them."""
    kind, idx = sample_index(name, a.shape)
    if kind == 'rows':
        return a[idx]
    if kind == 'flat':
        return a.reshape(-1)[idx]
    return a


def cotangents(variant, ambiguous_rows):
    """name -> float32 numpy cotangent of every output that gets one.  ``full``: all ten of ``OUTPUTS``; ``single``: only
    ``assets_refined/mean_3d``.  The rows ``ambiguous_rows`` (the fixture's ``relu/ambiguous_rows``) are zero: there a
    pre-ReLU activation of the float64 reference lies within ``RELU_MARGIN`` of 0 -- 4 times the largest error the
    reference's own float32 run commits on an activation below ``RELU_BAND`` in magnitude (1.2e-5; the generator asserts
    it) -- so whether the gradient passes that ReLU is not a fact two float32 evaluations share.  The nets, the skinning and the
    offsets work row by row, so a row without cotangents adds nothing to any gradient whichever way its ReLUs fall."""
    rs = np.random.RandomState(77)
    shapes = {n: (V, 1 if n == 'offsets/scale_offset' else 3) for n in OUTPUTS}
    G = {}
    for n in OUTPUTS:
        g = rs.randn(*shapes[n])
        g[np.asarray(ambiguous_rows, dtype=np.int64)] = 0.0
        G[n] = _f32(g)
    if variant == 'single':
        return {'assets_refined/mean_3d': G['assets_refined/mean_3d']}
    assert variant == 'full', variant
    return G


def flat_outputs(assets, assets_refined, offsets):
    """The three dicts of the forward as one ``OUTPUTS``-keyed dict."""
    d = {'assets': assets, 'assets_refined': assets_refined, 'offsets': offsets}
    return {n: d[n.split('/')[0]][n.split('/')[1]] for n in OUTPUTS}


# ---- the forward with the HIP modules ----------------------------------------------------------------------------------
class HipHuman:
    """What ``HumanGaussian.__init__`` / ``init()`` hold, built from the case on ``device``:
    buffers, the eight nets as ``nn.Sequential`` s with the case's parameters, the HIP modules over them, and ``leaves``
    (name -> the tensor that requires grad)."""

    def __init__(self, case, device):
        import exavatar_release_amd as exa
        c = case
        dev = torch.device(device)
        t = lambda k: torch.from_numpy(np.array(c[k])).to(dev)      # noqa: E731
        for k in ('pos_enc_mesh', 'skinning_weight', 'pose_dirs', 'expr_dirs', 'is_rhand', 'is_lhand', 'is_face',
                  'is_face_expr', 'is_cavity', 'mesh_lr', 'leye_pose', 'reye_pose'):
            setattr(self, k, t(k))
        self.face_upsampled = np.array(c['face_upsampled'])         # smpl_x.face_upsampled: a host array, one object
        self.cam_param = {'R': t('cam_R'), 't': t('cam_t'), 'focal': t('cam_focal'), 'princpt': t('cam_princpt')}
        self.leaves = {k: t(k).requires_grad_(True) for k in DATA_LEAVES}
        self.nets = {}
        for name in NETS:
            net = linear_layers(name)
            net.load_state_dict({k: torch.from_numpy(np.array(c['%s.%s' % (name, k)])) for k, _ in net_keys(name)})
            self.nets[name] = net.to(dev)
            for k, p in net.named_parameters():
                self.leaves['%s.%s' % (name, k)] = p
        assert tuple(self.leaves) == leaf_names()
        n = self.nets
        # HumanGaussian.init(), after the buffers are registered
        self.tri_lookup = exa.TriplaneFeatures(self.pos_enc_mesh, self.is_face, TRIPLANE_SHAPE_3D, TRIPLANE_FACE_SHAPE_3D,
                                               TRIPLANE_SHAPE)
        self.geo = exa.FusedMLP(n['geo_net'], heads=(n['mean_offset_net'], n['scale_net']))
        self.geo_off = exa.FusedMLP(n['geo_offset_net'], heads=(n['mean_offset_offset_net'], n['scale_offset_net']))
        self.rgb = exa.FusedMLP(n['rgb_net'])
        self.rgb_off = exa.FusedMLP(n['rgb_offset_net'])
        self.blend = exa.BlendShapes(self.pose_dirs, self.expr_dirs, self.is_rhand | self.is_lhand | self.is_face_expr)
        self.parents = list(PARENTS)
        # constants of the forward (module.py:545-546, 564-565)
        self.hand_face = (self.is_rhand + self.is_lhand + self.is_face) > 0
        self.arange = torch.arange(V, device=dev)
        self.rotation = p3d.matrix_to_quaternion(torch.eye(3, device=dev)[None, :, :].repeat(V, 1, 1))
        self.opacity = torch.ones((V, 1), device=dev)

    def smplx_param(self):
        p = {k: self.leaves[k] for k in POSE_LEAVES + ('expr', 'trans')}
        p['leye_pose'], p['reye_pose'] = self.leye_pose, self.reye_pose
        return p


def wire_hip(m, is_world_coord=False, capturable=False):
    """``HumanGaussian.forward`` (module.py:516-586) with every replaced piece wired as INTEGRATION.md section 5 says.
    ``capturable``: the index overwrite of module.py:546 written as a ``torch.where`` (boolean-mask indexing reads the
    mask back on the host, which a stream capture forbids); needs ``is_world_coord`` (no ``torch.inverse``).
    Returns ``(assets, assets_refined, offsets)``."""
    import exavatar_release_amd as exa
    L = m.leaves
    smplx_param, cam_param = m.smplx_param(), m.cam_param
    mesh_neutral_pose, mesh_neutral_pose_wo_upsample = L['mesh_neutral_pose'], m.mesh_lr
    transform_mat_neutral_pose, joint_zero_pose = L['transform_mat_neutral_pose'], L['joint_zero_pose']

    # extract triplane feature (module.py:424-457)
    tri_feat = m.tri_lookup(L['triplane'], L['triplane_face'])

    # get Gaussian assets (module.py:524-528)
    mean_offset, scale = m.geo(tri_feat)
    rgb = m.rgb(tri_feat)
    mean_3d = mesh_neutral_pose + mean_offset

    # forward kinematics (module.py:389-411); rot [55, 3, 3] is what module.py:464,484,498 rebuild
    pose = torch.cat((smplx_param['root_pose'].view(1, 3), smplx_param['body_pose'].view(-1, 3),
                      smplx_param['jaw_pose'].view(1, 3), smplx_param['leye_pose'].view(1, 3),
                      smplx_param['reye_pose'].view(1, 3), smplx_param['lhand_pose'].view(-1, 3),
                      smplx_param['rhand_pose'].view(-1, 3)))
    transform_mat_joint, _, rot = exa.joint_transforms(pose, joint_zero_pose, m.parents, transform_mat_neutral_pose)
    nb = JOINT_PART['body'] - 1
    pose6d = p3d.matrix_to_rotation_6d(rot[1:1 + nb]).reshape(nb * 6)                  # without root pose

    # get pose-dependent Gaussian assets (module.py:459-493, 531-534)
    mean_offset_offset, scale_offset = m.geo_off(tri_feat, pose6d.detach())
    scale, scale_refined = torch.exp(scale).repeat(1, 3), torch.exp(scale + scale_offset).repeat(1, 3)
    pose_feat = (rot[1:] - torch.eye(3, device=rot.device)[None, :, :]).view(1, (J - 1) * 9)
    mean_combined_offset, mean_offset_offset = m.blend.pose_offsets(pose_feat, mean_offset_offset)
    mean_3d_refined = mean_3d + mean_combined_offset

    # smplx facial expression offset (module.py:537-539)
    smplx_expr_offset = m.blend.expr_offsets(smplx_param['expr'])
    mean_3d = mean_3d + smplx_expr_offset
    mean_3d_refined = mean_3d_refined + smplx_expr_offset

    # get nearest vertex (module.py:543-546)
    nn_vertex_idxs = exa.knn_points(mean_3d[None, :, :], mesh_neutral_pose_wo_upsample[None, :, :], K=1,
                                    return_nn=True).idx[0, :, 0]
    if capturable:
        nn_vertex_idxs = torch.where(m.hand_face, m.arange, nn_vertex_idxs)
    else:
        mask = (m.is_rhand + m.is_lhand + m.is_face) > 0
        nn_vertex_idxs[mask] = torch.arange(V, device=mask.device)[mask]

    m.nn_vertex_idxs = nn_vertex_idxs                  # the forward keeps it to itself; the tests compare it

    # lbs and camera -> world (module.py:548-556)
    R, t = (None, None) if is_world_coord else (cam_param['R'], cam_param['t'])
    mean_3d, mean_3d_refined = exa.skin_points((mean_3d, mean_3d_refined), transform_mat_joint, m.skinning_weight,
                                               nn_vertex_idxs, smplx_param['trans'], R, t)

    # forward to rgb network (module.py:495-509, 560-561)
    with torch.no_grad():
        normal = exa.vertex_normals(mean_3d_refined, m.face_upsampled)[0]              # module.py:502
        is_cavity = m.is_cavity[:, None].float()
        normal = normal * (1 - is_cavity) + (-normal) * is_cavity
    rgb_offset = m.rgb_off(tri_feat, pose6d.detach(), normal.detach())
    rgb, rgb_refined = (torch.tanh(rgb) + 1) / 2, (torch.tanh(rgb + rgb_offset) + 1) / 2

    # Gaussians and offsets (module.py:564-585)
    if capturable:
        rotation, opacity = m.rotation, m.opacity
    else:
        rotation = p3d.matrix_to_quaternion(torch.eye(3, device=rot.device)[None, :, :].repeat(V, 1, 1))
        opacity = torch.ones((V, 1), device=rot.device)
    assets = {'mean_3d': mean_3d, 'opacity': opacity, 'scale': scale, 'rotation': rotation, 'rgb': rgb}
    assets_refined = {'mean_3d': mean_3d_refined, 'opacity': opacity, 'scale': scale_refined, 'rotation': rotation,
                      'rgb': rgb_refined}
    offsets = {'mean_offset': mean_offset, 'mean_offset_offset': mean_offset_offset, 'scale_offset': scale_offset,
               'rgb_offset': rgb_offset}
    return assets, assets_refined, offsets
