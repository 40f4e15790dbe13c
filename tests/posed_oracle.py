"""numpy restatement of the posed SMPL-X stage (include/exa_mesh.h exa_mesh_posed_*, exavatar_release_amd/posed_body.py),
independent of the HIP code and of the reference's torch expression.  The chain and the skinning are
``tests/kin_oracle.py`` and ``tests/skin_oracle.py``; the lane tree of the regressor sums is ``tests/body_oracle.py``'s.

Every function takes a ``dtype``: in float32 every line is one numpy operation, rounded and never fused, in the header's
order -- what the kernels are held to bit for bit; in float64 the same lines are the arbiter.  The one step a CPU does
not reproduce bit for bit is sin / cos of the Rodrigues angle: ``forward`` takes ``rot`` (the device's) for everything
behind that step and ``backward`` takes ``sincos`` (the device's); without them numpy's stand for the device's.

A *case* is a dict: v_template [V, 3], face_offset [V, 3] or None, shape_dirs [V, 3, L], posedirs [9 (J - 1), 3 V],
J_regressor [J, V], weights [V, J], parents, pose_mean [J, 3] or None.
"""
import numpy as np

import body_oracle
import kin_oracle
import skin_oracle

CHUNK = 256      # EXA_MESH_BODY_CHUNK
EPS = 1e-8
OUTPUTS = ('vertices', 'joints', 'vertices_world')
INPUTS = ('pose', 'betas', 'expression', 'transl', 'joint_offset')


# ---- steps 1 and 2: Rodrigues -----------------------------------------------------------------------------------------
def rod_parts(pose, pose_mean=None, dtype=np.float32):
    """f, e, a, d, K [J, 3, 3], KK [J, 3, 3]: everything of the header's steps 1 and 2 in front of sin / cos."""
    dt = np.dtype(dtype).type
    f = np.asarray(pose, dtype=dt).reshape(-1, 3)
    if pose_mean is not None:
        f = f + np.asarray(pose_mean, dtype=dt).reshape(-1, 3)
    e = f + dt(EPS)
    a = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    d = f / a[:, None]
    z = np.zeros_like(a)
    K = np.stack([z, -d[:, 2], d[:, 1], d[:, 2], z, -d[:, 0], -d[:, 1], d[:, 0], z], 1).reshape(-1, 3, 3)
    KK = np.zeros_like(K)
    for r in range(3):
        for k in range(3):
            KK[:, r, k] = (K[:, r, 0] * K[:, 0, k] + K[:, r, 1] * K[:, 1, k]) + K[:, r, 2] * K[:, 2, k]
    return dict(f=f, e=e, a=a, d=d, K=K, KK=KK)


def rodrigues(pose, pose_mean=None, dtype=np.float32, sincos=None):
    """(rot [J, 3, 3], sincos [J, 2]); ``sincos`` given: those values instead of numpy's."""
    dt = np.dtype(dtype).type
    p = rod_parts(pose, pose_mean, dt)
    if sincos is None:
        sincos = np.stack([np.sin(p['a']), np.cos(p['a'])], 1)
    sincos = np.asarray(sincos, dtype=dt)
    s, c = sincos[:, 0, None, None], sincos[:, 1, None, None]
    q = dt(1.0) - c
    rot = (np.eye(3, dtype=dt)[None] + s * p['K']) + q * p['KK']
    return rot, sincos


def rodrigues_backward(pose, pose_mean, G, sincos, dtype=np.float32):
    """dL/dpose [J, 3] from G = dL/drot [J, 3, 3], op by op as the header states it."""
    dt = np.dtype(dtype).type
    p = rod_parts(pose, pose_mean, dt)
    K, KK, a, d, e = p['K'], p['KK'], p['a'], p['d'], p['e']
    sincos = np.asarray(sincos, dtype=dt)
    s, c = sincos[:, 0], sincos[:, 1]
    q = dt(1.0) - c
    G = np.asarray(G, dtype=dt).reshape(-1, 3, 3)
    Gf, Kf, KKf = G.reshape(-1, 9), K.reshape(-1, 9), KK.reshape(-1, 9)
    gs, gq = np.zeros_like(a), np.zeros_like(a)
    for k in range(9):
        gs = gs + Gf[:, k] * Kf[:, k]
        gq = gq + Gf[:, k] * KKf[:, k]
    gK = np.zeros_like(G)
    for r in range(3):
        for k in range(3):
            X = (G[:, r, 0] * K[:, k, 0] + G[:, r, 1] * K[:, k, 1]) + G[:, r, 2] * K[:, k, 2]
            Y = (K[:, 0, r] * G[:, 0, k] + K[:, 1, r] * G[:, 1, k]) + K[:, 2, r] * G[:, 2, k]
            gK[:, r, k] = s * G[:, r, k] + q * (X + Y)
    gd = np.stack([gK[:, 2, 1] - gK[:, 1, 2], gK[:, 0, 2] - gK[:, 2, 0], gK[:, 1, 0] - gK[:, 0, 1]], 1)
    dot = (gd[:, 0] * d[:, 0] + gd[:, 1] * d[:, 1]) + gd[:, 2] * d[:, 2]
    ga = (gs * c + gq * s) - dot / a
    return gd / a[:, None] + ga[:, None] * (e / a[:, None])


# ---- the sums the stage shares with the template stage: body_oracle's ------------------------------------------------
_blend, _regress, _two_level = body_oracle.blend, body_oracle.regress, body_oracle.two_level


def _prepare(case, dt):
    f = lambda a: None if a is None else np.asarray(a, dtype=dt)      # noqa: E731
    return {k: f(case.get(k)) for k in ('v_template', 'face_offset', 'shape_dirs', 'posedirs', 'J_regressor', 'weights',
                                        'pose_mean')}


# ---- the stage --------------------------------------------------------------------------------------------------------
def forward(case, pose, betas, expression, transl, joint_offset=None, Rinv=None, t=None, dtype=np.float32, rot=None):
    """dict of the outputs (vertices, joints, vertices_world or None, rot) and the intermediates the backward reads."""
    dt = np.dtype(dtype).type
    c = _prepare(case, dt)
    parents = list(case['parents'])
    V, L = c['shape_dirs'].shape[0], c['shape_dirs'].shape[2]
    J = c['J_regressor'].shape[0]
    coef = np.concatenate([np.asarray(betas, dtype=dt).reshape(-1), np.asarray(expression, dtype=dt).reshape(-1)])
    assert coef.shape[0] == L
    transl = np.asarray(transl, dtype=dt).reshape(3)
    sincos = None
    if rot is None:
        rot, sincos = rodrigues(pose, c['pose_mean'], dt)
    rot = np.asarray(rot, dtype=dt)
    base = c['v_template'] if c['face_offset'] is None else c['v_template'] + c['face_offset']
    vs = _blend(coef, c['shape_dirs'].reshape(3 * V, L).T, base.reshape(-1), dt).reshape(V, 3)
    Jr = _regress(np.asarray(case['J_regressor']), c['J_regressor'], vs, dt)
    if joint_offset is not None:
        Jr = Jr + np.asarray(joint_offset, dtype=dt).reshape(J, 3)
    vp = vs
    if J > 1:
        feat = (rot[1:] - np.eye(3, dtype=dt)[None]).reshape(-1)
        vp = _blend(feat, c['posedirs'], vs.reshape(-1), dt).reshape(V, 3)
    A, posed = kin_oracle.forward(rot[None], Jr[None], parents, None, dt)
    vertices = skin_oracle.forward([vp], A[0], c['weights'], None, transl, None, None, dt)[0]
    joints = posed[0] + transl[None]
    world = None
    if Rinv is not None:
        R, tt = np.asarray(Rinv, dtype=dt), np.asarray(t, dtype=dt).reshape(3)
        dd = [vertices[:, k] - tt[k] for k in range(3)]
        world = np.stack([(R[r, 0] * dd[0] + R[r, 1] * dd[1]) + R[r, 2] * dd[2] for r in range(3)], 1)
    return dict(vertices=vertices, joints=joints, vertices_world=world, rot=rot, sincos=sincos, v_shaped=vs, v_posed=vp,
                Jr=Jr, A=A[0])


def backward(case, pose, fwd, cot, Rinv=None, dtype=np.float32, sincos=None, n_betas=None):
    """``cot``: {output name: cotangent or None (missing)}; ``fwd``: forward()'s dict in the same dtype; ``sincos``: the
    device's (default: the forward's own).  Returns {input name: gradient}, ``betas`` / ``expression`` split at
    ``n_betas``, every sum in the header's order."""
    dt = np.dtype(dtype).type
    c = _prepare(case, dt)
    parents = list(case['parents'])
    V, L = c['shape_dirs'].shape[0], c['shape_dirs'].shape[2]
    J = c['J_regressor'].shape[0]
    g = {k: None if cot.get(k) is None else np.asarray(cot[k], dtype=dt) for k in OUTPUTS}
    sincos = fwd['sincos'] if sincos is None else sincos
    gv = g['vertices']
    if g['vertices_world'] is not None:
        R, gw = np.asarray(Rinv, dtype=dt), g['vertices_world']
        gp = np.stack([(R[0, k] * gw[:, 0] + R[1, k] * gw[:, 1]) + R[2, k] * gw[:, 2] for k in range(3)], 1)
        gv = gp if gv is None else gv + gp
    gvp = gA = gtr = None
    if gv is not None:
        gpts, gA, gtr = skin_oracle.backward([fwd['v_posed']], [gv], fwd['A'], c['weights'], None, None, dt)
        gvp = gpts[0]
    gR = gJ = None
    if gv is not None or g['joints'] is not None:
        gR, gJ, _ = kin_oracle.backward(fwd['rot'][None], fwd['Jr'][None], parents, None,
                                        None if gA is None else gA[None],
                                        None if g['joints'] is None else g['joints'][None], dt)
        gR, gJ = gR[0], gJ[0]
    out = {}
    out['joint_offset'] = gJ if gJ is not None else np.zeros((J, 3), dtype=dt)
    dvs = gvp.copy() if gvp is not None else np.zeros((V, 3), dtype=dt)
    reg = np.asarray(case['J_regressor'])
    for j in range(J):                  # ascending joint: a vertex meets its column's non-zeros in that order
        cols = np.nonzero(reg[j])[0]
        dvs[cols] = dvs[cols] + c['J_regressor'][j, cols, None] * out['joint_offset'][j]
    dcoef = _two_level(c['shape_dirs'].reshape(3 * V, L).T, dvs.reshape(-1), dt)
    n_betas = L if n_betas is None else n_betas
    out['betas'], out['expression'] = dcoef[:n_betas], dcoef[n_betas:]
    G = gR
    if gvp is not None and J > 1:
        gfeat = _two_level(c['posedirs'], gvp.reshape(-1), dt).reshape(J - 1, 3, 3)
        if G is None:
            G = np.concatenate([np.zeros((1, 3, 3), dtype=dt), gfeat])
        else:
            G = G.copy()
            G[1:] = G[1:] + gfeat
    if G is None:
        G = np.zeros((J, 3, 3), dtype=dt)
    out['pose'] = rodrigues_backward(pose, c['pose_mean'], G, sincos, dt)
    tsum = None
    if g['joints'] is not None:
        tsum = np.zeros(3, dtype=dt)
        for j in range(J):
            tsum = tsum + g['joints'][j]
    out['transl'] = (gtr + tsum) if (gtr is not None and tsum is not None) else gtr if gtr is not None else tsum
    return out


# ---- test data --------------------------------------------------------------------------------------------------------
def random_case(verts, faces, L, parents, seed, pose_mean=True, face_offset=True, regressor='sparse'):
    """A synthetic posed body over the mesh: ``body_oracle.random_case``'s arrays plus posedirs and pose_mean."""
    case, _, _ = body_oracle.random_case(verts, faces, L, parents, 1, seed, regressor, face_offset)
    rng = np.random.RandomState(seed + 1000)
    V, J = case['v_template'].shape[0], len(parents)
    case = {k: case[k] for k in ('v_template', 'face_offset', 'shape_dirs', 'J_regressor', 'weights', 'parents')}
    case['posedirs'] = (0.01 * rng.standard_normal((9 * (J - 1), 3 * V))).astype(np.float32)
    case['pose_mean'] = (0.1 * rng.standard_normal((J, 3))).astype(np.float32) if pose_mean else None
    return case


def random_inputs(case, n_betas, seed, joint_offset=True, camera=True, zero_rows=(), pi_row=None):
    """dict(pose, betas, expression, transl, joint_offset or None, R, t or None), float32.  ``zero_rows``: joints whose
    full pose is exactly zero (their pose_mean rows must be zero); ``pi_row``: a joint whose full angle is within 1e-3 of
    pi."""
    rng = np.random.RandomState(seed)
    J, L = len(case['parents']), case['shape_dirs'].shape[2]
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32))      # noqa: E731
    pose = 0.4 * rng.standard_normal((J, 3))
    mean = np.zeros((J, 3)) if case.get('pose_mean') is None else case['pose_mean'].astype(np.float64)
    if pi_row is not None:
        axis = rng.standard_normal(3)
        pose[pi_row] = axis / np.linalg.norm(axis) * (np.pi - 4e-4) - mean[pi_row]
    pose = f32(pose)
    for j in zero_rows:
        assert not mean[j].any()
        pose[j] = 0
    coef = f32(rng.standard_normal(L))
    out = dict(pose=pose, betas=coef[:n_betas].copy(), expression=coef[n_betas:].copy(),
               transl=f32(rng.standard_normal(3)),
               joint_offset=f32(0.02 * rng.standard_normal((J, 3))) if joint_offset else None, R=None, t=None)
    if camera:
        q, r = np.linalg.qr(rng.standard_normal((3, 3)))
        out['R'] = f32(q * np.sign(np.diag(r))[None, :] + 0.05 * rng.standard_normal((3, 3)))
        out['t'] = f32(rng.standard_normal(3))
    return out


def random_cotangents(case, seed, camera=True):
    rng = np.random.RandomState(seed)
    V, J = case['v_template'].shape[0], len(case['parents'])
    cot = dict(vertices=rng.standard_normal((V, 3)).astype(np.float32), joints=rng.standard_normal((J, 3)).astype(np.float32),
               vertices_world=rng.standard_normal((V, 3)).astype(np.float32))
    if not camera:
        cot['vertices_world'] = None
    return cot


# ---- the inputs of tests/golden/ref_posed.npz (tests/golden/make_golden_posed.py) --------------------------------------
GOLDEN_SEED = 211
GOLDEN_BETAS = 7
GOLDEN_INPUTS = ('v_template', 'face_offset', 'shape_dirs', 'posedirs', 'J_regressor', 'weights', 'pose_mean', 'pose',
                 'betas', 'expression', 'transl', 'joint_offset', 'R', 't') + tuple('g_' + k for k in OUTPUTS)


def golden_inputs():
    """(case, inputs, cotangents) of the fixture: the level-3 stretched icosphere of ``body_oracle.golden_inputs()`` (642
    vertices), J = 55 with the SMPL-X tree, 7 + 5 coefficients, a pose_mean on the hands only (as ``flat_hand_mean =
    False`` has it), zero poses for both eyes and the jaw's angle within 1e-3 of pi."""
    import human_case
    from exavatar_release_amd import lbs
    verts, faces = human_case._icosphere(3)
    case = random_case(verts * np.asarray(human_case.RADII), faces, 12, lbs.SMPLX_PARENTS, GOLDEN_SEED)
    case['pose_mean'][:25] = 0
    inputs = random_inputs(case, GOLDEN_BETAS, GOLDEN_SEED + 1, zero_rows=(23, 24), pi_row=22)
    return case, inputs, random_cotangents(case, GOLDEN_SEED + 2)


def golden_digests(case, inputs, cot):
    """{input name: SHA-256 of its bytes}."""
    import hashlib
    arrays = dict(case, **inputs)
    arrays.update({'g_' + k: v for k, v in cot.items()})
    return {k: hashlib.sha256(np.ascontiguousarray(arrays[k]).tobytes()).hexdigest() for k in GOLDEN_INPUTS}


# ---- the reference's expression, restated with torch ------------------------------------------------------------------
def reference_expression(c, pose, betas, expression, transl, joint_offset=None, R=None, t=None):
    """What ``get_smplx_outputs`` evaluates, on whatever device and dtype the tensors have: ``+ pose_mean``, Rodrigues,
    the shape blend and the joint regression as einsums, the corrective matmul, one 4x4 matmul per joint, the dense
    skinning matmul, ``+ transl`` and ``inverse(R) (vertices - t)``.  ``c``: tensors v_template, face_offset, shape_dirs,
    posedirs, J_regressor, weights, pose_mean (or None); parents a list.  Returns (vertices, joints, vertices_world or
    None)."""
    import torch
    from exavatar_release_amd import body
    J, V = c['J_regressor'].shape[0], c['v_template'].shape[0]
    full = pose if c.get('pose_mean') is None else pose + c['pose_mean']
    rot = body.rodrigues(full)
    base = c['v_template'] if c.get('face_offset') is None else c['v_template'] + c['face_offset']
    v_shaped = base + torch.einsum('l,mkl->mk', torch.cat((betas, expression)), c['shape_dirs'])
    joints = torch.einsum('jv,vk->jk', c['J_regressor'], v_shaped)
    if joint_offset is not None:
        joints = joints + joint_offset
    eye = torch.eye(3, dtype=pose.dtype, device=pose.device)
    v_posed = torch.matmul((rot[1:] - eye).reshape(1, -1), c['posedirs']).view(V, 3) + v_shaped
    A, posed, _ = kin_oracle.reference_expression(rot, joints, c['parents'], None, rotations=True)
    T = torch.matmul(c['weights'], A.view(J, 16)).view(V, 4, 4)
    homo = torch.cat((v_posed, torch.ones_like(v_posed[:, :1])), 1)
    vertices = torch.matmul(T, homo[:, :, None])[:, :3, 0] + transl
    world = None
    if R is not None:
        world = torch.matmul(torch.inverse(R), (vertices - t.view(1, 3)).permute(1, 0)).permute(1, 0)
    return vertices, posed + transl, world
