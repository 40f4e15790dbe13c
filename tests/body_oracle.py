"""numpy restatement of the SMPL-X template stage and the mesh upsampling (include/exa_mesh.h exa_mesh_body_* and
exa_mesh_upsample_*, exavatar_release_amd/body.py), independent of the HIP code, of the host planner and of the
reference's torch expression.  The chains and the skinning are ``tests/kin_oracle.py`` and ``tests/skin_oracle.py``.

Every function takes a ``dtype``: in float32 every line is one numpy operation, rounded and never fused, in the header's
order -- what the kernels are held to bit for bit; in float64 the same lines are the exact semantics.  With
``magnitude=True`` (float64, fed absolute values) every subtraction becomes an addition, so every output is the sum of
the absolute values of the monomials it expands to; ``bounds`` multiplies that by K u, K the number of roundings on the
deepest path of a monomial (derived below from the sizes alone): the first-order bound of the fp32 evaluation.

A *case* is a dict: v_template [V, 3], face_offset [V, 3] or None, shape_dirs [V, 3, L], J_regressor [J, V], weights
[V, J], parents, rot_pose / rot_inverse [J, 3, 3], pose_offsets [V, 3] or None, root, faces [F, 3], levels.
"""
import numpy as np

import kin_oracle
import skin_oracle
import sum_oracle

U = 2.0 ** -24
CHUNK = 256      # EXA_MESH_BODY_CHUNK
OUTPUTS = ('mesh_upsampled', 'mesh', 'joint_neutral_pose', 'transform_mat_neutral_pose', 'joint_zero_pose')


# ---- upsampling -------------------------------------------------------------------------------------------------------
def subdivide(faces, V):
    """One round: (edges [E, 2] ascending (low, high), faces [4 F, 3]) -- vertex V + e is the midpoint of edge e."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    opposite = [(faces[:, 1], faces[:, 2]), (faces[:, 2], faces[:, 0]), (faces[:, 0], faces[:, 1])]
    pairs = sorted({(min(a, b), max(a, b)) for x, y in opposite for a, b in zip(x.tolist(), y.tolist())})
    index = {p: V + e for e, p in enumerate(pairs)}
    m = [np.array([index[(min(a, b), max(a, b))] for a, b in zip(x.tolist(), y.tolist())], dtype=np.int64).reshape(-1)
         for x, y in opposite]
    v0, v1, v2 = faces[:, 0], faces[:, 1], faces[:, 2]
    groups = [np.stack(g, 1) for g in ((v0, m[2], m[1]), (v1, m[0], m[2]), (v2, m[1], m[0]), (m[0], m[1], m[2]))]
    return np.asarray(pairs, dtype=np.int64).reshape(-1, 2), np.concatenate(groups, 0)


def plan(faces, V0, levels):
    """dict(rounds=[(V_coarse, edges)], faces, V=[V0, V1, (V2)])."""
    rounds, counts = [], [V0]
    for _ in range(levels):
        edges, faces = subdivide(faces, counts[-1])
        rounds.append((counts[-1], edges))
        counts.append(counts[-1] + edges.shape[0])
    return dict(rounds=rounds, faces=faces, V=counts)


def up_forward(x, pl, dtype=np.float32):
    """[V0, C] -> [Vn, C]: round after round, a midpoint is (a + b) * 0.5."""
    dt = np.dtype(dtype).type
    x = np.asarray(x, dtype=dt)
    for _, edges in pl['rounds']:
        x = np.concatenate([x, (x[edges[:, 0]] + x[edges[:, 1]]) * dt(0.5)], 0)
    return x


def _gather_round(g, Vc, edges, extra, dt):
    """out[p] = g[p] (extra[p] + g[p]), then its dependants' halves in ascending dependant, low parent before high."""
    out = g[:Vc].copy() if extra is None else extra + g[:Vc]
    deps = [[] for _ in range(Vc)]
    for e, (a, b) in enumerate(edges.tolist()):
        deps[a].append(Vc + e)
        deps[b].append(Vc + e)
    width = max([len(d) for d in deps] + [0])
    for k in range(width):              # the k-th dependant of every vertex that has one
        rows = np.array([p for p in range(Vc) if len(deps[p]) > k], dtype=np.int64)
        out[rows] = out[rows] + g[[deps[p][k] for p in rows]] * dt(0.5)
    return out


def up_backward(g, pl, g_extra=None, dtype=np.float32):
    """[Vn, C] (and g_extra [V0, C]) -> [V0, C], the finer round first."""
    dt = np.dtype(dtype).type
    h = np.asarray(g, dtype=dt)
    rounds = pl['rounds']
    for i in range(len(rounds) - 1, -1, -1):
        extra = None if (i > 0 or g_extra is None) else np.asarray(g_extra, dtype=dt)
        h = _gather_round(h, rounds[i][0], rounds[i][1], extra, dt)
    return h


def max_dependants(pl):
    return [int(np.bincount(edges.reshape(-1), minlength=1).max()) if edges.size else 0 for _, edges in pl['rounds']]


# ---- the sums the stage shares with the posed stage (tests/posed_oracle.py) -------------------------------------------
def blend(coef, dirs, base, dt):
    """base [M] + the sum over the rows of dirs [n, M] from +0.0 in ascending row."""
    s = np.zeros(dirs.shape[1], dtype=dt)
    for l in range(dirs.shape[0]):
        s = s + coef[l] * dirs[l]
    return base + s


def regress(reg, reg_dt, vs, dt):
    """[J, 3]: every row of the regressor over its non-zeros, lanes then the tree."""
    Jr = np.zeros((reg.shape[0], 3), dtype=dt)
    for j in range(reg.shape[0]):
        cols = np.nonzero(reg[j])[0]
        vals = reg_dt[j, cols]
        p = np.zeros((64, 3), dtype=dt)
        for i0 in range(0, cols.size, 64):
            n = min(64, cols.size - i0)
            p[:n] = p[:n] + vals[i0:i0 + n, None] * vs[cols[i0:i0 + n]]
        Jr[j] = sum_oracle.tree(p.T)
    return Jr


def two_level(T, g, dt):
    """[n]: sum_m T[l][m] g[m] over chunks of 256 (lanes, the tree per wave, the four waves), then the chunks in order."""
    n, M = T.shape
    chunks = -(-M // CHUNK)
    gq = np.zeros(chunks * CHUNK, dtype=dt)
    gq[:M] = g
    Tp = np.zeros((n, chunks * CHUNK), dtype=dt)
    Tp[:, :M] = T
    partial = sum_oracle.waves(sum_oracle.tree((Tp * gq[None]).reshape(n, chunks, 4, 64)))
    out = np.zeros(n, dtype=dt)
    for ch in range(chunks):
        out = out + partial[:, ch]
    return out


# ---- the stage --------------------------------------------------------------------------------------------------------
def _prepare(case, dt, magnitude):
    f = (lambda a: None if a is None else np.abs(np.asarray(a, dtype=dt))) if magnitude else \
        (lambda a: None if a is None else np.asarray(a, dtype=dt))
    return {k: f(case[k]) for k in ('v_template', 'face_offset', 'shape_dirs', 'J_regressor', 'weights', 'rot_pose',
                                    'rot_inverse', 'pose_offsets')}


def forward(case, coef, joint_offset, dtype=np.float32, magnitude=False):
    """dict of the five outputs and the intermediates (v_shaped, v_posed, Jr, A)."""
    dt = np.dtype(dtype).type
    c = _prepare(case, dt, magnitude)
    ab = np.abs if magnitude else (lambda a: a)
    coef, jo = ab(np.asarray(coef, dtype=dt).reshape(-1)), ab(np.asarray(joint_offset, dtype=dt).reshape(-1, 3))
    parents, root = list(case['parents']), case['root']
    V, L = c['shape_dirs'].shape[0], c['shape_dirs'].shape[2]
    J = c['J_regressor'].shape[0]
    base = c['v_template'] if c['face_offset'] is None else c['v_template'] + c['face_offset']
    vs = blend(coef, c['shape_dirs'].reshape(3 * V, L).T, base.reshape(-1), dt).reshape(V, 3)
    vp = vs if c['pose_offsets'] is None else vs + c['pose_offsets']
    Jr = regress(np.asarray(case['J_regressor']), c['J_regressor'], vs, dt)
    others = np.arange(J) != root                  # the root's joint gets no offset (not even + 0)
    Jr[others] = Jr[others] + jo[others]
    A, jnp = kin_oracle.forward(c['rot_pose'][None], Jr[None], parents, None, dt, magnitude)
    mesh = skin_oracle.forward([vp], A[0], c['weights'], None, None, None, None, dt)[0]
    pl = plan(case['faces'], V, case['levels'])
    tm, _ = kin_oracle.forward(c['rot_inverse'][None], jnp, parents, None, dt, magnitude)
    eye = np.broadcast_to(np.eye(3, dtype=dt), (1, J, 3, 3))
    _, jzp = kin_oracle.forward(eye, Jr[None], parents, None, dt, magnitude)
    return dict(mesh_upsampled=up_forward(mesh, pl, dt), mesh=mesh, joint_neutral_pose=jnp[0],
                transform_mat_neutral_pose=tm[0], joint_zero_pose=jzp[0], v_shaped=vs, v_posed=vp, Jr=Jr, A=A[0], plan=pl)


def backward(case, fwd, cot, dtype=np.float32, magnitude=False, want_coef=True):
    """``cot``: {output name: cotangent or None (missing)}; ``fwd``: forward()'s dict in the same mode.  Returns
    (dL/dcoef [L] or None, dL/djoint_offset [J, 3]), every sum in the header's order."""
    dt = np.dtype(dtype).type
    c = _prepare(case, dt, magnitude)
    g = {k: None if cot.get(k) is None else (np.abs if magnitude else np.asarray)(np.asarray(cot[k], dtype=dt))
         for k in OUTPUTS}
    parents, root = list(case['parents']), case['root']
    V, L = c['shape_dirs'].shape[0], c['shape_dirs'].shape[2]
    J = c['J_regressor'].shape[0]
    kin_grad_joints = lambda rot, joints, gT, gp: kin_oracle.backward(      # noqa: E731
        rot[None], joints[None], parents, None, None if gT is None else gT[None], None if gp is None else gp[None], dt,
        magnitude)[1][0]
    gB = None
    if g['transform_mat_neutral_pose'] is not None:
        gB = kin_grad_joints(c['rot_inverse'], fwd['joint_neutral_pose'], g['transform_mat_neutral_pose'], None)
    have_mesh = g['mesh_upsampled'] is not None or g['mesh'] is not None
    gvp = gA = None
    if have_mesh:
        gm = g['mesh']
        if g['mesh_upsampled'] is not None:
            gm = up_backward(g['mesh_upsampled'], fwd['plan'], g['mesh'], dt)
        gpts, gA, _ = skin_oracle.backward([fwd['v_posed']], [gm], fwd['A'], c['weights'], None, None, dt)
        gvp = gpts[0]
    gpA = g['joint_neutral_pose']
    if gpA is not None and gB is not None:
        gpA = gpA + gB
    elif gB is not None:
        gpA = gB
    gJA = gJC = None
    if have_mesh or gpA is not None:
        gJA = kin_grad_joints(c['rot_pose'], fwd['Jr'], gA, gpA)
    if g['joint_zero_pose'] is not None:
        gJC = kin_grad_joints(np.eye(3, dtype=dt)[None].repeat(J, 0), fwd['Jr'], None, g['joint_zero_pose'])
    if gJA is not None and gJC is not None:
        dJ = gJA + gJC
    else:
        dJ = gJA if gJA is not None else gJC if gJC is not None else np.zeros((J, 3), dtype=dt)
    djo = dJ.copy()
    djo[root] = 0
    if not want_coef:
        return None, djo
    dvs = gvp.copy() if gvp is not None else np.zeros((V, 3), dtype=dt)
    reg = np.asarray(case['J_regressor'])
    for j in range(J):                  # ascending joint: a vertex meets its column's non-zeros in that order
        cols = np.nonzero(reg[j])[0]
        dvs[cols] = dvs[cols] + c['J_regressor'][j, cols, None] * dJ[j]
    return two_level(c['shape_dirs'].reshape(3 * V, L).T, dvs.reshape(-1), dt), djo


# ---- first-order error bounds: |fp32 - exact| <= K u * magnitude ------------------------------------------------------
def roundings(case, extra=0):
    """K per output and per gradient: the roundings on the deepest path of a monomial, from the sizes alone.  ``extra``
    is added everywhere (roundings of the inputs themselves, when they are not exactly the other side's).

    Forward.  v_shaped: the product, at most L additions of the sum, the base's own addition and the final one: L + 3.
    Jr: a product, ceil(n / 64) additions in the lane (n the longest regressor row), 6 in the tree, 1 for the offset.
    v_posed: 1.  A chain adds kin_oracle.k_forward(D) to what its joints carry.  The mesh's monomials are w A x: the
    roundings of A, of v_posed and skin_oracle.k_forward(J).  A round of upsampling: one addition (the half is exact).
    Backward.  A monomial carries the roundings of its forward factor and those of the cotangent's path: the stages'
    own counts (kin_oracle.k_backward, skin_oracle.k_grad_points / k_grad_sums), one addition per dependant and round of
    the upsampling (+1 for g_extra), one per joint-gradient sum, a product and one addition per non-zero of the
    longest regressor column, and for dL/dcoef a product, 6 + 3 additions in the chunk and one per chunk."""
    reg = np.asarray(case['J_regressor'])
    V, L = case['shape_dirs'].shape[0], case['shape_dirs'].shape[2]
    J = reg.shape[0]
    D = max(kin_oracle.depths(list(case['parents'])))
    n_row = int((reg != 0).sum(1).max())
    n_col = int((reg != 0).sum(0).max())
    deg = max_dependants(plan(case['faces'], V, case['levels']))
    kf, kb = kin_oracle.k_forward(D, False), kin_oracle.k_backward(D, J, False)
    k_vs = L + 3
    k_J = k_vs + 1 + -(-n_row // 64) + 6 + 1
    k_vp = k_vs + 1
    k_A = k_J + kf
    k_mesh = k_A + k_vp + skin_oracle.k_forward(J)
    k_gB = kb + k_A
    k_gm = sum(d + 1 for d in deg) + 1
    k_gvp = skin_oracle.k_grad_points(J) + k_A + k_gm
    k_gA = skin_oracle.k_grad_sums(V, 1) + k_vp + k_gm
    k_gJA = kb + k_A + max(k_gA, k_gB + 1)
    k_gJC = kb + k_J + kf
    k_dJ = max(k_gJA, k_gJC) + 1
    k_dvs = max(k_gvp, k_dJ + 1 + n_col) + 1
    k = dict(mesh_upsampled=k_mesh + case['levels'], mesh=k_mesh, joint_neutral_pose=k_A,
             transform_mat_neutral_pose=k_A + kf, joint_zero_pose=k_J + kf, joint_offset=k_dJ,
             coef=k_dvs + 1 + 6 + 3 + -(-3 * V // CHUNK))
    return {n: v + extra for n, v in k.items()}


def exact(case, coef, joint_offset, cot, extra=0):
    """float64: {name: (value, first-order bound of the fp32 evaluation)} for the five outputs and, under 'coef' and
    'joint_offset', the two gradients."""
    val = forward(case, coef, joint_offset, np.float64)
    mag = forward(case, coef, joint_offset, np.float64, True)
    dval = backward(case, val, cot, np.float64)
    dmag = backward(case, mag, cot, np.float64, True)
    K = roundings(case, extra)
    out = {n: (val[n], K[n] * U * mag[n]) for n in OUTPUTS}
    out['coef'] = (dval[0], K['coef'] * U * dmag[0])
    out['joint_offset'] = (dval[1], K['joint_offset'] * U * dmag[1])
    return out


# ---- test data --------------------------------------------------------------------------------------------------------
def triangle():
    return np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.2], [0.3, 1.0, -0.1]]), np.array([[0, 1, 2]], dtype=np.int64)


def grid(rows, cols):
    """An open rows x cols grid, two triangles per cell."""
    y, x = np.mgrid[0:rows, 0:cols]
    verts = np.stack([x.ravel() / max(cols - 1, 1) - 0.5, y.ravel() / max(rows - 1, 1) - 0.5,
                      0.1 * np.sin(x.ravel() + 0.5 * y.ravel())], 1)
    i = (y[:-1, :-1] * cols + x[:-1, :-1]).ravel()
    faces = np.concatenate([np.stack([i, i + 1, i + cols], 1), np.stack([i + 1, i + cols + 1, i + cols], 1)], 0)
    return verts, faces.astype(np.int64)


def strip(n):
    """An open triangle strip of n >= 3 vertices (any vertex count)."""
    i = np.arange(n)
    verts = np.stack([i / n - 0.5, 0.2 * (i % 2) + 0.3 * np.cos(0.07 * i), 0.1 * np.sin(0.3 * i)], 1)
    f = np.arange(n - 2)
    faces = np.where((f % 2 == 0)[:, None], np.stack([f, f + 1, f + 2], 1), np.stack([f + 1, f, f + 2], 1))
    return verts, faces.astype(np.int64)


def chain_tree(J):
    return [-1] + list(range(J - 1))


def star_tree(J):
    return [-1] + [0] * (J - 1)


def random_case(verts, faces, L, parents, levels, seed, regressor='sparse', offsets=True, root=0, nnz=30):
    """A synthetic body over the mesh (verts [V, 3] float64, faces): every array float32, drawn with RandomState.
    regressor: 'sparse' (min(nnz, V) positive weights per joint that sum to 1) or 'rows' (joint 0 empty, joint 1 one
    entry, joint 2 -- where there is one -- dense, the others sparse).  Returns (case, coef, joint_offset)."""
    rng = np.random.RandomState(seed)
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32))      # noqa: E731
    V, J = verts.shape[0], len(parents)
    reg = np.zeros((J, V))
    for j in range(J):
        n = min(nnz, V)
        if regressor == 'rows':
            n = (0, 1, V)[j] if j < 3 else n
        cols = rng.choice(V, size=n, replace=False)
        w = rng.uniform(0.2, 1.0, size=n)
        reg[j, cols] = w / max(w.sum(), 1e-30)
    logits = np.full((V, J), -np.inf)
    for v in range(V):
        logits[v, rng.choice(J, size=min(4, J), replace=False)] = rng.standard_normal(min(4, J))
    w = np.exp(logits - logits.max(1, keepdims=True))
    pose = f32(0.4 * rng.standard_normal((J, 3)))
    rot = kin_oracle.axis_angle_to_matrix(pose, np.float32)
    case = dict(v_template=f32(verts), face_offset=f32(0.01 * rng.standard_normal((V, 3))) if offsets else None,
                shape_dirs=f32(0.03 * rng.standard_normal((V, 3, L))), J_regressor=f32(reg),
                weights=f32(w / w.sum(1, keepdims=True)), parents=list(parents), rot_pose=rot,
                rot_inverse=np.ascontiguousarray(np.swapaxes(rot, 1, 2)),
                pose_offsets=f32(0.01 * rng.standard_normal((V, 3))) if offsets else None, root=root,
                faces=np.asarray(faces, dtype=np.int64), levels=levels)
    return case, f32(rng.standard_normal(L)), f32(0.02 * rng.standard_normal((J, 3)))


def random_cotangents(case, seed, present=OUTPUTS):
    """{output: cotangent float32, or None for the outputs not in ``present``}."""
    rng = np.random.RandomState(seed)
    V, J = case['v_template'].shape[0], len(case['parents'])
    Vn = plan(case['faces'], V, case['levels'])['V'][-1]
    shapes = dict(mesh_upsampled=(Vn, 3), mesh=(V, 3), joint_neutral_pose=(J, 3), transform_mat_neutral_pose=(J, 4, 4),
                  joint_zero_pose=(J, 3))
    full = {k: rng.standard_normal(shapes[k]).astype(np.float32) for k in OUTPUTS}
    return {k: full[k] if k in present else None for k in OUTPUTS}


# ---- the inputs of tests/golden/ref_body.npz (tests/golden/make_golden_body.py) ----------------------------------------
GOLDEN_SEED = 11
GOLDEN_INPUTS = ('v_template', 'face_offset', 'shape_dirs', 'J_regressor', 'weights', 'faces', 'pose', 'posedirs', 'coef',
                 'joint_offset') + tuple('g_' + k for k in OUTPUTS)


def golden_inputs():
    """(case, coef, joint_offset, cotangents) of the fixture: a level-3 stretched icosphere (642 vertices, 1280 faces,
    10 242 after two rounds), J = 55 with the SMPL-X tree, L = 100, 30 non-zeros per regressor row, four-joint softmax
    weights; ``case['pose']`` [55, 3] is the constant big pose (body joints only, as the reference's) and
    ``case['posedirs']`` [486, 3 V] its pose-corrective directions.  The three pose constants are None: they follow from
    the pose (``exavatar_release_amd.body.pose_constants``), and the fixture stores the reference's."""
    import human_case
    from exavatar_release_amd import lbs
    verts, faces = human_case._icosphere(3)
    case, coef, jo = random_case(verts * np.asarray(human_case.RADII), faces, 100, lbs.SMPLX_PARENTS, 2, GOLDEN_SEED)
    rng = np.random.RandomState(GOLDEN_SEED + 1)
    pose = np.zeros((55, 3), dtype=np.float32)
    pose[1:22] = (0.3 * rng.standard_normal((21, 3))).astype(np.float32)
    case['pose'] = pose
    case['posedirs'] = (0.01 * rng.standard_normal((54 * 9, 3 * verts.shape[0]))).astype(np.float32)
    case['rot_pose'] = case['rot_inverse'] = case['pose_offsets'] = None
    return case, coef, jo, random_cotangents(case, GOLDEN_SEED + 2)


def golden_digests(case, coef, jo, cot):
    """{input name: SHA-256 of its bytes}."""
    import hashlib
    arrays = dict(case, coef=coef, joint_offset=jo, **{'g_' + k: v for k, v in cot.items()})
    return {k: hashlib.sha256(np.ascontiguousarray(arrays[k]).tobytes()).hexdigest() for k in GOLDEN_INPUTS}


# ---- the reference's expression, restated with torch ------------------------------------------------------------------
def reference_expression(c, coef, joint_offset, subdividers):
    """What ``get_neutral_pose_human(True, True)`` + ``get_zero_pose_human()`` evaluate, on whatever device and dtype the
    tensors have: two full ``lbs`` (shape blend and joint regression as einsums, the pose correctives, one 4x4 matmul per
    joint, the dense skinning matmul), a third chain over the inverse rotations and the ``SubdivideMeshes`` stand-ins in
    ``subdividers``, nothing shared between the two ``lbs``.  ``c``: tensors v_template, face_offset, shape_dirs,
    J_regressor, weights, rot_inverse [J, 3, 3], and either pose [J, 3] + posedirs [9 (J - 1), 3 V] (Rodrigues and the
    corrective matmul run, as in the reference) or rot_pose + pose_offsets (the constants); parents a list; root.  Returns
    the five outputs in OUTPUTS' order."""
    import torch
    from exavatar_release_amd import body, p3d_standins
    J, V = c['J_regressor'].shape[0], c['v_template'].shape[0]
    keep = torch.ones(J, 1, dtype=coef.dtype, device=coef.device)
    keep[c['root']] = 0
    eye = torch.eye(3, dtype=coef.dtype, device=coef.device)

    def lbs(rot, pose_offsets):
        base = c['v_template'] if c.get('face_offset') is None else c['v_template'] + c['face_offset']
        v_shaped = base + torch.einsum('l,mkl->mk', coef, c['shape_dirs'])
        joints = torch.einsum('jv,vk->jk', c['J_regressor'], v_shaped) + joint_offset * keep
        if pose_offsets is None and c.get('posedirs') is not None:
            pose_offsets = torch.matmul((rot[1:] - eye).reshape(1, -1), c['posedirs']).view(V, 3)
        v_posed = v_shaped if pose_offsets is None else v_shaped + pose_offsets
        A, posed, _ = kin_oracle.reference_expression(rot, joints, c['parents'], None, rotations=True)
        T = torch.matmul(c['weights'], A.view(J, 16)).view(V, 4, 4)
        homo = torch.cat((v_posed, torch.ones_like(v_posed[:, :1])), 1)
        return torch.matmul(T, homo[:, :, None])[:, :3, 0], posed

    if c.get('pose') is not None:
        mesh, jnp = lbs(body.rodrigues(c['pose']), None)
        _, jzp = lbs(body.rodrigues(torch.zeros_like(c['pose'])), None)
    else:
        mesh, jnp = lbs(c['rot_pose'], c.get('pose_offsets'))
        _, jzp = lbs(eye.expand(J, 3, 3), torch.zeros_like(c['v_template']))
    m = p3d_standins.Meshes(mesh[None], subdividers[0]._subdivided_faces.new_zeros(1, 1, 3))
    for sub in subdividers:
        m = sub(m)
    tm, _, _ = kin_oracle.reference_expression(c['rot_inverse'], jnp, c['parents'], None, rotations=True)
    return m.verts_padded()[0], mesh, jnp, tm, jzp


def stand_in_subdividers(verts, faces, levels):
    """The chained ``SubdivideMeshes`` stand-ins of ``smpl_x.get_subdivider`` (CPU; move them with ``.to()``)."""
    import torch
    from exavatar_release_amd import p3d_standins
    mesh = p3d_standins.Meshes(torch.as_tensor(verts, dtype=torch.float32)[None], torch.as_tensor(faces)[None])
    subs = [p3d_standins.SubdivideMeshes(mesh)]
    for _ in range(levels - 1):
        mesh = subs[-1](mesh)
        subs.append(p3d_standins.SubdivideMeshes(mesh))
    return subs
