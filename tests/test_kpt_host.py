"""The host side of the keypoint path (exavatar_release_amd/keypoints.py, csrc/keypoints.hip): the compiled tables against a
hand-written answer and against a brute-force transpose of the oracle's rows, ``from_layer`` on stub layers, every refusal by
name (index ranges, the 79 rows, ``rot`` missing with ``Ld > 0``, shapes, devices, a table that requires grad; no GPU work:
there is no GPU here), the library's size checks, and the wiring (exports, build flags, buffers)."""
import ctypes
import re
import types

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import _lib, build
from exavatar_release_amd import keypoints as module
from tests import kpt_oracle as ko

NAMES = ('BodyKeypoints', 'KeypointOutput', 'CoordLoss')


def test_exports_build_flags_and_constants():
    for name in NAMES:
        assert name in exa.__all__ and getattr(exa, name) is getattr(module, name)
    assert build.SOURCES['keypoints.hip'] == ['-ffp-contract=off']
    header = open(build.os.path.join(build.HERE, '..', 'include', 'exa_mesh.h')).read()
    assert int(re.search(r'#define EXA_MESH_KPT_ROWS (\d+)', header).group(1)) == module.ROWS == ko.fit_oracle.BLOCK
    assert int(re.search(r'#define EXA_MESH_KPT_BINS (\d+)', header).group(1)) == module.BINS == ko.BINS
    for i, name in enumerate(('JOINT', 'VERTEX', 'STATIC', 'DYNAMIC')):
        assert int(re.search(r'#define EXA_MESH_KPT_%s (\d+)' % name, header).group(1)) == getattr(module, name) == i
    lib = _lib.load()
    assert [lib.exa_mesh_keypoints_blocks(v) for v in (-1, 0, 1, 256, 257, 65537)] == [0, 0, 1, 1, 2, 257]
    assert _lib.size_query(_lib.MESH, 'exa_mesh_keypoints_workspace_size', 2, 300, 5) == 768      # rows 2 * 11 * 3 floats -> 512, partials 2 * 3 * 2 floats -> 256


def hand_written():
    """V = 5, J = 2, faces (0,1,2), (2,3,4); rows: 2 joints, vertex 4, landmark on face 1, one dynamic slot, appended vertex 2."""
    dyn_f = np.zeros((79, 1), np.int64)
    dyn_f[3, 0] = 1
    dyn_w = np.tile(np.array([[[0.5, 0.25, 0.25]]], np.float32), (79, 1, 1))
    return dict(num_vertices=5, num_joints=2, faces=[[0, 1, 2], [2, 3, 4]], extra_vertices=[4], lmk_faces_idx=[1],
                lmk_bary_coords=np.array([[0.2, 0.3, 0.5]], np.float32), dynamic_lmk_faces_idx=dyn_f,
                dynamic_lmk_bary_coords=dyn_w, neck_kin_chain=[1, 0], append_vertices=[2])


def test_the_tables_of_a_hand_written_selection():
    m = exa.BodyKeypoints(kpt_idx=[5, 1, 3, 4, 1, 2], root_idx=3, **hand_written())
    assert (m.num_rows, m.num_keypoints, m.num_dynamic, m.chain_length) == (6, 6, 1, 2)
    assert m.state_dict() == {} and {n for n, _ in m.named_buffers()} == set(m.TABLES)
    assert m.rec.dtype == torch.int32 and m.rec_w.dtype == torch.float32
    # record 6 is the root (row 3, the static landmark)
    assert m.rec.tolist() == [[1, 2, 0, 0], [0, 1, 0, 0], [2, 2, 3, 4], [3, 0, 0, 0], [0, 1, 0, 0], [1, 4, 0, 0], [2, 2, 3, 4]]
    assert m.rec_w[2].tolist() == m.rec_w[6].tolist() == pytest.approx([0.2, 0.3, 0.5])
    assert m.dyn_vtx[0, 0].tolist() == [0, 1, 2] and m.dyn_vtx[3, 0].tolist() == [2, 3, 4]
    assert m.joff.tolist() == [0, 0, 2] and m.jent.tolist() == [1, 4]
    # touched vertices 0 .. 4; vertex 2: record 0 (vertex), record 2 corner 0, record 3 corner 2 in 78 bins and corner 0 in bin 3,
    # record 6 corner 0
    assert m.vrow.tolist() == [0, 1, 2, 3, 4] and m.num_touched == 5
    lo, hi = m.voff[2].item(), m.voff[3].item()
    ks, bins = m.vent_k[lo:hi].tolist(), m.vent_bin[lo:hi].tolist()
    assert ks == [0, 2] + [3] * 79 + [6] and bins[:2] == [-1, -1] and bins[-1] == -1
    assert bins[2:-1] == [3] + [b for b in range(79) if b != 3]      # ascending (corner, bin): corner 0 is bin 3's, corner 2 the others'
    assert m.vent_w[lo].item() == 1.0 and m.vent_w[lo + 1].item() == pytest.approx(0.2)
    # vertex 4: record 2 corner 2, record 3 corner 2 in bin 3, record 5 (vertex), record 6 corner 2
    lo, hi = m.voff[4].item(), m.voff[5].item()
    assert m.vent_k[lo:hi].tolist() == [2, 3, 5, 6] and m.vent_bin[lo:hi].tolist() == [-1, 3, -1, -1]
    # an untouched vertex and an empty selection
    m = exa.BodyKeypoints(kpt_idx=[], root_idx=0, **hand_written())
    assert m.num_keypoints == 0 and m.vrow.tolist() == [-1] * 5 and m.voff.tolist() == [0] and m.joff.tolist() == [0, 1, 1]
    assert exa.BodyKeypoints(**hand_written()).num_keypoints == 6


@pytest.mark.parametrize('seed,V,K,Ld', [(1, 40, 30, 17), (2, 300, 135, 17), (3, 7, 9, 0)])
def test_the_transpose_equals_a_brute_force_over_the_oracles_rows(seed, V, K, Ld):
    c = ko.kpt_case(seed, 1, V, 5, K, Ld, duplicates=True)
    s = c['spec']
    m = exa.BodyKeypoints(**ko.module_args(s))
    sel, root = ko.rows_of(s)
    want = {}
    for k, row in enumerate(sel + [root]):
        if row[0] == 'v':
            want.setdefault(row[1], []).append((k, 0, -1, 1.0))
        elif row[0] == 's':
            v, w = ko.corners(s, row, 0)
            for corner in range(3):
                want.setdefault(int(v[corner]), []).append((k, corner, -1, float(w[corner])))
        elif row[0] == 'd':
            for b in range(ko.BINS):
                v, w = ko.corners(s, row, b)
                for corner in range(3):
                    want.setdefault(int(v[corner]), []).append((k, corner, b, float(w[corner])))
    assert m.num_touched == len(want)
    for v in range(V):
        t = m.vrow[v].item()
        if v not in want:
            assert t == -1
            continue
        lo, hi = m.voff[t].item(), m.voff[t + 1].item()
        entries = sorted(want[v])
        assert m.vent_k[lo:hi].tolist() == [e[0] for e in entries] and m.vent_bin[lo:hi].tolist() == [e[2] for e in entries]
        assert m.vent_w[lo:hi].tolist() == [np.float32(e[3]) for e in entries]
    for j in range(5):
        assert m.jent[m.joff[j]:m.joff[j + 1]].tolist() == [k for k, row in enumerate(sel + [root]) if row == ('j', j)]


# ---- from_layer -------------------------------------------------------------------------------------------------------------
def stub_layer(contour, extra):
    rs = np.random.RandomState(0)
    layer = types.SimpleNamespace(
        v_template=torch.zeros(20, 3), J_regressor=torch.zeros(4, 20), faces_tensor=torch.from_numpy(ko.faces_of(rs, 20, 30)),
        vertex_joint_selector=types.SimpleNamespace(extra_joints_idxs=torch.tensor(extra, dtype=torch.long)),
        lmk_faces_idx=torch.tensor([3, 7], dtype=torch.long), lmk_bary_coords=torch.tensor([[0.2, 0.3, 0.5], [1.0, 0.0, 0.0]]),
        use_face_contour=contour)
    if contour:
        layer.dynamic_lmk_faces_idx = torch.from_numpy(rs.randint(0, 30, (79, 3)))
        layer.dynamic_lmk_bary_coords = torch.from_numpy(ko.f32(rs.dirichlet(np.ones(3), (79, 3))))
        layer.neck_kin_chain = torch.tensor([2, 1, 0], dtype=torch.long)
    return layer


def test_from_layer_on_stub_smplx_and_flame_layers():
    smplx = exa.BodyKeypoints.from_layer(stub_layer(True, [5, 6, 7]), kpt_idx=[0, 11, 4, 8], root_idx=1)
    assert (smplx.num_vertices, smplx.num_joints, smplx.num_rows, smplx.num_keypoints, smplx.num_dynamic) == (20, 4, 12, 4, 3)
    assert smplx.rec[:, 0].tolist() == [module.JOINT, module.DYNAMIC, module.VERTEX, module.STATIC, module.JOINT]
    assert smplx.chain.tolist() == [2, 1, 0]
    # FLAME as the fitting uses it: no extra joints, no contour, lear / rear appended (model.py:143-145)
    flame = exa.BodyKeypoints.from_layer(stub_layer(False, []), append_vertices=[18, 19])
    assert (flame.num_rows, flame.num_keypoints, flame.num_dynamic, flame.chain_length) == (4 + 2 + 2, 8, 0, 0)
    assert flame.rec[6:8].tolist() == [[module.VERTEX, 18, 0, 0], [module.VERTEX, 19, 0, 0]]
    with pytest.raises(ValueError, match=r'BodyKeypoints: rot is required with dynamic landmarks \(Ld = 3\)'):
        smplx(torch.zeros(1, 20, 3), torch.zeros(1, 4, 3))


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_every_index_is_checked_on_the_host():
    base = hand_written()
    bad = lambda **kw: exa.BodyKeypoints(**dict(base, **kw))      # noqa: E731
    with pytest.raises(ValueError, match=r'BodyKeypoints: faces holds 5, outside \[0, 5\) \(the vertices\)'):
        bad(faces=[[0, 1, 5], [2, 3, 4]])
    with pytest.raises(ValueError, match=r'BodyKeypoints: extra_vertices holds -1, outside \[0, 5\)'):
        bad(extra_vertices=[-1])
    with pytest.raises(ValueError, match=r'BodyKeypoints: append_vertices holds 7, outside \[0, 5\)'):
        bad(append_vertices=[7])
    with pytest.raises(ValueError, match=r'BodyKeypoints: lmk_faces_idx holds 2, outside \[0, 2\) \(the faces\)'):
        bad(lmk_faces_idx=[2])
    dyn = base['dynamic_lmk_faces_idx'].copy()
    dyn[78, 0] = 2
    with pytest.raises(ValueError, match=r'BodyKeypoints: dynamic_lmk_faces_idx holds 2, outside \[0, 2\)'):
        bad(dynamic_lmk_faces_idx=dyn)
    with pytest.raises(ValueError, match=r'BodyKeypoints: neck_kin_chain holds 2, outside \[0, 2\) \(the joints\)'):
        bad(neck_kin_chain=[1, 2])
    with pytest.raises(ValueError, match=r'BodyKeypoints: kpt_idx holds 6, outside \[0, 6\)'):
        bad(kpt_idx=[0, 6])
    with pytest.raises(ValueError, match=r'BodyKeypoints: kpt_idx holds -1, outside \[0, 6\)'):
        bad(kpt_idx=[-1])
    with pytest.raises(ValueError, match=r'BodyKeypoints: root_idx holds 6, outside \[0, 6\)'):
        bad(root_idx=6)
    with pytest.raises(ValueError, match='BodyKeypoints: root_idx must be an integer >= 0'):
        bad(root_idx=-1)
    with pytest.raises(ValueError, match=r'BodyKeypoints: dynamic_lmk_faces_idx must have 79 rows, the yaw bins of the layer \(it has 78\)'):
        bad(dynamic_lmk_faces_idx=base['dynamic_lmk_faces_idx'][:78], dynamic_lmk_bary_coords=base['dynamic_lmk_bary_coords'][:78])
    with pytest.raises(ValueError, match=r'BodyKeypoints: dynamic_lmk_bary_coords must be \[79, 1, 3\]'):
        bad(dynamic_lmk_bary_coords=base['dynamic_lmk_bary_coords'][:, :, :2])
    with pytest.raises(ValueError, match='BodyKeypoints: dynamic_lmk_faces_idx and dynamic_lmk_bary_coords come together'):
        bad(dynamic_lmk_bary_coords=None)
    with pytest.raises(ValueError, match='BodyKeypoints: neck_kin_chain is required with dynamic landmarks'):
        bad(neck_kin_chain=[])
    with pytest.raises(ValueError, match='BodyKeypoints: faces is required with landmarks'):
        bad(faces=None)
    with pytest.raises(ValueError, match=r'BodyKeypoints: lmk_bary_coords must be \[1, 3\]'):
        bad(lmk_bary_coords=np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError, match='BodyKeypoints: lmk_bary_coords is a buffer in the reference and gets no gradient'):
        bad(lmk_bary_coords=torch.zeros(1, 3, requires_grad=True))
    with pytest.raises(ValueError, match='BodyKeypoints: dynamic_lmk_bary_coords is a buffer in the reference'):
        bad(dynamic_lmk_bary_coords=torch.zeros(79, 1, 3, requires_grad=True))
    with pytest.raises(ValueError, match='BodyKeypoints: lmk_faces_idx must hold integers'):
        bad(lmk_faces_idx=np.zeros(1, np.float32))
    with pytest.raises(ValueError, match='BodyKeypoints: num_vertices must be an integer >= 0'):
        bad(num_vertices=-5)


def test_the_python_surface_refuses_what_it_does_not_support():
    f = torch.zeros
    m = exa.BodyKeypoints(**hand_written())
    x, j, rot = f(2, 5, 3), f(2, 2, 3), f(2, 2, 3, 3)
    with pytest.raises(ValueError, match='BodyKeypoints: vertices must be on a ROCm device'):
        m(x, j, rot=rot)
    with pytest.raises(ValueError, match=r'BodyKeypoints: rot is required with dynamic landmarks \(Ld = 1\)'):
        m(x, j)
    with pytest.raises(ValueError, match=r'BodyKeypoints: vertices must be \[B, V, 3\] with V = 5'):
        m(f(2, 6, 3), j, rot=rot)
    with pytest.raises(ValueError, match=r'BodyKeypoints: joints must be \[2, 2, 3\]'):
        m(x, f(1, 2, 3), rot=rot)
    with pytest.raises(ValueError, match=r'BodyKeypoints: rot must be \[2, 2, 3, 3\]'):
        m(x, j, rot=f(2, 2, 9))
    with pytest.raises(ValueError, match=r'BodyKeypoints: trans must be \[2, 3\]'):
        m(x, j, rot=rot, trans=f(2, 1, 3))
    with pytest.raises(ValueError, match='BodyKeypoints: focal and princpt come together'):
        m(x, j, rot=rot, focal=f(2, 2))
    with pytest.raises(ValueError, match=r'BodyKeypoints: princpt must be \[2, 2\]'):
        m(x, j, rot=rot, focal=f(2, 2), princpt=f(2, 3))
    with pytest.raises(ValueError, match='BodyKeypoints: focal is camera data in the reference and gets no gradient'):
        m(x, j, rot=rot, focal=f(2, 2, requires_grad=True), princpt=f(2, 2))
    with pytest.raises(ValueError, match='BodyKeypoints: vertices must be float32'):
        m(x.double(), j, rot=rot)
    with pytest.raises(TypeError, match='BodyKeypoints: joints must be a tensor'):
        m(x, None, rot=rot)

    loss = exa.CoordLoss([3, 4], [5, 6], 1, 2)
    p, v, cam = f(2, 8, 2), f(2, 8, 1), f(2, 8, 3)
    with pytest.raises(ValueError, match='CoordLoss: kpt_proj must be on a ROCm device'):
        loss(p, p, v, cam)
    with pytest.raises(ValueError, match=r'CoordLoss: kpt_proj must be \[B, K, 2\]'):
        loss(f(2, 8, 3), p, v, cam)
    with pytest.raises(ValueError, match=r'CoordLoss: kpt_proj_gt must be \[2, 8, 2\], the shape of kpt_proj'):
        loss(p, f(2, 7, 2), v, cam)
    with pytest.raises(ValueError, match=r'CoordLoss: kpt_valid must be \[2, 8, 1\] or \[2, 8\]'):
        loss(p, p, f(2, 8, 2), cam)
    with pytest.raises(ValueError, match=r'CoordLoss: kpt_cam must be \[2, 8, 3\]'):
        loss(p, p, v, f(2, 8, 2))
    with pytest.raises(ValueError, match=r'CoordLoss: weight must be \[2, 8, 2\], the shape of kpt_proj'):
        loss(p, p, v, cam, weight=f(2, 8, 1))
    with pytest.raises(ValueError, match='CoordLoss: kpt_valid is data in the reference and gets no gradient'):
        loss(p, p, f(2, 8, 1, requires_grad=True), cam)
    with pytest.raises(ValueError, match='CoordLoss: weight is data in the reference'):
        loss(p, p, v, cam, weight=f(2, 8, 2, requires_grad=True))
    with pytest.raises(ValueError, match='CoordLoss: kpt_proj_gt must be float32'):
        loss(p, p.double(), v, cam)
    with pytest.raises(ValueError, match=r'CoordLoss: rhand_idx holds 6, outside \[0, 6\) \(the keypoints\)'):
        loss._device_tables(6, torch.device('cpu'))
    with pytest.raises(ValueError, match='CoordLoss: lhand_idx is empty'):
        exa.CoordLoss([], [5], 1, 2)
    with pytest.raises(ValueError, match=r'CoordLoss: lhand_idx holds -2, outside \[0, K\)'):
        exa.CoordLoss([-2], [5], 1, 2)
    with pytest.raises(ValueError, match='CoordLoss: lwrist_idx must be an integer >= 0'):
        exa.CoordLoss([1], [5], -1, 2)
    lhand, rhand, part = loss._device_tables(8, torch.device('cpu'))
    assert part.tolist() == [0, 1, 2, 1, 1, 2, 2, 0] and lhand.dtype == part.dtype == torch.int32
    assert loss._device_tables(8, torch.device('cpu'))[2] is part, 'built once per K and device'


def test_the_c_entry_points_check_sizes_before_any_launch():
    lib = _lib.load()
    z = ctypes.c_void_p(0)
    t = _lib.ExaMeshKeypoints(5, 2, 3, 1, 2, 0)
    fwd = lambda B, tab=t: lib.exa_mesh_keypoints_forward(ctypes.byref(tab), B, z, z, z, z, z, z, 0, z, z, z, z, z, z)      # noqa: E731
    assert lib.exa_mesh_keypoints_forward(None, 1, z, z, z, z, z, z, 0, z, z, z, z, z, z) == -2
    assert lib.exa_mesh_last_error() == b'exa_mesh: tables is NULL'
    assert fwd(-1) == -1 and lib.exa_mesh_last_error() == b'exa_mesh: negative size'
    assert fwd(65536) == -1 and lib.exa_mesh_last_error() == b'exa_mesh: B exceeds 65535'
    assert fwd(1) == -2 and lib.exa_mesh_last_error() == b'exa_mesh: rec / rec_w is NULL'
    assert fwd(1, _lib.ExaMeshKeypoints(5, 2, 3, 1, 2, 6)) == -1 and lib.exa_mesh_last_error() == b'exa_mesh: T exceeds V'
    assert fwd(1, _lib.ExaMeshKeypoints(1 << 20, 2, 3, 1, 2, 0)) == -2          # sizes pass, then the NULL tables
    assert fwd(4096, _lib.ExaMeshKeypoints(1 << 20, 2, 3, 1, 2, 0)) == -1
    assert lib.exa_mesh_last_error() == b'exa_mesh: B * V * 3 exceeds 2^30'
    assert lib.exa_mesh_keypoints_backward(ctypes.byref(t), -1, z, z, z, z, z, 0, z, z, z, z, z, z, 0, z, z, z, z) == -1
    assert lib.exa_mesh_keypoints_workspace_size(1, 1, 1, None) == -2
    assert lib.exa_mesh_keypoints_workspace_size(-1, 1, 1, ctypes.byref(ctypes.c_uint64())) == -1
    assert lib.exa_mesh_coord_loss_forward(-1, 5, 1, 1, z, z, z, z, z, z, z, z, z, z, z) == -1
    assert lib.exa_mesh_coord_loss_forward(1, 5, 0, 1, z, z, z, z, z, z, z, z, z, z, z) == -1
    assert lib.exa_mesh_last_error() == b'exa_mesh: a hand needs at least one keypoint'
    assert lib.exa_mesh_coord_loss_forward(0, 5, 1, 1, z, z, z, z, z, z, z, z, z, z, z) == 0          # B == 0: a no-op
    assert lib.exa_mesh_coord_loss_forward(1, 5, 1, 1, z, z, z, z, z, z, z, z, z, z, z) == -2
    assert lib.exa_mesh_coord_loss_backward(1, 0, z, z, z, z, z, z, z, z) == 0
    assert lib.exa_mesh_coord_loss_backward(1, 5, z, z, z, z, z, z, z, z) == -2
    assert lib.exa_mesh_coord_loss_backward(1 << 20, 1 << 10, z, z, z, z, z, z, z, z) == -1
