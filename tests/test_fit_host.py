"""The host side of the fitting loss's mesh terms (exavatar_release_amd/fit_terms.py, csrc/fit_terms.hip): the plans against
hand-written answers and against the oracle's own transpose, the refusals of the library (status, ``exa_mesh: `` message,
no GPU work: there is no GPU here) and of the Python surface, and the wiring (exports, build flags, buffers)."""
import ctypes
import re

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import _lib, build
from exavatar_release_amd import fit_terms as module
from tests import fit_oracle as fo

NAMES = ('EdgeLengthLoss', 'FaceOffsetSymmetricReg', 'PoseLoss', 'centered_v2v_loss', 'flip_symmetry_plan')


def test_exports_build_flags_and_constants():
    for name in NAMES:
        assert name in exa.__all__ and getattr(exa, name) is getattr(module, name)
    assert build.SOURCES['fit_terms.hip'] == ['-ffp-contract=off']
    header = open(build.os.path.join(build.HERE, '..', 'include', 'exa_mesh.h')).read()
    assert int(re.search(r'#define EXA_MESH_FIT_ROWS (\d+)', header).group(1)) == module.ROWS == fo.BLOCK
    lib = _lib.load()
    assert [lib.exa_mesh_centered_v2v_blocks(v) for v in (-1, 0, 1, 256, 257, 65537)] == [0, 0, 1, 1, 2, 257]


# ---- the plans ----------------------------------------------------------------------------------------------------------
def test_the_face_csr_of_a_hand_written_list():
    """Vertex 4 is in no face (an empty row), face 1 repeats vertex 3 (two slots of one face, ascending corner)."""
    m = exa.EdgeLengthLoss([[0, 1, 2], [3, 3, 1], [2, 1, 0]])
    faces, offsets, entries = m._device_tables(5, torch.device('cpu'))
    assert faces.dtype == offsets.dtype == entries.dtype == torch.int32
    assert faces.tolist() == [[0, 1, 2], [3, 3, 1], [2, 1, 0]]
    assert offsets.tolist() == [0, 2, 5, 7, 9, 9]
    assert entries.tolist() == [0, 8, 1, 5, 7, 2, 6, 3, 4]          # 3 * face + corner
    assert m._device_tables(5, torch.device('cpu'))[1] is offsets, 'built once per vertex count and device'
    off, ent = fo.transpose(np.array([[0, 1, 2], [3, 3, 1], [2, 1, 0]]), 5)
    assert off.tolist() == offsets.tolist() and ent.tolist() == entries.tolist()


def test_the_flip_plan_of_a_hand_written_table():
    """Vertices 1, 3, 4 of 6 carry offsets (rows 0, 1, 2).  Row 0 taps row 1 twice; rows 1 and 2 each have a tap of -1 (vertices
    0 and 2 carry no offset); row 2 taps itself; the rows of closest_faces that belong to no face vertex are not read."""
    closest = [[0, 1, 3], [3, 3, 4], [1, 1, 1], [1, 0, 4], [4, 2, 3], [0, 0, 0]]
    bc = np.arange(18, dtype=np.float32).reshape(6, 3)
    plan = exa.flip_symmetry_plan(6, [1, 3, 4], closest, bc)
    assert plan.vertex_row.tolist() == [-1, 0, -1, 1, 2, -1]
    assert plan.taps.tolist() == [[1, 1, 2], [0, -1, 2], [2, -1, 1]]
    assert plan.weights.tolist() == [[3, 4, 5], [9, 10, 11], [12, 13, 14]]
    assert plan.offsets.tolist() == [0, 1, 4, 7]
    assert plan.entries.tolist() == [3, 0, 1, 8, 2, 5, 6]          # 3 * row + slot, ascending per tapped row
    # a row named by no tap: vertex 5 carries an offset and nobody's closest_faces names it
    plan = exa.flip_symmetry_plan(6, [1, 5], closest, bc)
    assert plan.taps.tolist() == [[-1, -1, -1], [-1, -1, -1]] and plan.offsets.tolist() == [0, 0, 0]
    plan = exa.flip_symmetry_plan(6, [3, 5], closest, bc)
    assert plan.taps.tolist() == [[-1, -1, -1], [-1, -1, -1]]
    plan = exa.flip_symmetry_plan(6, [0, 5, 1], closest, bc)
    assert plan.taps.tolist() == [[0, 2, -1], [0, 0, 0], [-1, -1, -1]] and plan.offsets.tolist() == [0, 4, 4, 5]
    assert plan.entries.tolist() == [0, 3, 4, 5, 1]
    empty = exa.flip_symmetry_plan(6, [], closest, bc)
    assert empty.taps.shape == (0, 3) and empty.offsets.tolist() == [0]


@pytest.mark.parametrize('seed,V_full,Vf', [(1, 60, 25), (2, 300, 257), (3, 10, 10)])
def test_the_flip_plan_equals_the_oracles(seed, V_full, Vf):
    c = fo.sym_case(seed, 1, V_full, Vf, hub=min(Vf - 1, 70))
    plan = exa.flip_symmetry_plan(V_full, c['face_vertex_idx'], c['closest_faces'], c['bc'])
    taps, weights, offsets, entries = fo.flip_plan(V_full, c['face_vertex_idx'], c['closest_faces'], c['bc'])
    assert np.array_equal(plan.taps.numpy(), taps) and np.array_equal(plan.weights.numpy(), weights)
    assert np.array_equal(plan.offsets.numpy(), offsets) and np.array_equal(plan.entries.numpy()[:entries.size], entries)


def test_the_shared_transpose_leaves_the_existing_tables_as_they_were():
    """exa_mesh_neighbor_transpose and exa_mesh_vertex_faces now run through csrc/index_transpose.h: the same arrays as a
    stable argsort gives, and their own messages."""
    lib = _lib.load()
    rs = np.random.RandomState(0)
    idx = rs.randint(0, 40, (40, 7)).astype(np.int32)
    off, ent = np.zeros(41, np.int32), np.zeros(280, np.int32)
    assert lib.exa_mesh_neighbor_transpose(40, 7, idx.ctypes.data, off.ctypes.data, ent.ctypes.data) == 0
    want_off, want_ent = fo.transpose(idx, 40)
    assert np.array_equal(off, want_off) and np.array_equal(ent, want_ent)
    idx[3, 2] = 40
    assert lib.exa_mesh_neighbor_transpose(40, 7, idx.ctypes.data, off.ctypes.data, ent.ctypes.data) < 0
    assert lib.exa_mesh_last_error() == b'exa_mesh: neighbour index 40 of vertex 3, slot 2 is outside [0, 40)'
    faces = fo.random_faces(rs, 30, 50).astype(np.int32)
    off, ent = np.zeros(31, np.int32), np.zeros(150, np.int32)
    assert lib.exa_mesh_vertex_faces(30, 50, faces.ctypes.data, off.ctypes.data, ent.ctypes.data) == 0
    want_off, want_ent = fo.transpose(faces, 30)
    assert np.array_equal(off, want_off) and np.array_equal(ent, want_ent)


# ---- refusals of the library --------------------------------------------------------------------------------------------
def test_out_of_range_and_duplicate_indices_fail_with_their_status_and_message():
    closest = np.zeros((6, 3), dtype=np.int64)
    bc = np.zeros((6, 3), dtype=np.float32)
    with pytest.raises(RuntimeError, match=r'^exa_mesh: face_vertex_idx names vertex 3 twice \(rows 0 and 2\) \(status -1\)$'):
        exa.flip_symmetry_plan(6, [3, 1, 3], closest, bc)
    with pytest.raises(RuntimeError, match=r'^exa_mesh: face_vertex_idx\[1\] = 6 is outside \[0, 6\) \(status -1\)$'):
        exa.flip_symmetry_plan(6, [3, 6], closest, bc)
    with pytest.raises(RuntimeError, match=r'^exa_mesh: face_vertex_idx\[0\] = -1 is outside'):
        exa.flip_symmetry_plan(6, [-1], closest, bc)
    closest[4, 1] = 6
    with pytest.raises(RuntimeError, match=r'^exa_mesh: closest_faces index 6 of vertex 4, slot 1 is outside \[0, 6\) \(status -1\)$'):
        exa.flip_symmetry_plan(6, [3], closest, bc)
    with pytest.raises(RuntimeError, match=r'^exa_mesh: closest_faces index 6'):
        exa.FaceOffsetSymmetricReg(6, [3], closest, bc)
    m = exa.EdgeLengthLoss([[0, 1, 5]])
    with pytest.raises(RuntimeError, match=r'^exa_mesh: face index out of range \(status -1\)$'):
        m._device_tables(5, torch.device('cpu'))
    with pytest.raises(RuntimeError, match=r'^exa_mesh: face index out of range'):
        exa.EdgeLengthLoss([[0, -1, 2]])._device_tables(5, torch.device('cpu'))
    assert _lib.load().exa_mesh_flip_symmetry_plan(-1, 0, None, None, None, None, None, None, None, None) == -1
    assert _lib.load().exa_mesh_last_error() == b'exa_mesh: negative size'
    assert _lib.load().exa_mesh_flip_symmetry_plan(1, 0, None, None, None, None, None, None, None, None) == -2


def test_the_c_entry_points_check_sizes_before_any_launch():
    lib = _lib.load()
    z = ctypes.c_void_p(0)
    assert lib.exa_mesh_edge_length_forward(-1, 1, 1, 3, 1, z, z, z, z, z, z) == -1
    assert lib.exa_mesh_edge_length_forward(2, 3, 1, 3, 1, z, z, z, z, z, z) == -1
    assert b'Bt (coord_gt batch) must be 1 or B' in lib.exa_mesh_last_error()
    assert lib.exa_mesh_edge_length_forward(2, 1, 3, 3, 1, z, z, z, z, z, z) == -1
    assert lib.exa_mesh_edge_length_forward(1, 1, 1, 3, 1, z, z, z, z, z, z) == -2
    assert lib.exa_mesh_edge_length_forward(0, 1, 1, 3, 1, z, z, z, z, z, z) == 0          # B == 0: a no-op
    assert lib.exa_mesh_edge_length_backward(1, 1, 1, 3, 1, z, z, z, z, z, z, z, z, z) == -2
    assert lib.exa_mesh_flip_symmetry_forward(1, 3, z, z, z, z, z) == -2
    assert lib.exa_mesh_flip_symmetry_backward(1 << 20, 1 << 10, z, z, z, z, z, z, z, z) == -1
    assert lib.exa_mesh_pose_loss_forward(-1, z, z, z, z) == -1
    assert lib.exa_mesh_pose_loss_forward(0, z, z, z, z) == 0
    assert lib.exa_mesh_pose_loss_backward(4, z, z, z, z, z) == -2
    assert lib.exa_mesh_centered_v2v_forward(65536, 1, z, z, z, 10.0, z, z, z, z) == -1
    assert lib.exa_mesh_last_error() == b'exa_mesh: B exceeds 65535'
    assert lib.exa_mesh_centered_v2v_forward(2, 5, z, z, z, 10.0, z, z, z, z) == -2
    assert lib.exa_mesh_centered_v2v_backward(2, 0, z, z, z, 10.0, z, z, z, z, z) == 0


# ---- refusals of the Python surface (CPU tensors are refused before anything else could run) ----------------------------
def test_the_python_surface_refuses_what_it_does_not_support():
    f = torch.zeros
    edge = exa.EdgeLengthLoss([[0, 1, 2]])
    with pytest.raises(ValueError, match='EdgeLengthLoss: coord_out must be on a ROCm device'):
        edge(f(1, 3, 3), f(1, 3, 3), f(1, 3, 1))
    with pytest.raises(ValueError, match='EdgeLengthLoss: coord_out must be float32'):
        edge(f(1, 3, 3, dtype=torch.float64), f(1, 3, 3), f(1, 3, 1))
    with pytest.raises(TypeError, match='EdgeLengthLoss: coord_gt must be a tensor'):
        edge(f(1, 3, 3), None, f(1, 3, 1))
    with pytest.raises(ValueError, match=r'EdgeLengthLoss: coord_out must be \[B, V, 3\]'):
        edge(f(3, 3), f(1, 3, 3), f(1, 3, 1))
    with pytest.raises(ValueError, match=r'EdgeLengthLoss: coord_gt must be \[2, 3, 3\] or \[1, 3, 3\]'):
        edge(f(2, 3, 3), f(3, 3, 3), f(1, 3, 1))
    with pytest.raises(ValueError, match=r'EdgeLengthLoss: valid must be \[3\], \[1, 3, 1\] or \[2, 3, 1\]'):
        edge(f(2, 3, 3), f(1, 3, 3), f(3, 1))
    with pytest.raises(ValueError, match='EdgeLengthLoss: coord_gt is data in the reference and gets no gradient'):
        edge(f(1, 3, 3), f(1, 3, 3, requires_grad=True), f(1, 3, 1))
    with pytest.raises(ValueError, match='EdgeLengthLoss: valid is data in the reference'):
        edge(f(1, 3, 3), f(1, 3, 3), f(1, 3, 1, requires_grad=True))
    with pytest.raises(ValueError, match=r'EdgeLengthLoss: face must be \[n, 3\]'):
        exa.EdgeLengthLoss([[0, 1]])
    with pytest.raises(ValueError, match='EdgeLengthLoss: face must hold integers'):
        exa.EdgeLengthLoss(np.zeros((2, 3), np.float32))

    sym = exa.FaceOffsetSymmetricReg(6, [1, 3, 4], np.zeros((6, 3), np.int64), np.zeros((6, 3), np.float32))
    assert sym.state_dict() == {} and {n for n, _ in sym.named_buffers()} == set(sym.PLAN)
    assert sym.taps.dtype == torch.int32 and sym.weights.dtype == torch.float32
    with pytest.raises(ValueError, match='FaceOffsetSymmetricReg: face_offset must be on a ROCm device'):
        sym(f(2, 3, 3))
    with pytest.raises(ValueError, match=r'FaceOffsetSymmetricReg: face_offset must be \[B, Vf, 3\] with Vf = 3'):
        sym(f(2, 4, 3))
    with pytest.raises(ValueError, match='FaceOffsetSymmetricReg: face_offset must be float32'):
        sym(f(2, 3, 3, dtype=torch.float16))
    with pytest.raises(ValueError, match=r'flip_symmetry_plan: closest_faces must be \[6, 3\]'):
        exa.flip_symmetry_plan(6, [1], np.zeros((5, 3), np.int64), np.zeros((6, 3), np.float32))
    with pytest.raises(ValueError, match=r'flip_symmetry_plan: bc must be a floating \[6, 3\] array'):
        exa.flip_symmetry_plan(6, [1], np.zeros((6, 3), np.int64), np.zeros((6, 3), np.int64))
    with pytest.raises(ValueError, match='flip_symmetry_plan: vertex_num must be an integer >= 0'):
        exa.flip_symmetry_plan(-6, [1], np.zeros((6, 3), np.int64), np.zeros((6, 3), np.float32))

    pose = exa.PoseLoss()
    with pytest.raises(ValueError, match='PoseLoss: pose_out must be on a ROCm device'):
        pose(f(2, 9), f(2, 3, 3))
    with pytest.raises(ValueError, match=r'PoseLoss: pose_out must be \[B, 3J\] or \[B, J, 3\]'):
        pose(f(2, 10), f(2, 10))
    with pytest.raises(ValueError, match='PoseLoss: pose_gt must hold the rotations of pose_out'):
        pose(f(2, 9), f(2, 4, 3))
    with pytest.raises(ValueError, match='PoseLoss: pose_gt is data in the reference'):
        pose(f(2, 9), f(2, 9, requires_grad=True))
    with pytest.raises(ValueError, match='PoseLoss: pose_gt must be float32'):
        pose(f(2, 9), f(2, 9, dtype=torch.float64))

    with pytest.raises(ValueError, match='centered_v2v_loss: out must be on a ROCm device'):
        exa.centered_v2v_loss(f(2, 5, 3), f(2, 5, 3), f(1, 5, 1))
    with pytest.raises(ValueError, match=r'centered_v2v_loss: target must be \[2, 5, 3\], the shape of out'):
        exa.centered_v2v_loss(f(2, 5, 3), f(1, 5, 3), f(1, 5, 1))
    with pytest.raises(ValueError, match=r'centered_v2v_loss: weight must be \[V\], \[V, 1\] or \[1, V, 1\] with V = 5'):
        exa.centered_v2v_loss(f(2, 5, 3), f(2, 5, 3), f(2, 5, 1))
    with pytest.raises(ValueError, match='centered_v2v_loss: target is data in the reference'):
        exa.centered_v2v_loss(f(2, 5, 3), f(2, 5, 3, requires_grad=True), f(5))
    with pytest.raises(ValueError, match='centered_v2v_loss: weight is data in the reference'):
        exa.centered_v2v_loss(f(2, 5, 3), f(2, 5, 3), f(5, requires_grad=True))
    with pytest.raises(ValueError, match='centered_v2v_loss: scale must be a Python number'):
        exa.centered_v2v_loss(f(2, 5, 3), f(2, 5, 3), f(5), scale=torch.tensor(10.0))
    with pytest.raises(ValueError, match='centered_v2v_loss: out must be float32'):
        exa.centered_v2v_loss(f(2, 5, 3).double(), f(2, 5, 3), f(5))
