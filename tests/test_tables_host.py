"""The host tables the feature modules share (exavatar_release_amd/_tables.py) and the two shape checks they share
(_device.check_rows, _device.check_shape with shared=True): the stamp, the bounded cache and what it keeps alive, the
checked int32 table and its pointer, the vertex -> (face, corner) CSR behind both of its users, the buffers that follow
their input.  No GPU work: there is no GPU here."""
import ctypes
import gc
import importlib
import weakref

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import _device, _lib, _tables, mesh

FACES = [[0, 1, 2], [3, 3, 1], [2, 1, 0]]          # test_fit_host's list: V = 5, face 1 repeats vertex 3, vertex 4 is in no face
CPU = torch.device('cpu')


# ---- the stamp ------------------------------------------------------------------------------------------------------------
def test_a_stamp_is_equal_only_for_the_same_unwritten_object():
    a, b = torch.arange(6.0), torch.ones(3, dtype=torch.bool)
    first = _tables.stamp(a, b)
    assert _tables.stamp(a, b) == first and len(first) == 2
    assert _tables.stamp(a.clone(), b) != first, 'an equal tensor that is another object'
    assert _tables.stamp(a.view(6), b) != first, 'a view of the same storage is another object'
    assert a.view(6).data_ptr() == a.data_ptr()
    a.add_(1.0)
    assert _tables.stamp(a, b) != first, 'an in-place write'
    second = _tables.stamp(a, b)
    b[1] = False
    assert _tables.stamp(a, b) != second


# ---- the cache ------------------------------------------------------------------------------------------------------------
def test_the_cache_returns_what_it_keeps_and_is_cleared_beyond_16_entries():
    cache = _tables.Cache()
    assert cache.find('a') is None
    value = {'table': 1}
    assert cache.keep('a', value) is value and cache.find('a') is value and cache.find('a') is value
    seen = []
    for k in range(1, 40):
        cache.keep(k, [k])
        seen.append(len(cache))
        assert cache.find(k) == [k]
    assert max(seen) == 17 and all(n <= 17 for n in seen)
    # 'a' + 1 .. 16 are 17 entries: the 18th distinct key finds more than 16 and clears them first
    assert seen[15] == 17 and seen[16] == 1
    fresh = _tables.Cache()
    for k in range(17):
        fresh.keep(k, k)
    assert len(fresh) == 17 and fresh.find(0) == 0
    fresh.keep(17, 17)
    assert len(fresh) == 1 and fresh.find(0) is None and fresh.find(17) == 17


def test_an_entry_keeps_its_key_tensors_alive():
    cache = _tables.Cache()
    t = torch.arange(5)
    ref = weakref.ref(t)
    cache.keep(_tables.stamp(t), 'tables', t)
    del t
    gc.collect()
    assert ref() is not None, 'the entry holds the tensor, so its id stays its own'
    assert cache.find(_tables.stamp(ref())) == 'tables'
    cache.clear()
    gc.collect()
    assert ref() is None


def test_the_five_module_caches_are_instances_of_it():
    from exavatar_release_amd import kinematics, mesh_reg, vertex_regs
    offset_regs = importlib.import_module('exavatar_release_amd.offset_regs')      # the package exports a function of that name
    for cache in (mesh._topologies, mesh_reg._tables, vertex_regs._hand_tables, offset_regs._pair_cache, kinematics._trees):
        assert isinstance(cache, _tables.Cache)
    kinematics._trees.clear()
    for n in range(1, 30):                       # the trees were unbounded; a cleared tree is validated again
        assert list(kinematics._tree('t', [-1] + list(range(n)))) == [-1] + list(range(n))
        assert len(kinematics._trees) <= 17


# ---- the host int32 table -------------------------------------------------------------------------------------------------
def test_the_host_table_refuses_what_is_no_index_table():
    with pytest.raises(ValueError, match=r'^w: face must hold integers \(it is float32\)$'):
        _tables.host_i32('w', 'face', np.zeros((2, 3), np.float32), (None, 3))
    with pytest.raises(ValueError, match=r'^w: face must be \[n, 3\] \(it is \(6,\)\)$'):
        _tables.host_i32('w', 'face', np.zeros(6, np.int64), (None, 3))
    with pytest.raises(ValueError, match=r'^w: face must be \[n, 3\] \(it is \(2, 4\)\)$'):
        _tables.host_i32('w', 'face', np.zeros((2, 4), np.int64), (None, 3))
    with pytest.raises(ValueError, match=r'^w: cf must be \[6, 3\]'):
        _tables.host_i32('w', 'cf', np.zeros((5, 3), np.int64), (6, 3))
    with pytest.raises(ValueError, match=r'^w: face does not fit int32$'):
        _tables.host_i32('w', 'face', np.array([[0, 1, 2 ** 31]], np.int64), (None, 3))
    with pytest.raises(ValueError, match='does not fit int32'):
        _tables.host_i32('w', 'face', [[0, 1, -2 ** 31 - 1]], (None, 3))


@pytest.mark.parametrize('x', [np.zeros((0, 3), np.float64), torch.tensor([[0, 1, 2], [2, 1, 0]], dtype=torch.int64),
                               [[0, 1, 2], [4, 5, 6]], np.array([[7, 8, 255]], np.uint8),
                               np.arange(12, dtype=np.int64).reshape(3, 4)[:, 1:], [[0, 1, 2 ** 31 - 1]]],
                         ids=['empty', 'int64-tensor', 'nested-list', 'uint8', 'strided', 'int32-max'])
def test_the_host_table_accepts_and_gives_contiguous_int32(x):
    a = _tables.host_i32('w', 'face', x, (None, 3))
    assert a.dtype == np.int32 and a.flags['C_CONTIGUOUS'] and a.ndim == 2 and a.shape[1] == 3
    want = x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    assert np.array_equal(a, want.astype(np.int64))


def test_the_pointer_is_null_for_an_empty_array_and_fits_both_bindings():
    empty = _tables.host_i32('w', 'face', np.zeros((0, 3)), (None, 3))
    assert _tables.host_ptr(empty) is None
    with pytest.raises(KeyError):
        _tables.host_ptr(np.zeros(3, dtype=np.float64))      # never typed silently as int32*
    a = np.arange(6, dtype=np.int32)
    p = _tables.host_ptr(a)
    assert ctypes.cast(p, ctypes.c_void_p).value == a.ctypes.data and p[5] == 5
    f = np.arange(3, dtype=np.float32)
    assert ctypes.cast(_tables.host_ptr(f), ctypes.c_void_p).value == f.ctypes.data and _tables.host_ptr(f)[2] == 2.0
    # the two ways _lib.py binds a host array both take it (and NULL)
    lib = _lib.load()
    assert ctypes.POINTER(ctypes.c_int32) in lib.exa_mesh_offset_regs_pair_table.argtypes
    assert ctypes.c_void_p in lib.exa_mesh_vertex_faces.argtypes
    for binding in (ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p):
        binding.from_param(p)
        binding.from_param(_tables.host_ptr(empty))


# ---- the vertex -> (face, corner) CSR ---------------------------------------------------------------------------------------
def test_the_face_csr_is_one_for_both_of_its_users():
    faces = _tables.host_i32('w', 'face', FACES, (None, 3))
    offsets, entries = _tables.vertex_faces(faces, 5)
    assert offsets.dtype == entries.dtype == np.int32
    assert offsets.tolist() == [0, 2, 5, 7, 9, 9] and entries.tolist() == [0, 8, 1, 5, 7, 2, 6, 3, 4]
    edge = exa.EdgeLengthLoss(FACES)._device_tables(5, CPU)
    mesh._topologies.clear()
    face = np.array(FACES, dtype=np.int64)
    topo = mesh._topology(face, 5, CPU)
    assert mesh._topology(face, 5, CPU) is topo
    for got in (edge, topo, _tables.face_tables(faces, 5, CPU)):
        assert [t.dtype for t in got] == [torch.int32] * 3
        assert got[0].tolist() == FACES and got[1].tolist() == offsets.tolist() and got[2].tolist() == entries.tolist()
    # mesh._topology converts whatever it is given, as before: a flat list, floats that hold integers
    assert mesh._topology(np.array(FACES, dtype=np.float64).reshape(-1), 5, CPU)[2].tolist() == entries.tolist()
    none = _tables.vertex_faces(np.zeros((0, 3), np.int32), 4)
    assert none[0].tolist() == [0] * 5 and none[1].tolist() == [0]


@pytest.mark.parametrize('bad', [5, -1])
def test_the_face_csr_refuses_an_index_outside_the_vertices(bad):
    faces = np.array([[0, 1, bad]], dtype=np.int32)
    with pytest.raises(RuntimeError, match=r'^exa_mesh: face index out of range \(status -1\)$'):
        _tables.vertex_faces(faces, 5)
    with pytest.raises(RuntimeError, match=r'^exa_mesh: face index out of range \(status -1\)$'):
        mesh._topology(faces, 5, CPU)


# ---- the buffers of an unmoved module ---------------------------------------------------------------------------------------
def test_follow_moves_every_named_buffer_or_none():
    m = torch.nn.Module()
    m.register_buffer('a', torch.zeros(2), persistent=False)
    m.register_buffer('b', torch.ones(3, dtype=torch.int32), persistent=False)
    a = m.a
    _tables.follow(m, ('a', 'b'), CPU)
    assert m.a is a, 'already there: nothing is touched'
    _tables.follow(m, ('a', 'b'), torch.device('meta'))
    assert m.a.device.type == 'meta' and m.b.device.type == 'meta' and m.b.dtype == torch.int32
    assert {n for n, _ in m.named_buffers()} == {'a', 'b'} and m.state_dict() == {}


# ---- the two shape checks -----------------------------------------------------------------------------------------------------
def test_check_rows_takes_every_listed_shape_and_names_them_as_its_caller_does():
    from exavatar_release_amd import vertex_regs
    V = 4
    w = torch.arange(4.0)
    for shape in ((V,), (V, 1), (1, V, 1)):
        rows = _device.check_rows('f', 'weight', w.reshape(shape), V)
        assert tuple(rows.shape) == (V,) and rows.is_contiguous() and torch.equal(rows, w)
    n = torch.arange(12.0).reshape(V, 3)
    for shape in ((V, 3), (1, V, 3)):
        rows = vertex_regs._normal_rows('f', n.reshape(shape), V)
        assert tuple(rows.shape) == (V, 3) and torch.equal(rows, n)
    assert _device.check_rows('f', 'weight', torch.arange(8.0)[::2], V).is_contiguous()
    with pytest.raises(ValueError, match=r'^f: weight must be \[V\], \[V, 1\] or \[1, V, 1\] with V = 4 \(it is \(2, 4, 1\)\)$'):
        _device.check_rows('f', 'weight', torch.zeros(2, V, 1), V)
    with pytest.raises(ValueError, match=r'^f: weight must be \[V\], \[1, V, 1\] or \[V, 1\] with V = 4 \(it is \(1, 4\)\)$'):
        _device.check_rows('f', 'weight', torch.zeros(1, V), V, ((V,), (1, V, 1), (V, 1)), '[V], [1, V, 1] or [V, 1]')
    with pytest.raises(ValueError, match=r'^f: normal must be \[V, 3\] or \[1, V, 3\] with V = 4 \(it is \(4,\)\)$'):
        vertex_regs._normal_rows('f', w, V)
    with pytest.raises(ValueError, match='^f: weight is data in the reference and gets no gradient; detach it$'):
        _device.check_rows('f', 'weight', torch.zeros(V, requires_grad=True), V)
    with pytest.raises(ValueError, match=r'^f: weight must be float32 \(it is torch.float64\)$'):
        _device.check_rows('f', 'weight', torch.zeros(V, dtype=torch.float64), V)
    with pytest.raises(TypeError, match='^f: weight must be a tensor$'):
        _device.check_rows('f', 'weight', [0.0] * V, V)


def test_check_shape_of_shared_data_takes_the_batch_or_one():
    text = '[2, 5, 3] or [1, 5, 3]'
    _device.check_shape('f', 'gt', torch.zeros(2, 5, 3), (2, 5, 3), text, shared=True)
    _device.check_shape('f', 'gt', torch.zeros(1, 5, 3), (2, 5, 3), text, shared=True)
    _device.check_shape('f', 'gt', torch.zeros(1, 5, 3), torch.zeros(1, 5, 3).shape, text, shared=True)
    _device.check_shape('f', 'gt', torch.zeros(2, 5, 3, requires_grad=True), (2, 5, 3), text, shared=True)      # not its business
    for bad in ((3, 5, 3), (2, 4, 3), (2, 5, 1), (5, 3), (1, 2, 5, 3)):
        with pytest.raises(ValueError, match=r'^f: gt must be \[2, 5, 3\] or \[1, 5, 3\] \(it is \(%s\)\)$'
                           % ', '.join(str(s) for s in bad)):
            _device.check_shape('f', 'gt', torch.zeros(bad), (2, 5, 3), text, shared=True)
    with pytest.raises(TypeError, match='^f: gt must be a tensor$'):
        _device.check_shape('f', 'gt', None, (2, 5, 3), text, shared=True)
    with pytest.raises(ValueError, match='^f: gt must be float32'):
        _device.check_shape('f', 'gt', torch.zeros(2, 5, 3, dtype=torch.float16), (2, 5, 3), text, shared=True)
