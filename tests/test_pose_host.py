"""CPU tests of the pose-parameter stage's host side: the three entry points are exported and bound, the ABI version
stays 100, every invalid argument of the C calls fails with its negative status and its message before any GPU work, the
Python surface refuses what it does not support in the package's order, and ``SMPLXParamDict`` -- constructed, saved and
loaded on the CPU -- has the reference's state-dict keys, initial values and optimizer groups (tests/golden/ref_pose.npz).
The ABI itself (include/exa_mesh.h against its binding) is checked by tests/test_abi.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import _lib, build

pose_params = sys.modules['exavatar_release_amd.pose_params']      # the package's `pose_params` is the function
BAD = 0x1000      # never dereferenced: every call below fails validation, or has nothing to do, first
INVALID, NULLPTR = -1, -2
NAMES = ('root_pose', 'body_pose', 'jaw_pose', 'leye_pose', 'reye_pose', 'lhand_pose', 'rhand_pose', 'expr', 'trans')


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'ref_pose.npz'))


def _raw(golden, dtype=torch.float32):
    return {int(f): {n: torch.from_numpy(golden['raw/%d/%s' % (f, n)]).to(dtype) for n in NAMES} for f in golden['frames']}


def test_the_entry_points_are_exported_and_bound():
    lib = _lib.load()
    for name, n_args in (('exa_mesh_pose_params_forward', 7), ('exa_mesh_pose_params_backward', 7),
                         ('exa_mesh_pose_features', 6)):
        assert name in _lib.MESH.signatures
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args
    assert lib.exa_mesh_version() == 100 and _lib.MESH.version == 100
    assert build.SOURCES['pose_params.hip'] == ['-ffp-contract=off']
    for name in ('SMPLXParamDict', 'pose_params', 'pose_features'):
        assert name in exa.__all__ and getattr(exa, name) is getattr(pose_params, name)
    assert pose_params.MAX_SEGMENTS == 64 and pose_params.PARAM_NAMES == NAMES


def _arr(ctype, values):
    return (ctype * len(values))(*values)


def _fwd(lib, rows, d6='bad', out='bad', packed=BAD, quat=None):
    n = len(rows)
    ptrs = lambda v: None if v is None else _arr(ctypes.c_void_p, [BAD] * n if v == 'bad' else v)      # noqa: E731
    return lib.exa_mesh_pose_params_forward(n, _arr(ctypes.c_int32, rows) if rows is not None else None, ptrs(d6),
                                            ptrs(out), packed, quat, None)


def test_forward_rejects_bad_tables_on_the_host():
    lib = _lib.load()
    err = lib.exa_mesh_last_error
    assert lib.exa_mesh_pose_params_forward(-1, None, None, None, None, None, None) == INVALID
    assert err().startswith(b'exa_mesh: ') and b'n_seg must be 0 .. 64' in err()
    assert _fwd(lib, [1] * 65) == INVALID and b'n_seg must be 0 .. 64' in err()
    assert lib.exa_mesh_pose_params_forward(2, None, None, None, None, None, None) == NULLPTR and b'rows is NULL' in err()
    assert _fwd(lib, [3, -1]) == INVALID and b'negative row count' in err()
    assert _fwd(lib, [1 << 23, 1 << 23, 1]) == INVALID and b'more than 2^24 rows' in err()
    assert _fwd(lib, [2, 3], d6=None) == NULLPTR and b'd6 is NULL' in err()
    assert _fwd(lib, [2, 3], d6=[BAD, None]) == NULLPTR and b'd6 holds a NULL pointer' in err()
    # nothing to do: no segments, no rows, nothing wanted
    assert lib.exa_mesh_pose_params_forward(0, None, None, None, None, None, None) == 0
    assert _fwd(lib, [0, 0, 0]) == 0
    assert _fwd(lib, [0, 0], d6=[None, None]) == 0
    assert _fwd(lib, [2, 3], out=None, packed=None) == 0
    assert _fwd(lib, [2, 3], out=[None, None], packed=None) == 0


def _bwd(lib, rows, d6='bad', g_out='bad', g_packed=BAD, g_d6='bad'):
    n = len(rows)
    ptrs = lambda v: None if v is None else _arr(ctypes.c_void_p, [BAD] * n if v == 'bad' else v)      # noqa: E731
    return lib.exa_mesh_pose_params_backward(n, _arr(ctypes.c_int32, rows), ptrs(d6), ptrs(g_out), g_packed, ptrs(g_d6),
                                             None)


def test_backward_rejects_bad_tables_and_skips_what_is_not_wanted():
    lib = _lib.load()
    err = lib.exa_mesh_last_error
    assert _bwd(lib, [1] * 65) == INVALID and b'n_seg must be 0 .. 64' in err()
    assert _bwd(lib, [3, -1]) == INVALID and b'negative row count' in err()
    assert _bwd(lib, [2, 3], d6=None) == NULLPTR and b'd6 is NULL' in err()
    assert _bwd(lib, [2, 3], d6=[None, BAD]) == NULLPTR and b'd6 holds a NULL pointer' in err()
    assert _bwd(lib, [2, 3], g_d6=None) == 0                       # no gradient wanted: a successful no-op
    assert _bwd(lib, [2, 3], g_d6=[None, None]) == 0
    assert _bwd(lib, [2, 0], g_d6=[None, BAD]) == 0                # the only wanted segment has no rows
    assert _bwd(lib, [2, 3], d6=[None, None], g_d6=[None, None]) == 0
    assert lib.exa_mesh_pose_params_backward(0, None, None, None, None, None, None) == 0


def test_pose_features_rejects_bad_sizes_on_the_host():
    lib = _lib.load()
    err = lib.exa_mesh_last_error
    f = lib.exa_mesh_pose_features
    for J in (0, -3, 65):
        assert f(J, 0, BAD, BAD, BAD, None) == INVALID and b'J (joints) must be 1 .. 64' in err()
    for n_body in (-1, 55, 60):
        assert f(55, n_body, BAD, BAD, BAD, None) == INVALID and b'n_body must be 0 .. J - 1' in err()
    assert f(55, 21, None, BAD, BAD, None) == NULLPTR and b'rot is NULL' in err()
    assert f(1, 0, BAD, BAD, BAD, None) == 0                       # rot[1:] is empty
    assert f(55, 21, BAD, None, None, None) == 0                   # nothing wanted


def test_pose_params_raises_as_specified():
    pp = exa.pose_params
    ok = torch.zeros(4, 6)
    assert pp([]) == ()
    with pytest.raises(RuntimeError, match=r'pose_params runs on a ROCm device only \(no CPU path\)'):
        pp([ok])
    with pytest.raises(TypeError, match=r'pose_params: d6\[1\] must be a tensor'):
        pp([ok, ok.numpy()])
    with pytest.raises(ValueError, match=r'pose_params: d6\[1\] must be float32 \(it is torch.float64\)'):
        pp([ok, ok.double()])
    for shape in ((4, 3), (6, 4), ()):
        with pytest.raises(ValueError, match=r'pose_params: d6\[2\] must be \[\.\.\., 6\]'):
            pp([ok, ok, torch.zeros(shape)])
    # a later tensor's type and dtype before an earlier one's shape, the shape before the device
    with pytest.raises(TypeError, match=r'd6\[2\] must be a tensor'):
        pp([torch.zeros(4, 3), ok, None])
    with pytest.raises(ValueError, match=r'd6\[1\] must be float32'):
        pp([torch.zeros(4, 3), ok.double()])
    with pytest.raises(ValueError, match=r'd6\[0\] must be \[\.\.\., 6\] \(it has \(4, 3\)\)'):
        pp([torch.zeros(4, 3), ok], packed=True)


def test_pose_features_raises_as_specified():
    pf = exa.pose_features
    rot = torch.eye(3).repeat(55, 1, 1)
    with pytest.raises(RuntimeError, match=r'pose_features runs on a ROCm device only \(no CPU path\)'):
        pf(rot, 21)
    with pytest.raises(TypeError, match='pose_features: rot must be a tensor'):
        pf(rot.numpy(), 21)
    with pytest.raises(ValueError, match=r'pose_features: rot must be float32'):
        pf(rot.double(), 21)
    with pytest.raises(ValueError, match='pose_features: rot is detached in the reference and gets no gradient; detach it'):
        pf(rot.clone().requires_grad_(True), 21)
    for bad in (torch.zeros(55, 3), torch.zeros(55, 3, 4), torch.zeros(65, 3, 3), torch.zeros(0, 3, 3)):
        with pytest.raises(ValueError, match=r'pose_features: rot must be \[J, 3, 3\] with 1 <= J <= 64'):
            pf(bad, 0)
    for n_body in (55, 100, -1):
        with pytest.raises(ValueError, match=r'pose_features: n_body = %d asks for more rows than rot\[1:\] has \(54\)'
                                             % n_body):
            pf(rot, n_body)


def test_the_module_has_the_references_keys_values_and_groups(golden):
    m = exa.SMPLXParamDict()
    assert list(m.state_dict()) == []
    m.init(_raw(golden, torch.float64))
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in golden['state_dict_keys']]
    assert isinstance(m.smplx_params, torch.nn.ParameterDict) and isinstance(m.smplx_params['3'], torch.nn.ParameterDict)
    for k, v in sd.items():
        want = golden['init/' + k]
        assert tuple(v.shape) == want.shape and v.dtype == torch.float64
        assert np.abs(v.numpy() - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0), k
    groups = m.get_optimizable_params(float(golden['lr']))
    assert [g['name'] for g in groups] == [str(n) for n in golden['group_names']]
    for g, k in zip(groups, sd):
        f, n = k.split('.')[1:]
        assert g['lr'] == float(golden['lr']) and len(g['params']) == 1 and g['params'][0] is m.smplx_params[f][n]
    torch.optim.Adam(groups)                     # the groups are what an optimizer takes


def test_float32_initial_values_are_the_standins(golden):
    from exavatar_release_amd import p3d_standins as p3d
    raw = _raw(golden)
    m = exa.SMPLXParamDict()
    m.init(raw)
    for f, frame in raw.items():
        for n, x in frame.items():
            p = m.smplx_params[str(f)][n]
            assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.dtype == torch.float32 and p.device.type == 'cpu'
            want = p3d.matrix_to_rotation_6d(p3d.axis_angle_to_matrix(x)) if 'pose' in n else x
            assert torch.equal(p.detach(), want) and p.data_ptr() != x.data_ptr()
    assert tuple(m.smplx_params['3']['body_pose'].shape) == (21, 6) and tuple(m.smplx_params['3']['root_pose'].shape) == (6,)


def test_checkpoints_load_both_ways(golden, tmp_path):
    a = exa.SMPLXParamDict()
    a.init(_raw(golden))
    path = tmp_path / 'smplx_params.pt'
    torch.save(a.state_dict(), path)
    b = exa.SMPLXParamDict()
    b.init({f: {n: torch.zeros_like(x) for n, x in frame.items()} for f, frame in _raw(golden).items()})
    assert not torch.equal(b.smplx_params['17']['body_pose'], a.smplx_params['17']['body_pose'])
    result = b.load_state_dict(torch.load(path))
    assert not result.missing_keys and not result.unexpected_keys
    for k, v in a.state_dict().items():
        assert torch.equal(b.state_dict()[k], v)
    # a state dict written by the reference's class: its keys, its shapes (the fixture holds its values)
    ref = {str(k): torch.from_numpy(golden['init/' + str(k)]).float() for k in golden['state_dict_keys']}
    assert not b.load_state_dict(ref).missing_keys
    assert torch.equal(b.smplx_params['3']['lhand_pose'], ref['smplx_params.3.lhand_pose'])


def test_forward_raises_before_a_launch(golden, monkeypatch):
    calls = []
    monkeypatch.setattr(pose_params, 'launch', lambda *a: calls.append(a))
    m = exa.SMPLXParamDict()
    m.init(_raw(golden))
    with pytest.raises(KeyError, match='SMPLXParamDict.forward: no frame 4 among the 2 initialised'):
        m([3, 4])
    with pytest.raises(KeyError, match='no frame 4'):
        m(torch.tensor([4.0]))
    with pytest.raises(RuntimeError, match=r'SMPLXParamDict.forward runs on a ROCm device only \(no CPU path\)'):
        m([3])
    with pytest.raises(RuntimeError, match=r'runs on a ROCm device only'):
        m(torch.tensor([17, 3]), packed=True)
    with pytest.raises(RuntimeError, match=r'runs on a ROCm device only'):
        exa.pose_params([torch.zeros(2, 6)])
    with pytest.raises(ValueError, match='more rows than'):
        exa.pose_features(torch.zeros(55, 3, 3), 55)
    assert calls == []
