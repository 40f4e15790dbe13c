"""CPU tests of the posed SMPL-X stage's host side (include/exa_mesh.h exa_mesh_posed_*,
exavatar_release_amd/posed_body.py): the names are exported and bound and the versions unchanged, every invalid argument
of the C calls fails with its status and message before any GPU work, what the reference holds as data is refused a
gradient, ``from_layer`` reads a layer's attributes, and the module keeps nothing in its ``state_dict``."""
import ctypes
import types

import numpy as np
import pytest
import torch

import body_oracle as bo
import posed_oracle as po
import exavatar_release_amd as exa
from exavatar_release_amd import _lib, build, posed_body

INVALID, NULLPTR = -1, -2
FAKE = 0x1000            # a non-NULL device address no call below gets as far as using
IP = ctypes.POINTER(ctypes.c_int32)


def _fails(rc, status, word):
    msg = _lib.load().exa_mesh_last_error().decode()
    assert rc == status, (rc, msg)
    assert msg.startswith('exa_mesh: ') and word in msg, msg
    with pytest.raises(RuntimeError, match='exa_mesh: '):
        _lib.MESH.check(rc)


def test_exports_bindings_and_versions():
    for name in ('PosedBody', 'PosedBodyOutput'):
        assert name in exa.__all__ and getattr(exa, name) is getattr(posed_body, name)
    assert build.SOURCES['posed_body.hip'] == ['-ffp-contract=off']
    lib = _lib.load()
    assert lib.exa_mesh_version() == 100 == _lib.MESH.version and lib.exa_raster_version() == 139 == _lib.RASTER.version
    for name in ('exa_mesh_posed_workspace_sizes', 'exa_mesh_posed_forward', 'exa_mesh_posed_backward'):
        assert name in _lib.MESH.signatures and hasattr(lib, name)
    assert _lib.MESH.structs['ExaMeshPosed'] is _lib.ExaMeshPosed
    assert exa.PosedBodyOutput._fields == po.OUTPUTS + ('rot',)
    assert 'get_smplx_outputs' in exa.body.__doc__ and 'PosedBody' in exa.body.__doc__ and 'PosedBody' in exa.__doc__


class _Posed:
    """A descriptor with plausible sizes and fake addresses, one field changed at a time."""

    def __init__(self, **change):
        self.parents = (ctypes.c_int32 * 64)(-1, *range(63))
        f = dict(V=10, L=5, J=4, nnz=12, parents=ctypes.cast(self.parents, IP))
        f.update({k: FAKE for k, _ in _lib.ExaMeshPosed._fields_ if k not in f})
        f.update(change)
        self.d = _lib.ExaMeshPosed(**f)

    def sizes(self, out=True):
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        rc = _lib.load().exa_mesh_posed_workspace_sizes(ctypes.byref(self.d), ctypes.byref(a) if out else None,
                                                        ctypes.byref(b))
        return rc, a.value, b.value

    def forward(self, Lb=3, pose=FAKE, betas=FAKE, expression=FAKE, transl=FAKE, Rinv=FAKE, t=FAKE, ws=FAKE,
                nbytes=1 << 30, vertices=FAKE, world=FAKE, rot=FAKE):
        return _lib.load().exa_mesh_posed_forward(ctypes.byref(self.d), Lb, pose, betas, expression, transl, FAKE, Rinv, t,
                                                  ws, nbytes, vertices, FAKE, world, rot, None)

    def backward(self, Lb=3, pose=FAKE, Rinv=FAKE, fws=FAKE, fbytes=1 << 30, g_world=FAKE, bws=FAKE, bbytes=1 << 30,
                 dpose=FAKE, dbetas=FAKE, dexpr=FAKE, dtransl=FAKE, djo=FAKE):
        return _lib.load().exa_mesh_posed_backward(ctypes.byref(self.d), Lb, pose, Rinv, fws, fbytes, FAKE, FAKE, g_world,
                                                   bws, bbytes, dpose, dbetas, dexpr, dtransl, djo, None)


SHAPES = [(dict(J=65), 'J (joints) must be 1 .. 64'), (dict(J=0), 'J (joints) must be 1 .. 64'),
          (dict(L=0), 'L (coefficients) must be 1 .. 512'), (dict(L=513), 'L (coefficients) must be 1 .. 512'),
          (dict(V=0), 'V (vertices) must be 1 .. 2^24'), (dict(V=-3), 'V (vertices) must be 1 .. 2^24'),
          (dict(V=(1 << 24) + 1), 'V (vertices) must be 1 .. 2^24'),
          (dict(nnz=-1), 'nnz (regressor non-zeros) must be 0 .. J V'), (dict(nnz=41), 'nnz (regressor non-zeros)')]


@pytest.mark.parametrize('change, word', SHAPES, ids=[w[:12] + str(sorted(c.items())) for c, w in SHAPES])
def test_shape_validation_in_every_entry_point(change, word):
    b = _Posed(**change)
    for rc in (b.sizes()[0], b.forward(), b.backward()):
        _fails(rc, INVALID, word)


def test_call_validation():
    lib = _lib.load()
    rc, fwd_bytes, bwd_bytes = _Posed().sizes()
    assert rc == 0 and fwd_bytes % 256 == 0 and bwd_bytes % 256 == 0
    # what the sections hold at V = 10, J = 4, L = 5 (P = 27), each rounded up to 256 bytes
    assert fwd_bytes >= 4 * (2 * 4 + 9 * 4 + 27 + 2 * 30 + 3 * 4 + 16 * 4 + 3 * 4)
    assert bwd_bytes >= 4 * (3 * 30 + 16 * 4 + 3 + 9 * 4 + 3 * 4 + 27 + 27) + _lib.skin_workspace_size(10, 4)
    _fails(lib.exa_mesh_posed_workspace_sizes(None, None, None), NULLPTR, 'posed (the descriptor) is NULL')
    _fails(_Posed().sizes(out=False)[0], NULLPTR, 'fwd_bytes / bwd_bytes is NULL')
    for call in (_Posed().forward, _Posed().backward):
        for Lb in (-1, 6):
            _fails(call(Lb=Lb), INVALID, 'Lb (betas) must be 0 .. L')
    for call in (_Posed(parents=None).forward, _Posed(parents=None).backward):
        _fails(call(), NULLPTR, 'parents is NULL')
    bad = _Posed()
    bad.parents[0] = 0
    _fails(bad.forward(), INVALID, 'parents[0] must be -1')
    bad.parents[0], bad.parents[2] = -1, 2
    _fails(bad.backward(), INVALID, 'parents[2] = 2 must lie in [0, 2)')
    for field in ('v_base', 'dirs', 'weights'):
        for call in (_Posed(**{field: None}).forward, _Posed(**{field: None}).backward):
            _fails(call(), NULLPTR, 'v_base / dirs / weights is NULL')
    _fails(_Posed(posedirs=None).forward(), NULLPTR, 'posedirs is NULL')
    assert _Posed(J=1, nnz=3, posedirs=None).backward(dpose=None, dbetas=None, dexpr=None, dtransl=None, djo=None) == 0
    _fails(_Posed(jreg_off=None).forward(), NULLPTR, 'jreg_off / jreg_col / jreg_val is NULL')
    _fails(_Posed(jreg_val=None).forward(), NULLPTR, 'jreg_off / jreg_col / jreg_val is NULL')
    _fails(_Posed().forward(pose=None), NULLPTR, 'pose / transl is NULL')
    _fails(_Posed().forward(transl=None), NULLPTR, 'pose / transl is NULL')
    _fails(_Posed().forward(betas=None), NULLPTR, 'betas / expression is NULL')
    _fails(_Posed().forward(expression=None), NULLPTR, 'betas / expression is NULL')
    _fails(_Posed().forward(Rinv=None), INVALID, 'Rinv and t must be given together')
    _fails(_Posed().forward(world=None), INVALID, 'vertices_world needs Rinv and t')
    _fails(_Posed().forward(Rinv=None, t=None), INVALID, 'vertices_world needs Rinv and t')
    _fails(_Posed().forward(vertices=None), NULLPTR, 'vertices / joints / rot is NULL')
    _fails(_Posed().forward(rot=None), NULLPTR, 'vertices / joints / rot is NULL')
    _fails(_Posed().forward(ws=None), NULLPTR, 'fwd_ws (workspace) is NULL')
    _fails(_Posed().forward(nbytes=fwd_bytes - 1), INVALID, 'fwd_ws is smaller than exa_mesh_posed_workspace_sizes')
    assert _Posed().backward(dpose=None, dbetas=None, dexpr=None, dtransl=None, djo=None) == 0      # nothing wanted
    assert _Posed().backward(Lb=5, dpose=None, dbetas=None, dtransl=None, djo=None) == 0            # an empty expression
    _fails(_Posed(jregT_off=None).backward(), NULLPTR, 'jregT_off / jregT_row / jregT_val is NULL')
    _fails(_Posed().backward(pose=None), NULLPTR, 'pose is NULL')
    _fails(_Posed().backward(Rinv=None), NULLPTR, 'g_vertices_world needs Rinv')
    _fails(_Posed().backward(fws=None), NULLPTR, 'fwd_ws / bwd_ws (workspace) is NULL')
    _fails(_Posed().backward(bws=None), NULLPTR, 'fwd_ws / bwd_ws (workspace) is NULL')
    _fails(_Posed().backward(fbytes=fwd_bytes - 1), INVALID, 'fwd_ws is smaller')
    _fails(_Posed().backward(bbytes=bwd_bytes - 1), INVALID, 'bwd_ws is smaller')


def _args(**change):
    verts, faces = bo.grid(3, 4)
    case = po.random_case(verts, faces, 5, [-1, 0, 1, 1], 1)
    t = torch.from_numpy
    args = dict(v_template=t(case['v_template']), shape_dirs=t(case['shape_dirs']), posedirs=t(case['posedirs']),
                J_regressor=t(case['J_regressor']), lbs_weights=t(case['weights']), parents=case['parents'],
                pose_mean=t(case['pose_mean']), face_offset=t(case['face_offset']))
    args.update(change)
    return args


DATA = ('v_template', 'shape_dirs', 'posedirs', 'J_regressor', 'lbs_weights', 'pose_mean', 'face_offset')


@pytest.mark.parametrize('name', DATA)
def test_data_that_requires_grad_is_refused(name):
    args = _args()
    args[name] = args[name].clone().requires_grad_(True)
    with pytest.raises(ValueError, match='PosedBody: %s is data in the reference and gets no gradient' % name):
        exa.PosedBody(**args)


def test_python_argument_checks():
    body = exa.PosedBody(**_args())
    assert body.state_dict() == {} and (body.num_verts, body.num_coef, body.num_joints, body.nnz) == (12, 5, 4, 48)
    assert {n for n, _ in body.named_buffers()} >= {'v_base', 'dirs', 'posedirs', 'pose_mean', 'jreg_off', 'jregT_off',
                                                    'weights'}
    assert exa.PosedBody(**_args(pose_mean=None, face_offset=None)).pose_mean is None
    assert exa.PosedBody(**_args(pose_mean=torch.zeros(12))).pose_mean.shape == (4, 3)      # the layer's flat [3 J]
    with pytest.raises(RuntimeError, match='runs on a ROCm device only'):
        body(torch.zeros(4, 3), torch.zeros(3), torch.zeros(2), torch.zeros(3))
    with pytest.raises(TypeError, match='PosedBody: pose must be a tensor'):
        body(None, torch.zeros(3), torch.zeros(2), torch.zeros(3))
    with pytest.raises(ValueError, match=r'shape_dirs must be \[V, 3, L\]'):
        exa.PosedBody(**_args(shape_dirs=torch.zeros(12, 3, 513)))
    with pytest.raises(ValueError, match=r'shape_dirs must be \[V, 3, L\]'):
        exa.PosedBody(**_args(shape_dirs=torch.zeros(12, 3, 0)))
    with pytest.raises(ValueError, match='1 <= J <= 64'):
        exa.PosedBody(**_args(J_regressor=torch.zeros(65, 12)))
    with pytest.raises(ValueError, match='parents names 3 joints'):
        exa.PosedBody(**_args(parents=[-1, 0, 1]))
    with pytest.raises(ValueError, match=r'posedirs must be \[9 \(J - 1\), 3 V\] = \[27, 36\]'):
        exa.PosedBody(**_args(posedirs=torch.zeros(36, 27)))
    with pytest.raises(ValueError, match=r'lbs_weights must be \[V, J\]'):
        exa.PosedBody(**_args(lbs_weights=torch.zeros(12, 5)))
    with pytest.raises(ValueError, match='pose_mean must hold 3 J = 12 values'):
        exa.PosedBody(**_args(pose_mean=torch.zeros(5, 3)))
    with pytest.raises(ValueError, match=r'face_offset must be \[V, 3\]'):
        exa.PosedBody(**_args(face_offset=torch.zeros(11, 3)))
    with pytest.raises(ValueError, match='must be float32'):
        exa.PosedBody(**_args(v_template=torch.zeros(12, 3, dtype=torch.float64)))
    with pytest.raises(TypeError, match='posedirs must be a tensor'):
        exa.PosedBody(**_args(posedirs=None))


def test_from_layer_reads_the_layers_tables():
    a = _args()
    layer = types.SimpleNamespace(v_template=a['v_template'], shapedirs=a['shape_dirs'][:, :, :3],
                                  expr_dirs=a['shape_dirs'][:, :, 3:], posedirs=a['posedirs'], J_regressor=a['J_regressor'],
                                  lbs_weights=a['lbs_weights'], parents=torch.tensor(a['parents']),
                                  pose_mean=a['pose_mean'].reshape(-1))
    got, want = exa.PosedBody.from_layer(layer, face_offset=a['face_offset']), exa.PosedBody(**a)
    assert got.state_dict() == {}
    names = sorted(n for n, _ in want.named_buffers())
    assert names == sorted(n for n, _ in got.named_buffers())
    for n in names:
        assert torch.equal(getattr(got, n), getattr(want, n)), n
    assert list(got._parents) == list(want._parents) == a['parents']
    assert np.array_equal(want.dirs.numpy(), a['shape_dirs'].numpy().reshape(36, 5).T)
    assert np.array_equal(want.v_base.numpy(), (a['v_template'] + a['face_offset']).numpy())
    # a layer without expression directions or a pose_mean, and a float64 one
    del layer.pose_mean
    layer.expr_dirs = None
    layer.v_template = layer.v_template.double()
    plain = exa.PosedBody.from_layer(layer)
    assert plain.num_coef == 3 and plain.pose_mean is None and plain.v_base.dtype == torch.float32
