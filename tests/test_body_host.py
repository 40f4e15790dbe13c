"""CPU tests of the template stage's host side (include/exa_mesh.h exa_mesh_upsample_* / exa_mesh_body_*,
exavatar_release_amd/body.py): every invalid argument fails with its status and message before any GPU work, the new
names are exported and built without contraction, and what the reference holds as data is refused a gradient."""
import ctypes

import numpy as np
import pytest
import torch

import body_oracle as bo
import exavatar_release_amd as exa
from exavatar_release_amd import _lib, build

INVALID, NULLPTR = -1, -2
FAKE = 0x1000            # a non-NULL device address no call below gets as far as using
IP = ctypes.POINTER(ctypes.c_int32)


def _fails(rc, status, word):
    msg = _lib.load().exa_mesh_last_error().decode()
    assert rc == status, (rc, msg)
    assert msg.startswith('exa_mesh: ') and word in msg, msg
    with pytest.raises(RuntimeError, match='exa_mesh: '):
        _lib.MESH.check(rc)


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(IP)


def _plan(V0, faces, levels, counts=True, arrays=None):
    keep, f = _i32(faces)
    c = np.zeros(3, np.int32)
    arrays = arrays or [None] * 6
    return _lib.load().exa_mesh_upsample_plan(V0, len(faces), f if len(faces) else None, levels,
                                              c.ctypes.data_as(IP) if counts else None, *arrays), c


def test_exports_and_build_flags():
    for name in ('BodyTemplate', 'BodyOutput', 'MeshUpsampler'):
        assert name in exa.__all__ and hasattr(exa, name)
    assert build.SOURCES['body.hip'] == ['-ffp-contract=off']
    assert _lib.load().exa_mesh_version() == 100 == _lib.MESH.version
    assert exa.BodyOutput._fields == bo.OUTPUTS


def test_plan_validation():
    tri = [[0, 1, 2]]
    rc, c = _plan(3, tri, 2)
    assert rc == 0 and c.tolist() == [6, 15, 16]
    rc, c = _plan(3, tri, 1)
    assert rc == 0 and c.tolist() == [6, 6, 4]
    for levels in (0, 3):
        _fails(_plan(3, tri, levels)[0], INVALID, 'levels (subdivide_num) must be 1 or 2')
    _fails(_plan(3, [[0, 1, 3]], 2)[0], INVALID, 'faces[0][2] = 3 lies outside [0, 3)')
    _fails(_plan(3, [[0, 1, 2], [-1, 1, 2]], 1)[0], INVALID, 'faces[1][0] = -1 lies outside')
    _fails(_plan(-1, tri, 1)[0], INVALID, 'negative size')
    _fails(_plan(3, tri, 2, counts=False)[0], NULLPTR, 'counts is NULL')
    _fails(_lib.load().exa_mesh_upsample_plan(3, 1, None, 1, np.zeros(3, np.int32).ctypes.data_as(IP), *[None] * 6),
           NULLPTR, 'faces is NULL')
    keep, p = _i32(np.zeros(64))
    _fails(_plan(3, tri, 2, arrays=[p, None, None, None, None, None])[0], NULLPTR, 'all given or all NULL')
    _fails(_plan(3, tri, 2, arrays=[p, p, p, p, None, None])[0], NULLPTR, 'all given or all NULL')
    _fails(_plan(1 << 26, tri, 1)[0], INVALID, 'exceed 2^26')


def _up(levels=2, V0=3, V1=6, Vn=15, par=FAKE, off1=FAKE, dep1=FAKE, off2=FAKE, dep2=FAKE):
    return _lib.ExaMeshUpsample(levels, V0, V1, Vn, par, off1, dep1, off2, dep2)


def test_upsample_call_validation():
    lib = _lib.load()
    fwd = lambda up, C=3, x=FAKE, out=FAKE: lib.exa_mesh_upsample_forward(      # noqa: E731
        None if up is None else ctypes.byref(up), C, x, out, None)
    bwd = lambda up, C=3, g=FAKE, ws=FAKE, nbytes=1 << 20, dx=FAKE: lib.exa_mesh_upsample_backward(      # noqa: E731
        None if up is None else ctypes.byref(up), C, g, None, ws, nbytes, dx, None)
    for call in (fwd, bwd):
        _fails(call(None), NULLPTR, 'up (the upsampling plan) is NULL')
        for levels in (0, 3):
            _fails(call(_up(levels=levels)), INVALID, 'levels (subdivide_num) must be 1 or 2')
        for C in (0, 9):
            _fails(call(_up(), C=C), INVALID, 'C (channels) must be 1 .. 8')
        _fails(call(_up(V1=2)), INVALID, 'need 0 <= V0 <= V1 <= Vn')
        _fails(call(_up(levels=1)), INVALID, 'Vn must equal V1 with one round')
        _fails(call(_up(V1=1 << 26, Vn=(1 << 26) + 1)), INVALID, 'exceeds 2^26')
        _fails(call(_up(par=None)), NULLPTR, 'par is NULL')
    _fails(fwd(_up(), x=None), NULLPTR, 'x / out is NULL')
    _fails(fwd(_up(), out=None), NULLPTR, 'x / out is NULL')
    _fails(bwd(_up(), g=None), NULLPTR, 'g / dx is NULL')
    _fails(bwd(_up(off1=None)), NULLPTR, 'off1 / dep1 is NULL')
    _fails(bwd(_up(dep2=None)), NULLPTR, 'off2 / dep2 is NULL')
    _fails(bwd(_up(), ws=None), NULLPTR, 'ws (workspace) is NULL')
    _fails(bwd(_up(), nbytes=4 * 6 * 3 - 1), INVALID, 'workspace is smaller than 4 V1 C bytes')
    assert fwd(_up(V0=0, V1=0, Vn=0, par=None)) == 0 and bwd(_up(V0=0, V1=0, Vn=0, par=None)) == 0      # empty: no-ops


class _Body:
    """A descriptor with plausible sizes and fake addresses, one field changed at a time."""

    def __init__(self, **change):
        self.parents = (ctypes.c_int32 * 64)(-1, *range(63))
        self.up = _up(V0=change.pop('up_V0', 10), V1=20, Vn=40)
        f = dict(V=10, L=5, J=4, nnz=12, root=0, parents=ctypes.cast(self.parents, IP), up=ctypes.pointer(self.up))
        f.update({k: FAKE for k, _ in _lib.ExaMeshBody._fields_ if k not in f})
        f.update(change)
        self.d = _lib.ExaMeshBody(**f)

    def sizes(self, out=True):
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        rc = _lib.load().exa_mesh_body_workspace_sizes(ctypes.byref(self.d), ctypes.byref(a) if out else None,
                                                       ctypes.byref(b))
        return rc, a.value, b.value

    def forward(self, coef=FAKE, ws=FAKE, nbytes=1 << 30, out=FAKE):
        return _lib.load().exa_mesh_body_forward(ctypes.byref(self.d), coef, FAKE, ws, nbytes, FAKE, FAKE, out, FAKE, FAKE,
                                                 None)

    def backward(self, fws=FAKE, fbytes=1 << 30, jnp=FAKE, bws=FAKE, bbytes=1 << 30, dcoef=FAKE, djo=FAKE):
        return _lib.load().exa_mesh_body_backward(ctypes.byref(self.d), fws, fbytes, jnp, FAKE, FAKE, FAKE, FAKE, FAKE,
                                                  bws, bbytes, dcoef, djo, None)


SHAPES = [(dict(J=65), 'J (joints) must be 1 .. 64'), (dict(J=0), 'J (joints) must be 1 .. 64'),
          (dict(L=0), 'L (coefficients) must be 1 .. 512'), (dict(L=513), 'L (coefficients) must be 1 .. 512'),
          (dict(V=0), 'V (vertices) must be 1 .. 2^24'), (dict(V=(1 << 24) + 1), 'V (vertices) must be 1 .. 2^24'),
          (dict(nnz=-1), 'nnz (regressor non-zeros) must be 0 .. J V'), (dict(nnz=41), 'nnz (regressor non-zeros)'),
          (dict(root=4), 'root must lie in [0, J)'), (dict(root=-1), 'root must lie in [0, J)'),
          (dict(up_V0=9), "the upsampling plan's V0 is not V")]


@pytest.mark.parametrize('change, word', SHAPES, ids=[w[:12] + str(sorted(c.items())) for c, w in SHAPES])
def test_body_shape_validation_in_every_entry_point(change, word):
    b = _Body(**change)
    for rc in (b.sizes()[0], b.forward(), b.backward()):
        _fails(rc, INVALID, word)


def test_body_call_validation():
    lib = _lib.load()
    rc, fwd_bytes, bwd_bytes = _Body().sizes()
    assert rc == 0 and fwd_bytes % 256 == 0 and bwd_bytes % 256 == 0
    assert fwd_bytes >= 4 * (2 * 30 + 4 * (3 + 16 + 9 + 16 + 3 + 3) + 3) and bwd_bytes >= 4 * (3 * 30 + 20 * 3 + 5)
    _fails(lib.exa_mesh_body_workspace_sizes(None, None, None), NULLPTR, 'body is NULL')
    _fails(_Body().sizes(out=False)[0], NULLPTR, 'fwd_bytes / bwd_bytes is NULL')
    _fails(_Body(up=None).sizes()[0], NULLPTR, 'up (the upsampling plan) is NULL')
    for call in (_Body(parents=None).forward, _Body(parents=None).backward):
        _fails(call(), NULLPTR, 'parents is NULL')
    bad = _Body()
    bad.parents[0] = 0
    _fails(bad.forward(), INVALID, 'parents[0] must be -1')
    bad.parents[0], bad.parents[2] = -1, 2
    _fails(bad.backward(), INVALID, 'parents[2] = 2 must lie in [0, 2)')
    _fails(_Body().forward(coef=None), NULLPTR, 'coef / joint_offset is NULL')
    for field in ('v_base', 'dirs', 'weights'):
        _fails(_Body(**{field: None}).forward(), NULLPTR, 'v_base / dirs / weights is NULL')
    _fails(_Body(jreg_off=None).forward(), NULLPTR, 'jreg_off / jreg_col / jreg_val is NULL')
    _fails(_Body(jreg_val=None).forward(), NULLPTR, 'jreg_off / jreg_col / jreg_val is NULL')
    _fails(_Body(rot_inverse=None).forward(), NULLPTR, 'rot_pose / rot_inverse / rot_identity is NULL')
    _fails(_Body().forward(out=None), NULLPTR, 'an output is NULL')
    _fails(_Body().forward(ws=None), NULLPTR, 'fwd_ws (workspace) is NULL')
    _fails(_Body().forward(nbytes=fwd_bytes - 1), INVALID, 'fwd_ws is smaller than exa_mesh_body_workspace_sizes')
    assert _Body().backward(dcoef=None, djo=None) == 0                      # nothing wanted: a no-op
    _fails(_Body(jregT_off=None).backward(), NULLPTR, 'jregT_off / jregT_row / jregT_val is NULL')
    _fails(_Body(dirs=None).backward(), NULLPTR, 'dirs / weights is NULL')
    _fails(_Body(rot_pose=None).backward(), NULLPTR, 'rot_pose / rot_inverse / rot_identity is NULL')
    _fails(_Body().backward(jnp=None), NULLPTR, 'joint_neutral_pose is NULL')
    _fails(_Body().backward(fws=None), NULLPTR, 'fwd_ws / bwd_ws (workspace) is NULL')
    _fails(_Body().backward(bws=None), NULLPTR, 'fwd_ws / bwd_ws (workspace) is NULL')
    _fails(_Body().backward(fbytes=fwd_bytes - 1), INVALID, 'fwd_ws is smaller')
    _fails(_Body().backward(bbytes=bwd_bytes - 1), INVALID, 'bwd_ws is smaller')


def _template_args(**change):
    verts, faces = bo.grid(3, 4)
    case, _, _ = bo.random_case(verts, faces, 5, [-1, 0, 1, 1], 2, 1)
    t = torch.from_numpy
    args = dict(v_template=t(case['v_template']), shape_dirs=t(case['shape_dirs']), J_regressor=t(case['J_regressor']),
                lbs_weights=t(case['weights']), parents=case['parents'], upsampler=exa.MeshUpsampler(faces, 2),
                rot_pose=t(case['rot_pose']), rot_inverse=t(case['rot_inverse']), pose_offsets=t(case['pose_offsets']),
                face_offset=t(case['face_offset']))
    args.update(change)
    return args


DATA = ('v_template', 'shape_dirs', 'J_regressor', 'lbs_weights', 'rot_pose', 'rot_inverse', 'pose_offsets', 'face_offset')


@pytest.mark.parametrize('name', DATA)
def test_data_that_requires_grad_is_refused(name):
    args = _template_args()
    args[name] = args[name].clone().requires_grad_(True)
    with pytest.raises(ValueError, match='BodyTemplate: %s is data in the reference and gets no gradient' % name):
        exa.BodyTemplate(**args)


def test_python_argument_checks():
    tpl = exa.BodyTemplate(**_template_args())
    assert tpl.state_dict() == {} and (tpl.num_verts, tpl.num_coef, tpl.num_joints, tpl.nnz) == (12, 5, 4, 48)
    assert tpl.upsampler.num_verts == bo.plan(bo.grid(3, 4)[1], 12, 2)['V'][-1]
    with pytest.raises(RuntimeError, match='runs on a ROCm device only'):
        tpl(torch.zeros(5), torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match='runs on a ROCm device only'):
        tpl.upsampler.up(torch.zeros(12, 3))
    with pytest.raises(ValueError, match='subdivide_num must be 1 or 2'):
        exa.MeshUpsampler([[0, 1, 2]], 3)
    with pytest.raises(ValueError, match=r'faces must be \[F, 3\] ints'):
        exa.MeshUpsampler(np.zeros((2, 3)))
    with pytest.raises(RuntimeError, match=r'faces\[0\]\[1\] = 7 lies outside \[0, 3\)'):
        exa.MeshUpsampler([[0, 7, 2]], 2, num_verts=3)
    with pytest.raises(ValueError, match=r'shape_dirs must be \[V, 3, L\]'):
        exa.BodyTemplate(**_template_args(shape_dirs=torch.zeros(12, 3, 513)))
    with pytest.raises(ValueError, match='1 <= J <= 64'):
        exa.BodyTemplate(**_template_args(J_regressor=torch.zeros(65, 12)))
    with pytest.raises(ValueError, match='parents names 3 joints'):
        exa.BodyTemplate(**_template_args(parents=[-1, 0, 1]))
    with pytest.raises(ValueError, match='root_joint_idx must lie in'):
        exa.BodyTemplate(**_template_args(root_joint_idx=4))
    with pytest.raises(ValueError, match='the upsampler is planned for 3 vertices'):
        exa.BodyTemplate(**_template_args(upsampler=exa.MeshUpsampler([[0, 1, 2]], 2)))
    with pytest.raises(TypeError, match='upsampler must be a MeshUpsampler'):
        exa.BodyTemplate(**_template_args(upsampler=None))
    with pytest.raises(ValueError, match='must be float32'):
        exa.BodyTemplate(**_template_args(v_template=torch.zeros(12, 3, dtype=torch.float64)))
