"""HIP SMPL-X template stage: a drop-in for the first two lines of ExAvatar's ``HumanGaussian.forward``.

* ``MeshUpsampler(faces, subdivide_num=2)`` -- reference ``smpl_x.upsample_mesh(vert)`` (``avatar/common/utils/
  smpl_x.py:84-91``): one or two rounds of pytorch3d's ``SubdivideMeshes.subdivide_homogeneous`` as ONE launch over a
  flat plan built once.  ``.faces`` and ``.num_verts`` are what chaining ``p3d_standins.SubdivideMeshes`` gives, so
  ``smpl_x.face_upsampled`` and the low-resolution-first vertex order stay as they are.  ``up(vert)`` is bit-equal to
  the two-pass stand-in.
* ``BodyTemplate(...)`` -- reference ``get_neutral_pose_human(jaw_zero_pose=True, use_id_info=True)`` +
  ``get_zero_pose_human()`` (``avatar/common/nets/module.py:337-387``): two ``smplx_layer`` forwards, a third
  ``batch_rigid_transform`` and two subdivisions, as ONE autograd node with one C call each way.  Both poses are
  constants there, so the rotations, the pose-corrective offsets and the inverse rotations are data, computed once
  (``BodyTemplate.from_layer``); what varies -- and what gets a gradient -- is ``coef`` (``shape_param``) and
  ``joint_offset``.

The kernels are ``csrc/body.hip`` behind ``include/exa_mesh.h`` (``exa_mesh_upsample_*``, ``exa_mesh_body_*``); the chains
and the skinning inside the stage are the library's own ``exa_mesh_kinematics_*`` and ``exa_skin_*``.  ROCm device tensors
only, no CPU path.  The CPU restatement that pins the stage bit for bit is ``tests/body_oracle.py``.

Semantics (the header writes out every order)
---------------------------------------------
``v_shaped = (v_template + face_offset) + sum_l coef[l] shape_dirs[v][c][l]``; ``J = J_regressor v_shaped +
joint_offset`` over the regressor's non-zeros, the row ``root_joint_idx`` of ``joint_offset`` ignored
(``smpl_x.get_joint_offset``); ``v_posed = v_shaped + pose_offsets``; chain A, the kinematics of ``rot_pose`` over ``J``,
gives ``joint_neutral_pose`` and the skinning transforms; ``mesh = skin(v_posed)``; ``mesh_upsampled = up(mesh)``; chain
B, the kinematics of ``rot_inverse`` over ``joint_neutral_pose``, gives ``transform_mat_neutral_pose``; chain C, identity
rotations over ``J``, gives ``joint_zero_pose``.  Every operation is rounded in fp32 without fused multiply-adds, every
sum runs in an order that depends on the sizes and the tables alone, and no kernel uses an atomic: the same inputs give
the same bits, forward and backward.

``get_smplx_outputs`` (``avatar/main/model.py:37-58``), the third ``smplx_layer`` call, whose pose varies per frame, is
``posed_body.PosedBody``.  Not covered: the init-time ``get_neutral_pose_human(jaw_zero_pose=False, use_id_info=False)``, which runs once.  The
``feat_list`` form of ``upsample_mesh`` runs at init only and stays with the stand-in.
"""
import collections
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib, p3d_standins
from ._device import _ptr, _workspace, check_no_grad, check_tensor, grad_in, launch
from ._tables import host_i32, host_ptr
from .kinematics import MAX_JOINTS, _tree

MAX_COEF = 512           # EXA_MESH_BODY_MAX_COEF
MAX_CHANNELS = 8         # EXA_MESH_UP_MAX_CHANNELS

BodyOutput = collections.namedtuple('BodyOutput', ['mesh_upsampled', 'mesh', 'joint_neutral_pose',
                                                   'transform_mat_neutral_pose', 'joint_zero_pose'])

_IP = ctypes.POINTER(ctypes.c_int32)


def upsample_plan(faces, num_verts, subdivide_num):
    """The flat plan of ``subdivide_num`` rounds over ``faces`` [F, 3] (a contiguous int32 numpy array) as the library
    builds and validates it on the host: dict(V1, Vn, par, faces, off1, dep1, off2, dep2), numpy int32 arrays."""
    lib = _lib.load()
    F, counts = faces.shape[0], np.zeros(3, dtype=np.int32)
    _lib.MESH.check(lib.exa_mesh_upsample_plan(num_verts, F, host_ptr(faces), subdivide_num, host_ptr(counts),
                                               *(None,) * 6))
    V1, Vn, Fn = (int(c) for c in counts)
    plan = dict(par=np.zeros((Vn - num_verts, 2), np.int32), faces=np.zeros((Fn, 3), np.int32),
                off1=np.zeros(num_verts + 1, np.int32), dep1=np.zeros(2 * (V1 - num_verts), np.int32),
                off2=np.zeros(V1 + 1 if subdivide_num == 2 else 0, np.int32), dep2=np.zeros(2 * (Vn - V1), np.int32))
    _lib.MESH.check(lib.exa_mesh_upsample_plan(num_verts, F, host_ptr(faces), subdivide_num, host_ptr(counts),
                                               *(plan[k].ctypes.data_as(_IP)      # given as a set: an empty one is not NULL
                                                 for k in ('par', 'faces', 'off1', 'dep1', 'off2', 'dep2'))))
    plan.update(V1=V1, Vn=Vn)
    return plan


class _Upsample(torch.autograd.Function):
    """x [V0, C] float32 contiguous -> [Vn, C]."""

    @staticmethod
    def forward(ctx, x, up):
        out = torch.empty((up.num_verts, x.shape[1]), dtype=torch.float32, device=x.device)
        launch(_lib.MESH, 'exa_mesh_upsample_forward', x.device, up._plan(), x.shape[1], _ptr(x), _ptr(out))
        ctx.up = up
        return out

    @staticmethod
    def backward(ctx, g):
        up = ctx.up
        g = grad_in(g)
        C = g.shape[1]
        dx = torch.empty((up.num_coarse, C), dtype=torch.float32, device=g.device)
        nbytes = 4 * up.num_mid * C if up.subdivide_num == 2 else 0
        ws = _workspace(nbytes, g.device) if nbytes else None
        launch(_lib.MESH, 'exa_mesh_upsample_backward', g.device, up._plan(), C, _ptr(g), None, _ptr(ws), nbytes, _ptr(dx))
        return dx, None


class MeshUpsampler(nn.Module):
    """``subdivide_num`` (1 or 2) rounds of ``SubdivideMeshes`` over the topology ``faces`` [F, 3] (a host array, a CPU
    tensor or a device tensor of ints), planned once on the host; every index is checked there.  ``faces`` [4^n F, 3]
    int64 and ``num_verts`` are the chained stand-in's.  The tables are non-persistent buffers: move the module with
    ``.to(device)``; ``state_dict`` is empty."""

    def __init__(self, faces, subdivide_num=2, num_verts=None):
        super(MeshUpsampler, self).__init__()
        what = 'MeshUpsampler'
        device = torch.device('cpu')
        if isinstance(faces, torch.Tensor):
            device, faces = faces.device, faces.detach().cpu().numpy()
        faces = np.asarray(faces)
        if faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype.kind not in 'iu':
            raise ValueError('%s: faces must be [F, 3] ints (it is %s %s)' % (what, faces.dtype, faces.shape))
        if subdivide_num not in (1, 2):
            raise ValueError('%s: subdivide_num must be 1 or 2 (it is %r)' % (what, subdivide_num))
        faces = host_i32(what, 'faces', faces, (None, 3))      # refuses what does not fit int32
        if faces.size and faces.min() < 0:
            raise ValueError('%s: faces holds an index outside [0, 2^31)' % what)
        if num_verts is None:
            num_verts = int(faces.max()) + 1 if faces.size else 0
        plan = upsample_plan(faces, int(num_verts), int(subdivide_num))
        self.subdivide_num = int(subdivide_num)
        self.num_coarse, self.num_mid, self.num_verts = int(num_verts), plan['V1'], plan['Vn']
        self.register_buffer('faces', torch.from_numpy(plan['faces'].astype(np.int64)).to(device), persistent=False)
        for k in ('par', 'off1', 'dep1', 'off2', 'dep2'):
            self.register_buffer('_' + k, torch.from_numpy(plan[k]).to(device), persistent=False)
        self._struct = None

    def _plan(self):
        """The plan as the C ABI takes it (rebuilt when the buffers moved)."""
        key = self._par.data_ptr()
        if self._struct is None or self._struct[0] != key:
            s = _lib.ExaMeshUpsample(self.subdivide_num, self.num_coarse, self.num_mid, self.num_verts,
                                     *(getattr(self, '_' + k).data_ptr() or None for k in ('par', 'off1', 'dep1', 'off2',
                                                                                          'dep2')))
            self._struct = (key, s)
        return ctypes.byref(self._struct[1])

    def up(self, vert):
        """``vert`` [V0, C] (1 <= C <= 8, float32, ROCm) -> [num_verts, C]: ``smpl_x.upsample_mesh(vert)``."""
        what = 'MeshUpsampler.up'
        check_tensor(what, 'vert', vert, rocm=True)
        if vert.dim() != 2 or vert.shape[0] != self.num_coarse or not 1 <= vert.shape[1] <= MAX_CHANNELS:
            raise ValueError('%s: vert must be [V0, C] with V0 = %d and 1 <= C <= %d (it is %s)'
                             % (what, self.num_coarse, MAX_CHANNELS, tuple(vert.shape)))
        if self._par.device != vert.device:
            raise ValueError('%s: the plan is not on the device of vert; move the module with .to()' % what)
        return _Upsample.apply(vert.contiguous(), self)

    forward = up


class _Body(torch.autograd.Function):
    """coef [L], joint_offset [J, 3] (float32, contiguous), the module -> the five outputs."""

    @staticmethod
    def forward(ctx, coef, joint_offset, body):
        dev = coef.device
        V, J, Vn = body.num_verts, body.num_joints, body.upsampler.num_verts
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
        out = BodyOutput(new(Vn, 3), new(V, 3), new(J, 3), new(J, 4, 4), new(J, 3))
        desc, fwd_bytes, _ = body._descriptor()
        ws = _workspace(fwd_bytes, dev)
        launch(_lib.MESH, 'exa_mesh_body_forward', dev, desc, _ptr(coef), _ptr(joint_offset), _ptr(ws), fwd_bytes,
               *(_ptr(t) for t in out))
        ctx.save_for_backward(ws, out.joint_neutral_pose)
        ctx.body = body
        ctx.set_materialize_grads(False)      # a missing cotangent arrives as None and travels as NULL
        return tuple(out)

    @staticmethod
    def backward(ctx, g_up, g_mesh, g_jnp, g_tm, g_jzp):
        want_coef, want_jo = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_coef or want_jo):
            return None, None, None
        ws, jnp = ctx.saved_tensors
        body = ctx.body
        dev = ws.device
        desc, fwd_bytes, bwd_bytes = body._descriptor()
        dcoef = torch.empty(body.num_coef, dtype=torch.float32, device=dev) if want_coef else None
        djo = torch.empty((body.num_joints, 3), dtype=torch.float32, device=dev) if want_jo else None
        bws = _workspace(bwd_bytes, dev)
        grads = [grad_in(g) for g in (g_up, g_mesh, g_jnp, g_tm, g_jzp)]
        launch(_lib.MESH, 'exa_mesh_body_backward', dev, desc, _ptr(ws), fwd_bytes, _ptr(jnp),
               *(_ptr(g) for g in grads), _ptr(bws), bwd_bytes, _ptr(dcoef), _ptr(djo))
        return dcoef, djo, None


def rodrigues(pose):
    """smplx's ``batch_rodrigues`` ([J, 3] axis-angle -> [J, 3, 3]) in the dtype of ``pose``: ``angle = |v + 1e-8|``,
    ``I + sin K + (1 - cos) K^2`` with K the cross-product matrix of ``v / angle``."""
    angle = torch.norm(pose + 1e-8, dim=1, keepdim=True)
    d = pose / angle
    cos, sin = torch.cos(angle)[:, None], torch.sin(angle)[:, None]
    rx, ry, rz = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    zeros = torch.zeros_like(rx)
    K = torch.cat([zeros, -rz, ry, rz, zeros, -rx, -ry, rx, zeros], dim=1).view(-1, 3, 3)
    ident = torch.eye(3, dtype=pose.dtype, device=pose.device)[None]
    return ident + sin * K + (1 - cos) * torch.bmm(K, K)


def pose_constants(pose, posedirs=None):
    """The three pose constants of a fixed axis-angle ``pose`` [J, 3], computed once in float64 on the CPU and rounded to
    float32: ``rot_pose`` (``rodrigues``), ``pose_offsets`` [V, 3] = ``(rot_pose[1:] - I).view(1, -1) @ posedirs`` (None
    without ``posedirs`` [9 (J - 1), 3 V]) and ``rot_inverse`` by the route of ``module.py:363-366``:
    ``axis_angle_to_matrix(matrix_to_axis_angle(inverse(axis_angle_to_matrix(pose))))`` (the stand-ins' pytorch3d)."""
    pose = pose.detach().to('cpu', torch.float64)
    rot = rodrigues(pose)
    offsets = None
    if posedirs is not None:
        feat = (rot[1:] - torch.eye(3, dtype=torch.float64)).reshape(1, -1)
        offsets = torch.matmul(feat, posedirs.detach().to('cpu', torch.float64)).view(-1, 3)
    inv = p3d_standins.matrix_to_axis_angle(torch.inverse(p3d_standins.axis_angle_to_matrix(pose)))
    rot_inverse = p3d_standins.axis_angle_to_matrix(inv)
    f32 = lambda x: None if x is None else x.to(torch.float32)      # noqa: E731
    return f32(rot), f32(offsets), f32(rot_inverse)


_f32 = lambda x: x.detach().to(torch.float32)      # noqa: E731


class _SmplxTables(nn.Module):
    """What ``BodyTemplate`` and ``PosedBody`` (posed_body.py) share: the checks of the data tensors and of the five
    tables' shapes, the re-laid non-persistent buffers, the head of ``from_layer`` and the cache of the C descriptor."""

    def _check_data(self, what, named):
        """``named``: (name, float32 data tensor on ``v_template``'s device, may be None) entries, ``v_template`` first."""
        for name, x, optional in named:
            if x is None and optional:
                continue
            check_tensor(what, name, x)
            check_no_grad(what, name, x)
            if x.device != named[0][1].device:
                raise ValueError('%s: %s is not on the device of v_template' % (what, name))

    def _check_tables(self, what, v_template, shape_dirs, J_regressor, parents, lbs_weights):
        """The shape checks of the five tables, in this order; sets ``_parents`` and the three sizes, returns (V, L, J)."""
        if v_template.dim() != 2 or v_template.shape[1] != 3 or v_template.shape[0] < 1:
            raise ValueError('%s: v_template must be [V, 3] (it is %s)' % (what, tuple(v_template.shape)))
        V = v_template.shape[0]
        if shape_dirs.dim() != 3 or tuple(shape_dirs.shape[:2]) != (V, 3) or not 1 <= shape_dirs.shape[2] <= MAX_COEF:
            raise ValueError('%s: shape_dirs must be [V, 3, L] with V = %d and 1 <= L <= %d (it is %s)'
                             % (what, V, MAX_COEF, tuple(shape_dirs.shape)))
        L = shape_dirs.shape[2]
        if J_regressor.dim() != 2 or J_regressor.shape[1] != V or not 1 <= J_regressor.shape[0] <= MAX_JOINTS:
            raise ValueError('%s: J_regressor must be [J, V] with V = %d and 1 <= J <= %d (it is %s)'
                             % (what, V, MAX_JOINTS, tuple(J_regressor.shape)))
        J = J_regressor.shape[0]
        self._parents = _tree(what, parents)
        if len(self._parents) != J:
            raise ValueError('%s: parents names %d joints, J_regressor %d' % (what, len(self._parents), J))
        if tuple(lbs_weights.shape) != (V, J):
            raise ValueError('%s: lbs_weights must be [V, J] = [%d, %d] (it is %s)' % (what, V, J, tuple(lbs_weights.shape)))
        self.num_verts, self.num_coef, self.num_joints = V, L, J
        return V, L, J

    def _register_tables(self, v_template, face_offset, shape_dirs, own, J_regressor, lbs_weights):
        """The non-persistent buffers, in this order: ``v_base``, ``dirs``, the class's ``own`` (name, tensor or None),
        the regressor's non-zeros as a CSR (``jreg_*``), its transpose's (``jregT_*``) and ``weights``; sets ``nnz``."""
        V, L = self.num_verts, self.num_coef
        i32 = lambda x: x.to(torch.int32).contiguous()      # noqa: E731
        buf = lambda name, x: self.register_buffer(name, x, persistent=False)      # noqa: E731
        buf('v_base', (v_template if face_offset is None else v_template + face_offset).contiguous().clone())
        buf('dirs', shape_dirs.reshape(3 * V, L).t().contiguous())                   # feature-major [L, 3 V]

        def csr(prefix, index, m):
            nz = torch.nonzero(m, as_tuple=False)                                    # ascending (row, column)
            counts = torch.bincount(nz[:, 0], minlength=m.shape[0])
            buf(prefix + '_off', i32(torch.cat((counts.new_zeros(1), torch.cumsum(counts, 0)))))
            buf(prefix + '_' + index, i32(nz[:, 1]))
            buf(prefix + '_val', m[nz[:, 0], nz[:, 1]].contiguous())
            return int(nz.shape[0])

        for name, x in own:
            buf(name, x)
        self.nnz = csr('jreg', 'col', J_regressor)
        csr('jregT', 'row', J_regressor.t())
        buf('weights', lbs_weights.contiguous().clone())
        self._desc = None

    @staticmethod
    def _layer_tables(smplx_layer):
        """(``v_template``, ``cat(shapedirs, expr_dirs)``, ``parents`` as a list) of a smplx layer, float32."""
        dirs = [_f32(smplx_layer.shapedirs)]
        if getattr(smplx_layer, 'expr_dirs', None) is not None:
            dirs.append(_f32(smplx_layer.expr_dirs))
        parents = smplx_layer.parents
        parents = parents.tolist() if isinstance(parents, torch.Tensor) else list(parents)
        return _f32(smplx_layer.v_template), torch.cat(dirs, 2), parents

    def _cached_descriptor(self, key, sizes, make):
        """(the C descriptor, forward workspace bytes, backward workspace bytes), rebuilt when ``key`` (the buffers' data
        pointers) changed: ``make(p)`` builds the struct, ``p(t)`` a buffer's address or None; ``sizes`` names the size query."""
        if self._desc is None or self._desc[0] != key:
            d = make(lambda t: None if t is None else (t.data_ptr() or None))
            fwd, bwd = ctypes.c_uint64(), ctypes.c_uint64()
            _lib.MESH.check(getattr(_lib.load(), sizes)(ctypes.byref(d), ctypes.byref(fwd), ctypes.byref(bwd)))
            self._desc = (key, d, int(fwd.value), int(bwd.value))
        return ctypes.byref(self._desc[1]), self._desc[2], self._desc[3]


class BodyTemplate(_SmplxTables):
    """The shaped SMPL-X template in the big pose and the zero pose (module docstring).

    ``v_template`` [V, 3], ``shape_dirs`` [V, 3, L] (1 <= L <= 512; concatenate ``expr_dirs`` behind ``shapedirs`` if
    expression coefficients are wanted), ``J_regressor`` [J, V], ``lbs_weights`` [V, J] (J <= 64), ``parents`` a sequence
    or CPU tensor of J ints, ``upsampler`` a ``MeshUpsampler`` over the template's faces, ``rot_pose`` and
    ``rot_inverse`` [J, 3, 3], ``pose_offsets`` and ``face_offset`` [V, 3] or None.  All of them are data
    (float32): a tensor that requires a gradient is refused.  The re-laid tables are non-persistent buffers, so
    ``state_dict`` does not change; the sparse ``J_regressor`` is compacted once to its non-zeros."""

    def __init__(self, v_template, shape_dirs, J_regressor, lbs_weights, parents, upsampler, *, rot_pose, rot_inverse,
                 pose_offsets=None, face_offset=None, root_joint_idx=0):
        super(BodyTemplate, self).__init__()
        what = 'BodyTemplate'
        self._check_data(what, (('v_template', v_template, False), ('shape_dirs', shape_dirs, False),
                                ('J_regressor', J_regressor, False), ('lbs_weights', lbs_weights, False),
                                ('rot_pose', rot_pose, False), ('rot_inverse', rot_inverse, False),
                                ('pose_offsets', pose_offsets, True), ('face_offset', face_offset, True)))
        if not isinstance(upsampler, MeshUpsampler):
            raise TypeError('%s: upsampler must be a MeshUpsampler' % what)
        V, _, J = self._check_tables(what, v_template, shape_dirs, J_regressor, parents, lbs_weights)
        for name, x in (('rot_pose', rot_pose), ('rot_inverse', rot_inverse)):
            if tuple(x.shape) != (J, 3, 3):
                raise ValueError('%s: %s must be [J, 3, 3] with J = %d (it is %s)' % (what, name, J, tuple(x.shape)))
        for name, x in (('pose_offsets', pose_offsets), ('face_offset', face_offset)):
            if x is not None and tuple(x.shape) != (V, 3):
                raise ValueError('%s: %s must be [V, 3] with V = %d (it is %s)' % (what, name, V, tuple(x.shape)))
        if not 0 <= int(root_joint_idx) < J:
            raise ValueError('%s: root_joint_idx must lie in [0, %d) (it is %r)' % (what, J, root_joint_idx))
        if upsampler.num_coarse != V:
            raise ValueError('%s: the upsampler is planned for %d vertices, v_template has %d'
                             % (what, upsampler.num_coarse, V))
        self.root_joint_idx = int(root_joint_idx)
        self.upsampler = upsampler
        own = (('pose_offsets', None if pose_offsets is None else pose_offsets.contiguous().clone()),)
        self._register_tables(v_template, face_offset, shape_dirs, own, J_regressor, lbs_weights)
        eye = torch.eye(3, dtype=torch.float32, device=v_template.device)
        for name, x in (('rot_pose', rot_pose.clone()), ('rot_inverse', rot_inverse.clone()), ('rot_identity', eye)):
            self.register_buffer(name, x.expand(J, 3, 3).contiguous(), persistent=False)

    @classmethod
    def from_layer(cls, smplx_layer, faces, pose, *, face_offset=None, subdivide_num=2, root_joint_idx=0):
        """From a (vendored) smplx ``SMPLX`` layer, its faces and the constant axis-angle ``pose`` [J, 3] of the big pose
        (root, body, jaw, eyes, hands in the layer's order; the jaw zero, as ``jaw_zero_pose=True`` has it).  The shape
        directions are ``cat(shapedirs, expr_dirs)``: hand over ``cat(shape_param, zeros)`` as ``coef``, or slice the
        directions yourself and use the constructor.  The three pose constants come from ``pose_constants``."""
        what = 'BodyTemplate.from_layer'
        v_template, shape_dirs, parents = cls._layer_tables(smplx_layer)
        dev = v_template.device
        check_tensor(what, 'pose', pose, f32=False)
        J = smplx_layer.J_regressor.shape[0]
        if tuple(pose.shape) != (J, 3):
            raise ValueError('%s: pose must be [J, 3] with J = %d (it is %s)' % (what, J, tuple(pose.shape)))
        rot_pose, pose_offsets, rot_inverse = pose_constants(pose, smplx_layer.posedirs)
        up = MeshUpsampler(faces, subdivide_num, num_verts=v_template.shape[0]).to(dev)
        return cls(v_template, shape_dirs, _f32(smplx_layer.J_regressor), _f32(smplx_layer.lbs_weights), parents, up,
                   rot_pose=rot_pose.to(dev), rot_inverse=rot_inverse.to(dev), pose_offsets=pose_offsets.to(dev),
                   face_offset=None if face_offset is None else _f32(face_offset).to(dev), root_joint_idx=root_joint_idx)

    def _descriptor(self):
        """(the ``ExaMeshBody`` the C ABI takes, forward workspace bytes, backward workspace bytes); rebuilt when the
        buffers moved."""
        def make(p):
            self.upsampler._plan()      # its struct, which the pointer field below keeps alive
            return _lib.ExaMeshBody(self.num_verts, self.num_coef, self.num_joints, self.nnz, self.root_joint_idx,
                                    ctypes.cast(self._parents, _IP), p(self.v_base), p(self.dirs), p(self.pose_offsets),
                                    p(self.jreg_off), p(self.jreg_col), p(self.jreg_val), p(self.jregT_off),
                                    p(self.jregT_row), p(self.jregT_val), p(self.weights), p(self.rot_pose),
                                    p(self.rot_inverse), p(self.rot_identity),
                                    ctypes.pointer(self.upsampler._struct[1]))

        return self._cached_descriptor((self.v_base.data_ptr(), self.upsampler._par.data_ptr()),
                                       'exa_mesh_body_workspace_sizes', make)

    def forward(self, coef, joint_offset):
        """``coef`` [L] or [1, L] and ``joint_offset`` [J, 3] or [1, J, 3] (float32, ROCm) -> ``BodyOutput``:
        ``mesh_upsampled`` [Vn, 3], ``mesh`` [V, 3], ``joint_neutral_pose`` [J, 3], ``transform_mat_neutral_pose``
        [J, 4, 4] -- the four results of ``get_neutral_pose_human(True, True)`` -- and ``joint_zero_pose`` [J, 3], the
        result of ``get_zero_pose_human()``.  Gradients reach ``coef`` and ``joint_offset``."""
        what = 'BodyTemplate'
        L, J = self.num_coef, self.num_joints
        check_tensor(what, 'coef', coef, rocm=True)
        check_tensor(what, 'joint_offset', joint_offset, rocm=True, on=(coef, 'coef'))
        if tuple(coef.shape) not in ((L,), (1, L)):
            raise ValueError('%s: coef must be [L] or [1, L] with L = %d (it is %s)' % (what, L, tuple(coef.shape)))
        if tuple(joint_offset.shape) not in ((J, 3), (1, J, 3)):
            raise ValueError('%s: joint_offset must be [J, 3] or [1, J, 3] with J = %d (it is %s)'
                             % (what, J, tuple(joint_offset.shape)))
        if self.v_base.device != coef.device or self.upsampler._par.device != coef.device:
            raise ValueError('%s: the tables are not on the device of coef; move the module with .to()' % what)
        return BodyOutput(*_Body.apply(coef.reshape(L).contiguous(), joint_offset.reshape(J, 3).contiguous(), self))
