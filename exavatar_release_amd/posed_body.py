"""HIP posed SMPL-X stage: a drop-in for ExAvatar's ``Model.get_smplx_outputs`` (``avatar/main/model.py:37-58``), the
``smplx_layer`` call whose pose varies per frame, with the camera -> world step behind it.

``PosedBody(...)`` is ONE autograd node with one C call each way (``exa_mesh_posed_*`` of ``include/exa_mesh.h``,
``csrc/posed_body.hip``): smplx's ``batch_rodrigues`` on the device, the shape and expression blend, the joint
regression, the 486 x 3 V pose correctives as a function of the live pose, ``batch_rigid_transform``, the dense skinning,
``+ transl`` and ``inverse(R) (vertices - t)``.  The shape blend, the regression and the two-level sums are the template
stage's launches (``csrc/body.hip``); the chain and the skinning are the library's own ``exa_mesh_kinematics_*`` and
``exa_skin_*``.  ``pose`` is the layer's [J, 3] axis-angle in its own joint order -- for SMPL-X exactly the ``'pose'``
entry of ``SMPLXParamDict.forward(..., packed=True)``, so nothing is concatenated -- and ``betas`` / ``expression`` travel
as two pointers.  One sample per call, as in the reference.  ROCm device tensors only, no CPU path.  The CPU restatement
that pins the stage bit for bit is ``tests/posed_oracle.py``.

Semantics (the header writes out every order)
---------------------------------------------
``full = pose + pose_mean``; ``rot = I + sin(angle) K + (1 - cos(angle)) K K`` with ``angle = |full + 1e-8|`` and K the
cross-product matrix of ``full / angle`` (``lbs.py:311-345``; the ``1e-8`` keeps the gradient finite at a zero row);
``v_shaped = (v_template + face_offset) + sum_l coef[l] dirs[v][c][l]``; ``Jr = J_regressor v_shaped + joint_offset``,
every row of ``joint_offset`` added as given (``model.py:50`` passes the parameter itself, the root row included);
``v_posed = (rot[1:] - I).view(-1) @ posedirs + v_shaped``; the chain over ``Jr`` with ``rot``; the skinning of
``v_posed``; ``+ transl`` on the vertices and the posed joints; ``vertices_world = inverse(R) (vertices - t)``.  Every
operation is rounded in fp32 without fused multiply-adds, every sum runs in an order that depends on the sizes and the
tables alone, and no kernel uses an atomic: the same inputs give the same bits, forward and backward.  ``sinf`` / ``cosf``
are the only transcendentals.

The extra joints of ``vertex_joint_selector`` and the static and dynamic landmarks -- the rest of the layer's ``joints`` --
are ``exavatar_release_amd.keypoints.BodyKeypoints``, which takes this stage's ``vertices``, ``joints`` and ``rot`` stacked
over the frames.  Not covered: ``joint_mapper``, PCA hands, ``locator_offset`` and a gradient to ``face_offset`` (the avatar
code reads only ``output.vertices``); batches of frames per call.
"""
import collections
import ctypes

import torch

from . import _lib
from ._device import _ptr, _workspace, check_no_grad, check_tensor, config, grad_in, launch
from .body import _f32, _SmplxTables

PosedBodyOutput = collections.namedtuple('PosedBodyOutput', ['vertices', 'joints', 'vertices_world', 'rot'])

_IP = ctypes.POINTER(ctypes.c_int32)


class _Posed(torch.autograd.Function):
    """pose [J, 3], betas [Lb], expression [Le], transl [3], joint_offset [J, 3] or None (float32, contiguous), Rinv
    [3, 3] and t [3] or None, the module -> vertices, joints, vertices_world (or None), rot."""

    @staticmethod
    def forward(ctx, pose, betas, expression, transl, joint_offset, Rinv, t, body):
        dev = pose.device
        V, J = body.num_verts, body.num_joints
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
        vertices, joints, rot = new(V, 3), new(J, 3), new(J, 3, 3)
        world = new(V, 3) if Rinv is not None else None
        desc, fwd_bytes, _ = body._descriptor()
        ws = _workspace(fwd_bytes, dev)
        Lb = betas.shape[0]
        launch(_lib.MESH, 'exa_mesh_posed_forward', dev, desc, Lb, _ptr(pose), _ptr(betas if Lb else None),
               _ptr(expression if expression.shape[0] else None), _ptr(transl), _ptr(joint_offset), _ptr(Rinv), _ptr(t),
               _ptr(ws), fwd_bytes, _ptr(vertices), _ptr(joints), _ptr(world), _ptr(rot))
        ctx.save_for_backward(ws, pose, Rinv)
        ctx.body, ctx.Lb, ctx.Le = body, Lb, expression.shape[0]
        ctx.mark_non_differentiable(rot)
        ctx.set_materialize_grads(False)      # a missing cotangent arrives as None and travels as NULL
        if config.keep_debug:
            body.debug_workspace = ws
        return vertices, joints, world, rot

    @staticmethod
    def backward(ctx, g_vertices, g_joints, g_world, _g_rot):
        want = ctx.needs_input_grad[:5]
        if not any(want):
            return (None,) * 8
        ws, pose, Rinv = ctx.saved_tensors
        body = ctx.body
        dev = ws.device
        J = body.num_joints
        desc, fwd_bytes, bwd_bytes = body._descriptor()
        new = lambda ok, *shape: torch.empty(shape, dtype=torch.float32, device=dev) if ok else None      # noqa: E731
        dpose, dbetas, dexpr = new(want[0], J, 3), new(want[1], ctx.Lb), new(want[2], ctx.Le)
        dtransl, djo = new(want[3], 3), new(want[4], J, 3)
        bws = _workspace(bwd_bytes, dev)
        grads = [grad_in(g) for g in (g_vertices, g_joints, g_world)]
        launch(_lib.MESH, 'exa_mesh_posed_backward', dev, desc, ctx.Lb, _ptr(pose), _ptr(Rinv), _ptr(ws), fwd_bytes,
               *(_ptr(g) for g in grads), _ptr(bws), bwd_bytes, _ptr(dpose), _ptr(dbetas if ctx.Lb else None),
               _ptr(dexpr if ctx.Le else None), _ptr(dtransl), _ptr(djo))
        return dpose, dbetas, dexpr, dtransl, djo, None, None, None


class PosedBody(_SmplxTables):
    """The posed SMPL-X layer of ``get_smplx_outputs`` (module docstring).

    ``v_template`` [V, 3], ``shape_dirs`` [V, 3, L] (1 <= L <= 512: ``cat(shapedirs, expr_dirs)``), ``posedirs``
    [9 (J - 1), 3 V] in the layer's own layout, ``J_regressor`` [J, V], ``lbs_weights`` [V, J] (J <= 64), ``parents`` a
    sequence or CPU tensor of J ints, ``pose_mean`` [J, 3] or [3 J] or None, ``face_offset`` [V, 3] or None.  All of them
    are data (float32): a tensor that requires a gradient is refused.  The re-laid tables are non-persistent buffers, so
    ``state_dict`` stays empty and ``.to(device)`` moves them; the sparse ``J_regressor`` is compacted once to its
    non-zeros."""

    def __init__(self, v_template, shape_dirs, posedirs, J_regressor, lbs_weights, parents, *, pose_mean=None,
                 face_offset=None):
        super(PosedBody, self).__init__()
        what = 'PosedBody'
        self._check_data(what, (('v_template', v_template, False), ('shape_dirs', shape_dirs, False),
                                ('posedirs', posedirs, False), ('J_regressor', J_regressor, False),
                                ('lbs_weights', lbs_weights, False), ('pose_mean', pose_mean, True),
                                ('face_offset', face_offset, True)))
        V, _, J = self._check_tables(what, v_template, shape_dirs, J_regressor, parents, lbs_weights)
        if tuple(posedirs.shape) != (9 * (J - 1), 3 * V):
            raise ValueError('%s: posedirs must be [9 (J - 1), 3 V] = [%d, %d] (it is %s)'
                             % (what, 9 * (J - 1), 3 * V, tuple(posedirs.shape)))
        if pose_mean is not None and pose_mean.numel() != 3 * J:
            raise ValueError('%s: pose_mean must hold 3 J = %d values (it is %s)' % (what, 3 * J, tuple(pose_mean.shape)))
        if face_offset is not None and tuple(face_offset.shape) != (V, 3):
            raise ValueError('%s: face_offset must be [V, 3] with V = %d (it is %s)' % (what, V, tuple(face_offset.shape)))
        own = (('posedirs', posedirs.contiguous().clone()),
               ('pose_mean', None if pose_mean is None else pose_mean.reshape(J, 3).contiguous().clone()))
        self._register_tables(v_template, face_offset, shape_dirs, own, J_regressor, lbs_weights)
        self.debug_workspace = None          # config.keep_debug: the most recent forward's workspace

    @classmethod
    def from_layer(cls, smplx_layer, *, face_offset=None):
        """From a (vendored) smplx ``SMPLX`` layer: its ``v_template``, ``cat(shapedirs, expr_dirs)``, ``posedirs``,
        ``J_regressor``, ``lbs_weights``, ``parents`` and ``pose_mean`` (a layer without one, or with ``flat_hand_mean``'s
        zeros, adds nothing that changes a value)."""
        v_template, shape_dirs, parents = cls._layer_tables(smplx_layer)
        dev = v_template.device
        pose_mean = getattr(smplx_layer, 'pose_mean', None)
        return cls(v_template, shape_dirs, _f32(smplx_layer.posedirs), _f32(smplx_layer.J_regressor),
                   _f32(smplx_layer.lbs_weights), parents,
                   pose_mean=None if pose_mean is None else _f32(torch.as_tensor(pose_mean)).to(dev),
                   face_offset=None if face_offset is None else _f32(face_offset).to(dev))

    def _descriptor(self):
        """(the ``ExaMeshPosed`` the C ABI takes, forward workspace bytes, backward workspace bytes); rebuilt when the
        buffers moved."""
        def make(p):
            return _lib.ExaMeshPosed(self.num_verts, self.num_coef, self.num_joints, self.nnz,
                                     ctypes.cast(self._parents, _IP), p(self.v_base), p(self.dirs), p(self.posedirs),
                                     p(self.pose_mean), p(self.jreg_off), p(self.jreg_col), p(self.jreg_val),
                                     p(self.jregT_off), p(self.jregT_row), p(self.jregT_val), p(self.weights))

        return self._cached_descriptor(self.v_base.data_ptr(), 'exa_mesh_posed_workspace_sizes', make)

    def forward(self, pose, betas, expression, transl, joint_offset=None, R=None, t=None):
        """``pose`` [J, 3] axis-angle in the layer's joint order, ``betas`` [Lb], ``expression`` [Le] (Lb + Le == L, either
        may be empty), ``transl`` [3], ``joint_offset`` [J, 3] or None -- each may carry one leading axis of 1 -- and the
        camera data ``R`` [3, 3], ``t`` [3] or neither (float32, ROCm) -> ``PosedBodyOutput``: ``vertices`` [V, 3]
        (``output.vertices[0]``, camera space), ``joints`` [J, 3] (the first J rows of ``output.joints[0]``),
        ``vertices_world`` [V, 3] (``get_smplx_outputs``' result; None without a camera) and ``rot`` [J, 3, 3] (the
        Rodrigues rotations, not differentiable).  Gradients reach ``pose``, ``betas``, ``expression``, ``transl`` and
        ``joint_offset``."""
        what = 'PosedBody'
        L, J = self.num_coef, self.num_joints
        check_tensor(what, 'pose', pose, rocm=True)
        named = [('betas', betas), ('expression', expression), ('transl', transl)]
        if joint_offset is not None:
            named.append(('joint_offset', joint_offset))
        if (R is None) != (t is None):
            raise ValueError('%s: R and t must be given together' % what)
        if R is not None:
            named += [('R', R), ('t', t)]
        for name, x in named:
            check_tensor(what, name, x, rocm=True, on=(pose, 'pose'))
        check_no_grad(what, 'R', R, 'camera data')
        check_no_grad(what, 't', t, 'camera data')

        def one(name, x, shape, spelled):
            """x without its leading axis of 1; any other batch is refused."""
            if x.dim() == len(shape) + 1 and tuple(x.shape[1:]) == shape and x.shape[0] != 1:
                raise ValueError('%s: %s holds a batch of %d; the stage takes one sample per call, as the reference does'
                                 % (what, name, x.shape[0]))
            if tuple(x.shape) not in (shape, (1,) + shape):
                raise ValueError('%s: %s must be %s (it is %s)' % (what, name, spelled, tuple(x.shape)))
            return x.reshape(shape).contiguous()

        pose = one('pose', pose, (J, 3), '[J, 3] or [1, J, 3] with J = %d' % J)
        for name, x in (('betas', betas), ('expression', expression)):
            if x.dim() == 2 and x.shape[0] != 1:
                raise ValueError('%s: %s holds a batch of %d; the stage takes one sample per call, as the reference does'
                                 % (what, name, x.shape[0]))
            if x.dim() not in (1, 2):
                raise ValueError('%s: %s must be [n] or [1, n] (it is %s)' % (what, name, tuple(x.shape)))
        betas, expression = betas.reshape(-1).contiguous(), expression.reshape(-1).contiguous()
        if betas.shape[0] + expression.shape[0] != L:
            raise ValueError('%s: betas and expression hold %d + %d coefficients, shape_dirs %d'
                             % (what, betas.shape[0], expression.shape[0], L))
        transl = one('transl', transl, (3,), '[3] or [1, 3]')
        if joint_offset is not None:
            joint_offset = one('joint_offset', joint_offset, (J, 3), '[J, 3] or [1, J, 3] with J = %d' % J)
        Rinv = None
        if R is not None:
            if tuple(R.shape) not in ((3, 3), (1, 3, 3)) or t.numel() != 3:
                raise ValueError('%s: R must be [3, 3] and t [3] (they are %s and %s)' % (what, tuple(R.shape), tuple(t.shape)))
            Rinv = torch.inverse(R.reshape(3, 3)).contiguous()
            t = t.reshape(3).contiguous()
        if self.v_base.device != pose.device:
            raise ValueError('%s: the tables are not on the device of pose; move the module with .to()' % what)
        return PosedBodyOutput(*_Posed.apply(pose, betas, expression, transl, joint_offset, Rinv, t, self))
