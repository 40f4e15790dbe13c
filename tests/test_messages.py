"""The exact text of the argument errors that the feature modules raise through the shared host layer
(``_device.check_tensor``, ``check_no_grad``, ``need_rocm``): type and ``str(exc)`` of every such raise, compared with
``==``.  The expected strings were recorded by running these calls before the modules shared the helpers, so a reworded
message, a changed exception type or a check that moved in front of another fails here.

Every call fails its checks before any kernel is launched.  The cases that need no device are the CPU test; the ones
that must get past the ROCm guard are the one GPU test.  Those whose two tensors must sit on two different ROCm devices
are part of it where there are two; their strings were read from the earlier source, not recorded, for want of a second
device."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import exavatar_release_amd as exa
from exavatar_release_amd.blend_shapes import BlendTable, make_table

V, J = 6, 3
FACE = np.array([[0, 1, 2], [1, 2, 3], [2, 3, 4], [3, 4, 5]])
NO_CPU = 'exavatar_release_amd: %s runs on a ROCm device only (no CPU path)'


def _f(*shape, device=None):
    return torch.zeros(*shape, device=device)


def _grad(x):
    return x.clone().requires_grad_(True)


def _mlp(device=None):
    return exa.FusedMLP(nn.Sequential(nn.Linear(8, 128), nn.GroupNorm(4, 128), nn.ReLU(), nn.Linear(128, 3)).to(device))


def _blend(device=None):
    expr_dirs = _f(V, 3, 2, device=device)
    expr_dirs[:2] = 1.0
    return _f(4, 3 * V, device=device), expr_dirs, torch.arange(V, device=device) < 3


def cpu_cases():
    """[(label, call, exception type, message)] that fail without a device."""
    x, T, W, R, t = _f(V, 3), torch.eye(4).repeat(J, 1, 1), _f(V, J), torch.eye(3), _f(3)
    sk = exa.skin_points
    pose_dirs, expr_dirs, mask = _blend()
    shapes = exa.BlendShapes(pose_dirs, expr_dirs, mask)
    plan = shapes.expr_plan
    reg = exa.LaplacianReg(V, FACE)
    out = _f(1, V, 3)
    mlp = _mlp()
    a = _f(1, 5, 3)
    img = _f(1, 3, 16, 16)
    return [
        ('skin weight grad', lambda: sk(x, T, _grad(W)), ValueError,
         'skin_points: skinning_weight is a buffer in the reference and gets no gradient; detach it'),
        ('skin R grad', lambda: sk(x, T, W, R=_grad(R), t=t), ValueError,
         'skin_points: R is camera data in the reference and gets no gradient; detach it'),
        ('skin t grad', lambda: sk(x, T, W, R=R, t=_grad(t)), ValueError,
         'skin_points: t is camera data in the reference and gets no gradient; detach it'),
        ('skin T type', lambda: sk(x, T.numpy(), W), TypeError, 'skin_points: transform_mat_joint must be a tensor'),
        ('skin T dtype', lambda: sk(x, T.double(), W), ValueError,
         'skin_points: transform_mat_joint must be float32 (it is torch.float64)'),
        ('skin points type', lambda: sk((x, x.numpy()), T, W), TypeError, 'skin_points: points[1] must be a tensor'),
        ('skin points dtype', lambda: sk(x.half(), T, W), ValueError,
         'skin_points: points[0] must be float32 (it is torch.float16)'),
        ('skin weight type', lambda: sk(x, T, W.numpy()), TypeError, 'skin_points: skinning_weight must be a tensor'),
        ('skin weight dtype', lambda: sk(x, T, W.double()), ValueError,
         'skin_points: skinning_weight must be float32 (it is torch.float64)'),
        ('skin trans type', lambda: sk(x, T, W, trans=[0.0, 0.0, 0.0]), TypeError, 'skin_points: trans must be a tensor'),
        ('skin trans dtype', lambda: sk(x, T, W, trans=t.double()), ValueError,
         'skin_points: trans must be float32 (it is torch.float64)'),
        ('skin R type', lambda: sk(x, T, W, R=R.numpy(), t=t), TypeError, 'skin_points: R must be a tensor'),
        ('skin R dtype', lambda: sk(x, T, W, R=R.double(), t=t), ValueError,
         'skin_points: R must be float32 (it is torch.float64)'),
        ('skin R shape', lambda: sk(x, T, W, R=torch.eye(4), t=t), ValueError,
         'skin_points: R must have shape (3, 3) (it has (4, 4))'),
        ('skin t type', lambda: sk(x, T, W, R=R, t=t.numpy()), TypeError, 'skin_points: t must be a tensor'),
        ('skin t dtype', lambda: sk(x, T, W, R=R, t=t.double()), ValueError,
         'skin_points: t must be float32 (it is torch.float64)'),
        ('skin cpu', lambda: sk(x, T, W, R=R, t=t), RuntimeError, NO_CPU % 'skin_points'),

        ('mlp block type', lambda: mlp(_f(2, 8).numpy()), TypeError, 'FusedMLP: input block 0 must be a tensor'),
        ('mlp block dtype', lambda: mlp(_f(2, 8).double()), ValueError,
         'FusedMLP: input block 0 must be float32 (it is torch.float64)'),
        ('mlp cpu', lambda: mlp(_f(2, 8)), RuntimeError,
         'exavatar_release_amd: FusedMLP runs on a ROCm device only (no CPU path); input block 0 is on cpu'),

        ('lap out type', lambda: reg(out.numpy(), None), TypeError, 'LaplacianReg: out must be a tensor'),
        ('lap cpu', lambda: reg(out, out.clone()), RuntimeError, NO_CPU % 'LaplacianReg'),
        ('lap loss out type', lambda: exa.mesh_laplacian_loss(None, None, reg.neighbor_idxs, reg.neighbor_weights),
         TypeError, 'mesh_laplacian_loss: out must be a tensor'),
        ('lap loss table grad', lambda: exa.mesh_laplacian_loss(out, None, reg.neighbor_idxs, _grad(reg.neighbor_weights)),
         ValueError, 'mesh_laplacian_loss: neighbor_weights is data in the reference and gets no gradient; detach it'),
        ('lap loss cpu', lambda: exa.mesh_laplacian_loss(out, None, reg.neighbor_idxs.cpu(), reg.neighbor_weights.cpu()),
         RuntimeError, NO_CPU % 'mesh_laplacian_loss'),

        ('table dirs grad', lambda: make_table(_grad(pose_dirs), mask.repeat_interleave(3)), ValueError,
         'make_table: dirs is data in the reference and gets no gradient; detach it'),
        ('table dirs dtype', lambda: make_table(pose_dirs.double(), mask.repeat_interleave(3)), ValueError,
         'make_table: dirs must be float32 (it is torch.float64)'),
        ('shapes pose_dirs type', lambda: exa.BlendShapes(pose_dirs.numpy(), expr_dirs, mask), TypeError,
         'BlendShapes: pose_dirs must be a tensor'),
        ('shapes expr_dirs type', lambda: exa.BlendShapes(pose_dirs, expr_dirs.numpy(), mask), TypeError,
         'BlendShapes: expr_dirs must be a tensor'),
        ('shapes pose_mask type', lambda: exa.BlendShapes(pose_dirs, expr_dirs, mask.numpy()), TypeError,
         'BlendShapes: pose_mask must be a tensor'),
        ('shapes pose_dirs grad', lambda: exa.BlendShapes(_grad(pose_dirs), expr_dirs, mask), ValueError,
         'BlendShapes: pose_dirs is data in the reference and gets no gradient; detach it'),
        ('shapes expr_dirs grad', lambda: exa.BlendShapes(pose_dirs, _grad(expr_dirs), mask), ValueError,
         'BlendShapes: expr_dirs is data in the reference and gets no gradient; detach it'),
        ('shapes pose_dirs dtype', lambda: exa.BlendShapes(pose_dirs.double(), expr_dirs.double(), mask), ValueError,
         'BlendShapes: pose_dirs must be float32 (it is torch.float64)'),
        ('shapes expr_dirs dtype', lambda: exa.BlendShapes(pose_dirs, expr_dirs.half(), mask), ValueError,
         'BlendShapes: expr_dirs must be float32 (it is torch.float16)'),
        ('blend table grad', lambda: exa.blend_offsets(_f(2), BlendTable(_grad(plan.table), plan.cols, plan.inv)),
         ValueError, 'blend_offsets: table is data in the reference and gets no gradient; detach it'),
        ('blend coef type', lambda: exa.blend_offsets([0.0, 0.0], plan), TypeError, 'blend_offsets: coef must be a tensor'),
        ('blend cpu', lambda: exa.blend_offsets(_f(2), plan), RuntimeError, NO_CPU % 'blend_offsets'),
        ('expr type', lambda: shapes.expr_offsets(np.zeros(2, np.float32)), TypeError,
         'BlendShapes.expr_offsets: expr must be a tensor'),
        ('expr cpu', lambda: shapes.expr_offsets(_f(2)), RuntimeError, NO_CPU % 'BlendShapes.expr_offsets'),
        ('pose cpu', lambda: shapes.pose_offsets(_f(4), _f(V, 3)), RuntimeError, NO_CPU % 'BlendShapes.pose_offsets'),

        ('knn cpu', lambda: exa.knn_points(a, a), RuntimeError, NO_CPU % 'knn_points'),
        ('triplane cpu', lambda: exa.TriplaneFeatures(_f(V, 3), torch.zeros(V, dtype=torch.bool)), RuntimeError,
         NO_CPU % 'TriplaneFeatures'),
        ('mesh cpu', lambda: exa.get_face_index_map_xy(_f(1, V, 3), FACE, {}, (8, 8)), RuntimeError,
         NO_CPU % 'get_face_index_map_xy'),
        ('normals cpu', lambda: exa.vertex_normals(_f(1, V, 3), FACE), RuntimeError, NO_CPU % 'vertex_normals'),
        ('l1 cpu', lambda: exa.RGBLoss()(img, img), RuntimeError, NO_CPU % 'RGBLoss'),
        ('ssim cpu', lambda: exa.SSIM()(img, img), RuntimeError, NO_CPU % 'the fused SSIM'),
        ('photo cpu', lambda: exa.PhotometricLoss()(img, img), RuntimeError, NO_CPU % 'PhotometricLoss'),
    ]


def gpu_cases():
    """[(label, call, exception type, message)] that get past the ROCm guard of their first argument."""
    dev = torch.device('cuda:0')
    x, T, W = _f(V, 3, device=dev), torch.eye(4, device=dev).repeat(J, 1, 1), _f(V, J, device=dev)
    sk = exa.skin_points
    pose_dirs, expr_dirs, mask = _blend(dev)
    shapes = exa.BlendShapes(pose_dirs, expr_dirs, mask)
    plan = shapes.expr_plan
    reg = exa.LaplacianReg(V, FACE)
    out, w = _f(1, V, 3, device=dev), _f(V, device=dev)
    lap = exa.mesh_laplacian_loss
    cases = [
        ('skin weight cpu', lambda: sk(x, T, W.cpu()), RuntimeError, NO_CPU % 'skin_points'),
        ('mlp weights elsewhere', lambda: _mlp()(_f(2, 8, device=dev)), ValueError,
         'FusedMLP: input block 0 is not on the device of the weights'),
        ('lap out dtype', lambda: reg(out.double(), None), ValueError,
         'LaplacianReg: out must be float32 (it is torch.float64)'),
        ('lap target dtype', lambda: reg(out, out.half()), ValueError,
         'LaplacianReg: target must be float32 (it is torch.float16)'),
        ('lap weight dtype', lambda: reg(out, None, w.double()), ValueError,
         'LaplacianReg: weight must be float32 (it is torch.float64)'),
        ('lap target cpu', lambda: reg(out, out.cpu()), RuntimeError, NO_CPU % 'LaplacianReg'),
        ('lap target grad', lambda: reg(out, _grad(out)), ValueError,
         'LaplacianReg: target is data in the reference and gets no gradient; detach it'),
        ('lap weight grad', lambda: reg(out, None, _grad(w)), ValueError,
         'LaplacianReg: weight is data in the reference and gets no gradient; detach it'),
        ('lap loss target dtype', lambda: lap(out, out.double(), reg.neighbor_idxs, reg.neighbor_weights), ValueError,
         'mesh_laplacian_loss: target must be float32 (it is torch.float64)'),
        ('lap loss weight grad', lambda: lap(out, None, reg.neighbor_idxs, reg.neighbor_weights, _grad(w)), ValueError,
         'mesh_laplacian_loss: weight is data in the reference and gets no gradient; detach it'),
        ('blend coef dtype', lambda: exa.blend_offsets(_f(2, device=dev).double(), plan), ValueError,
         'blend_offsets: coef must be float32 (it is torch.float64)'),
        ('blend base dtype', lambda: exa.blend_offsets(_f(2, device=dev), plan, _f(3 * V, device=dev).half()), ValueError,
         'blend_offsets: base must be float32 (it is torch.float16)'),
        ('blend base cpu', lambda: exa.blend_offsets(_f(2, device=dev), plan, _f(3 * V)), RuntimeError,
         NO_CPU % 'blend_offsets'),
        ('expr dtype', lambda: shapes.expr_offsets(_f(2, device=dev).double()), ValueError,
         'BlendShapes.expr_offsets: coef must be float32 (it is torch.float64)'),
        ('pose base dtype', lambda: shapes.pose_offsets(_f(4, device=dev), _f(V, 3, device=dev).double()), ValueError,
         'BlendShapes.pose_offsets: base must be float32 (it is torch.float64)'),
    ]
    if torch.cuda.device_count() > 1:
        far = torch.device('cuda:1')
        cases += [
            ('skin points elsewhere', lambda: sk(x.to(far), T, W), ValueError,
             'skin_points: points[0] is not on the device of transform_mat_joint'),
            ('skin idx elsewhere', lambda: sk(x, T, W, idx=torch.arange(V, device=far)), ValueError,
             'skin_points: idx is not on the device of transform_mat_joint'),
            ('lap target elsewhere', lambda: reg(out, out.to(far)), ValueError,
             'LaplacianReg: target is not on the device of out'),
            ('lap loss weight elsewhere', lambda: lap(out, None, reg.neighbor_idxs, reg.neighbor_weights, w.to(far)),
             ValueError, 'mesh_laplacian_loss: weight is not on the device of out'),
            ('blend base elsewhere', lambda: exa.blend_offsets(_f(2, device=dev), plan, _f(3 * V, device=far)),
             ValueError, 'blend_offsets: base is not on the device of coef'),
        ]
    return cases


def raised(call):
    """(exception type, message) of ``call``, or (None, None) when it returns."""
    try:
        call()
    except Exception as e:      # noqa: BLE001  (the type is what is compared)
        return type(e), str(e)
    return None, None


def _check(cases):
    got = [(label,) + raised(call) for label, call, _, _ in cases]
    want = [(label, exc, msg) for label, _, exc, msg in cases]
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, '\n'.join('%s: raised %s %r, expected %s %r' % (g[0], g[1], g[2], w[1], w[2]) for g, w in wrong)


def test_argument_errors_without_a_device_keep_their_type_and_text():
    _check(cpu_cases())


@pytest.mark.gpu
def test_argument_errors_on_the_device_keep_their_type_and_text():
    _check(gpu_cases())
