"""HIP scene-Gaussian stage: a drop-in for the body of ExAvatar's ``SceneGaussian.forward``.

* ``scene_assets(mean, opacity, scale, rotation, feature_dc, feature_rest, sh_degree, cam_param)`` -- reference
  ``avatar/common/nets/module.py:253-272``: ``sigmoid`` / ``exp`` on the opacity and the scale,
  ``matrix_to_quaternion(rotation_6d_to_matrix(rotation))`` and ``eval_sh`` of the coefficients seen from the camera
  centre, ``+ 0.5``, clamped at 0, in ONE launch (the reference runs well over a hundred P-sized ones, forward plus
  backward, and reads the device back at the boolean-mask gather of ``matrix_to_quaternion`` and at every
  ``if deg > k`` of ``eval_sh``).  Returns the reference's asset dict ``{'mean_3d', 'opacity', 'scale', 'rotation',
  'rgb'}``; gradients reach all six parameters, bit-reproducibly.

The kernels are ``csrc/scene_assets.hip`` behind ``include/exa_raster.h`` (``exa_raster_scene_assets_*``); ROCm device
tensors only, no CPU path.  The CPU restatement that pins them is ``tests/scene_oracle.py``.

Semantics
---------
``include/exa_raster.h`` writes out every operation and the order of every sum.  Everything is rounded in fp32 without
fused multiply-adds, and only ``+ - * / sqrt`` occur outside the two activations, so all outputs and gradients except
``opacity`` and ``scale`` (the device's ``expf``) equal the float32 numpy restatement bit for bit.  The camera centre
``inverse(R) (-t)`` is computed on the device by cofactors: no ``torch.inverse``, no read-back.  ``mean_3d`` is the
caller's own ``mean``, untouched, as in the reference; the node adds the view-direction term of its gradient and autograd
adds what reaches ``mean_3d`` itself.

The backward is one launch without atomics (one Gaussian is one lane and nothing is summed across Gaussians).  The
rotation's gradient is torch's autograd of the expression: ``clamp_min`` / ``norm`` conventions at the eps switch of
``F.normalize``, nothing through the candidate index or the sign; a zero row gets finite values.  The colour's gradient is
masked where the unclamped colour is ``< 0``.  The rows of ``feature_rest`` above the active degree get exactly ``+0``.
A gradient nobody needs is not computed, and a missing cotangent counts as zero.

``sh_degree`` is a host int -- ``int(min(itr // cfg.increase_sh_degree_interval, cfg.max_sh_degree))``, not the
reference's device buffer ``active_sh_degree`` -- with ``(sh_degree + 1) ** 2 <= 1 + Mr``.  Each call allocates its
outputs and launches one kernel each way without synchronising, so it can be captured into a hipGraph; a capture bakes
``sh_degree`` in (capture again when the degree goes up), while the parameters and the camera are read at replay.
"""
import torch

from . import _lib
from ._device import _ptr, check_no_grad, check_tensor, grad_in, launch

REST_ROWS = (0, 3, 8, 15)      # feature_rest rows of SH degree 0 .. 3
KEYS = ('mean_3d', 'opacity', 'scale', 'rotation', 'rgb')


class _SceneAssets(torch.autograd.Function):
    """mean [P, 3], opacity [P, 1], scale [P, 3], rotation [P, 6], dc [P, 1, 3], rest [P, Mr, 3], R [3, 3], t [3] (all
    float32, contiguous) -> (opacity [P, 1], scale [P, 3], rotation [P, 4], rgb [P, 3])."""

    @staticmethod
    def forward(ctx, mean, opacity, scale, rotation, dc, rest, R, t, sh_degree):
        P, Mr, dev = mean.shape[0], rest.shape[1], mean.device
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
        opacity_out, scale_out, rotation_out, rgb = new(P, 1), new(P, 3), new(P, 4), new(P, 3)
        launch(_lib.RASTER, 'exa_raster_scene_assets_forward', dev, P, Mr, sh_degree, _ptr(mean), _ptr(opacity),
               _ptr(scale), _ptr(rotation), _ptr(dc), _ptr(rest) if Mr else None, _ptr(R), _ptr(t), _ptr(opacity_out),
               _ptr(scale_out), _ptr(rotation_out), _ptr(rgb))
        ctx.save_for_backward(mean, rotation, dc, rest, R, t, opacity_out, scale_out)
        ctx.sh_degree = sh_degree
        ctx.set_materialize_grads(False)      # a missing cotangent arrives as None and travels as NULL
        return opacity_out, scale_out, rotation_out, rgb

    @staticmethod
    def backward(ctx, g_opacity, g_scale, g_rotation, g_rgb):
        mean, rotation, dc, rest, R, t, opacity_out, scale_out = ctx.saved_tensors
        P, Mr, dev = mean.shape[0], rest.shape[1], mean.device
        need = ctx.needs_input_grad
        new = lambda on, *shape: torch.empty(shape, dtype=torch.float32, device=dev) if on else None      # noqa: E731
        gm, go, gs, gr = new(need[0], P, 3), new(need[1], P, 1), new(need[2], P, 3), new(need[3], P, 6)
        gdc, grest = new(need[4], P, 1, 3), new(need[5], P, Mr, 3)
        if any(need[:6]):
            launch(_lib.RASTER, 'exa_raster_scene_assets_backward', dev, P, Mr, ctx.sh_degree, _ptr(mean), _ptr(rotation),
                   _ptr(dc), _ptr(rest) if Mr else None, _ptr(R), _ptr(t), _ptr(opacity_out), _ptr(scale_out),
                   _ptr(grad_in(g_opacity)), _ptr(grad_in(g_scale)), _ptr(grad_in(g_rotation)), _ptr(grad_in(g_rgb)),
                   _ptr(gm), _ptr(go), _ptr(gs), _ptr(gr), _ptr(gdc), _ptr(grest) if Mr else None)
        return gm, go, gs, gr, gdc, grest, None, None, None


def scene_assets(mean, opacity, scale, rotation, feature_dc, feature_rest, sh_degree, cam_param):
    """The scene's asset dict for one camera (module docstring): ``{'mean_3d', 'opacity', 'scale', 'rotation', 'rgb'}``.

    ``mean`` [P, 3], ``opacity`` [P, 1] (logits), ``scale`` [P, 3] (logs), ``rotation`` [P, 6], ``feature_dc``
    [P, 1, 3], ``feature_rest`` [P, Mr, 3] with Mr in (0, 3, 8, 15): float32 tensors on one ROCm device; ``sh_degree``
    a host int, 0 .. 3, with ``(sh_degree + 1) ** 2 <= 1 + Mr``; ``cam_param`` a dict with ``'R'`` [3, 3] and ``'t'``
    [3] on the same device (camera data: no gradient).  ``mean_3d`` is ``mean`` itself."""
    what = 'scene_assets'
    params = (('mean', mean, (3,)), ('opacity', opacity, (1,)), ('scale', scale, (3,)), ('rotation', rotation, (6,)),
              ('feature_dc', feature_dc, (1, 3)), ('feature_rest', feature_rest, (None, 3)))
    for name, x, _ in params:
        check_tensor(what, name, x)
    if isinstance(sh_degree, bool) or not isinstance(sh_degree, int):
        raise TypeError('%s: sh_degree must be a host int (int(min(itr // interval, max_sh_degree))), not %s' % (
            what, type(sh_degree).__name__))
    try:
        R, t = cam_param['R'], cam_param['t']
    except (TypeError, KeyError, IndexError):
        raise TypeError("%s: cam_param must be a dict with 'R' and 't'" % what) from None
    check_tensor(what, "cam_param['R']", R)
    check_tensor(what, "cam_param['t']", t)
    if mean.dim() != 2 or mean.shape[1] != 3:
        raise ValueError('%s: mean must be [P, 3] (it has %s)' % (what, tuple(mean.shape)))
    P = mean.shape[0]
    for name, x, tail in params[1:5]:
        if tuple(x.shape) != (P,) + tail:
            raise ValueError('%s: %s must be [P, %s] with P = %d (it has %s)' % (
                what, name, ', '.join(map(str, tail)), P, tuple(x.shape)))
    if feature_rest.dim() != 3 or feature_rest.shape[0] != P or feature_rest.shape[2] != 3 \
            or feature_rest.shape[1] not in REST_ROWS:
        raise ValueError('%s: feature_rest must be [P, Mr, 3] with P = %d and Mr in %s (it has %s)' % (
            what, P, REST_ROWS, tuple(feature_rest.shape)))
    Mr = feature_rest.shape[1]
    if not 0 <= sh_degree <= 3:
        raise ValueError('%s: sh_degree must be 0 .. 3 (it is %d)' % (what, sh_degree))
    if (sh_degree + 1) ** 2 > 1 + Mr:
        raise ValueError('%s: sh_degree %d needs %d rows of feature_rest (it has %d)' % (
            what, sh_degree, (sh_degree + 1) ** 2 - 1, Mr))
    if tuple(R.shape) != (3, 3):
        raise ValueError("%s: cam_param['R'] must be [3, 3] (it has %s)" % (what, tuple(R.shape)))
    if t.numel() != 3:
        raise ValueError("%s: cam_param['t'] must hold 3 elements (it has %s)" % (what, tuple(t.shape)))
    check_no_grad(what, "cam_param['R']", R, kind='camera data')
    check_no_grad(what, "cam_param['t']", t, kind='camera data')
    for name, x in [(n, x) for n, x, _ in params] + [("cam_param['R']", R), ("cam_param['t']", t)]:
        check_tensor(what, name, x, f32=False, rocm=True, on=(mean, 'mean'))
    if P == 0:
        e = lambda *shape: mean.new_empty(shape)      # noqa: E731
        return {'mean_3d': mean, 'opacity': e(0, 1), 'scale': e(0, 3), 'rotation': e(0, 4), 'rgb': e(0, 3)}
    op, sc, rot, rgb = _SceneAssets.apply(mean.contiguous(), opacity.contiguous(), scale.contiguous(),
                                          rotation.contiguous(), feature_dc.contiguous(), feature_rest.contiguous(),
                                          R.contiguous(), t.reshape(3).contiguous(), sh_degree)
    return {'mean_3d': mean, 'opacity': op, 'scale': sc, 'rotation': rot, 'rgb': rgb}
