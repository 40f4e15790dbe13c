"""``SceneGaussian``: the reference's scene-Gaussian module (``avatar/common/nets/module.py:74-272``) over this package's
HIP stages, without its ``cfg`` global.

Same parameters and buffers under the same names (``mean``, ``scale``, ``rotation``, ``feature_dc``, ``feature_rest``,
``opacity``; ``point_num``, ``active_sh_degree``, ``radius_max``, ``xyz_grad_accum``, ``track_cnt``, ``cam_dist_trans``,
``cam_dist_radius``), so checkpoints load both ways, and the same optimizer group names.  ``forward`` is
:func:`scene_assets`, ``track_stats`` is :func:`track_densify_stats`, ``init_from_point_cloud`` uses this package's
:func:`knn_points`, and the one operation that changes P -- ``densify_and_prune``, with ``prune_points`` -- is the
single-pass densification of ``csrc/densify.hip`` (``densify.densify_plan`` / ``densify_apply``): one classification, one
scan, ONE host synchronisation to learn the new P, one move of the six parameters and their Adam moments.  The reference
makes three passes of boolean-mask surgery over eighteen tensors, each mask a synchronisation, and ends with
``empty_cache()``; this class never calls it.

Everything else (construction, ``reset_opacity`` once per 3 000 iterations, the group list) is torch, as in the reference.
Works with ``torch.optim.Adam`` and with this package's ``Adam``: fresh ``nn.Parameter`` s are installed in the groups and
the per-parameter state is re-keyed with ``'step'`` and every other key kept.
"""
import torch
from torch import nn

from .densify import densify_apply, densify_plan, prune_plan, track_densify_stats
from .knn import knn_points
from .scene_assets import scene_assets

PARAMS = ('mean', 'feature_dc', 'feature_rest', 'opacity', 'scale', 'rotation')       # the reference's group order
STATS = ('radius_max', 'xyz_grad_accum', 'track_cnt')
SH_C0 = 0.28209479177387814


class SceneGaussian(nn.Module):
    """The reference's ``SceneGaussian`` (module docstring).  The hyperparameters the reference reads from ``cfg``
    (``avatar/main/config.py:13-31``) are keywords here.  ``split_factor`` is the reference's default argument of
    ``split_points``; ``reference_radius_reset=False`` applies the screen-space prune the reference's code intends but
    never executes (``densify.densify_and_prune``)."""

    def __init__(self, *, max_sh_degree=3, increase_sh_degree_interval=1000, densify_grad_thr=0.0002, opacity_min=0.005,
                 dense_percent_thr=0.01, position_lr_init=0.00016, feature_lr=0.0025, opacity_lr=0.05, scale_lr=0.005,
                 rotation_lr=0.001, split_factor=2, reference_radius_reset=True):
        super().__init__()
        self.max_sh_degree, self.increase_sh_degree_interval = int(max_sh_degree), int(increase_sh_degree_interval)
        self.densify_grad_thr, self.opacity_min, self.dense_percent_thr = densify_grad_thr, opacity_min, dense_percent_thr
        self.position_lr_init, self.feature_lr, self.opacity_lr = position_lr_init, feature_lr, opacity_lr
        self.scale_lr, self.rotation_lr = scale_lr, rotation_lr
        self.split_factor, self.reference_radius_reset = int(split_factor), bool(reference_radius_reset)
        self._sh_degree = 0           # the host's copy of active_sh_degree: scene_assets takes a host int

    # ---- construction ------------------------------------------------------------------------------------------------
    def _register(self, tensors, cam_trans, cam_radius):
        P = tensors['mean'].shape[0]
        device = tensors['mean'].device
        self.register_buffer('point_num', torch.tensor([P], dtype=torch.int64, device=device))
        for k in ('mean', 'scale', 'rotation', 'feature_dc', 'feature_rest', 'opacity'):
            setattr(self, k, nn.Parameter(tensors[k]))
        self.register_buffer('active_sh_degree', torch.zeros(1, dtype=torch.float32, device=device))
        self._sh_degree = 0
        self.register_buffer('radius_max', torch.zeros(P, dtype=torch.float32, device=device))
        self.register_buffer('xyz_grad_accum', torch.zeros(P, 1, dtype=torch.float32, device=device))
        self.register_buffer('track_cnt', torch.zeros(P, 1, dtype=torch.float32, device=device))
        self.register_buffer('cam_dist_trans', cam_trans.to(device))
        self.register_buffer('cam_dist_radius', cam_radius.to(device))

    def init_from_point_cloud(self, xyz, rgb, cam_dist, device='cuda'):
        """Gaussians from a point cloud ``xyz`` / ``rgb`` [P, 3] and the camera distribution ``{'translate', 'radius'}``:
        isotropic scales from the mean squared distance to the three nearest points (this package's ``knn_points``),
        identity rotations, the colour in the first SH band, opacity 0.1."""
        xyz, rgb = xyz.to(device).float(), rgb.to(device).float()
        P = xyz.shape[0]
        points = knn_points(xyz[None], xyz[None], K=4, return_nn=True)
        dist = torch.sum((xyz[:, None, :] - points.knn[0, :, 1:, :]) ** 2, 2).mean(1)
        dist = torch.clamp_min(dist, 0.0000001)
        feature = torch.zeros((P, (self.max_sh_degree + 1) ** 2, 3), dtype=torch.float32, device=xyz.device)
        feature[:, 0, :] = (rgb - 0.5) / SH_C0
        opacity = 0.1 * torch.ones((P, 1), dtype=torch.float32, device=xyz.device)
        self._register({'mean': xyz, 'scale': torch.log(torch.sqrt(dist))[:, None].repeat(1, 3),
                        'rotation': torch.tensor([1.0, 0, 0, 0, 1, 0], device=xyz.device).repeat(P, 1),
                        'feature_dc': feature[:, 0:1, :].contiguous(), 'feature_rest': feature[:, 1:, :].contiguous(),
                        'opacity': torch.log(opacity / (1 - opacity))}, cam_dist['translate'], cam_dist['radius'])

    def init_from_point_num(self, point_num, device='cuda'):
        """Zero Gaussians of the right shapes, to be overwritten by ``load_state_dict``."""
        P = int(point_num)
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)      # noqa: E731
        self._register({'mean': z(P, 3), 'scale': z(P, 3), 'rotation': z(P, 6), 'feature_dc': z(P, 1, 3),
                        'feature_rest': z(P, (self.max_sh_degree + 1) ** 2 - 1, 3), 'opacity': z(P, 1)}, z(3), z(1))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        if prefix + 'active_sh_degree' in state_dict:
            self._sh_degree = int(state_dict[prefix + 'active_sh_degree'].reshape(-1)[0])

    def get_optimizable_params(self):
        return [
            {'params': [self.mean], 'name': 'mean_scene', 'lr': self.position_lr_init * float(self.cam_dist_radius)},
            {'params': [self.feature_dc], 'name': 'feature_dc_scene', 'lr': self.feature_lr},
            {'params': [self.feature_rest], 'name': 'feature_rest_scene', 'lr': self.feature_lr / 20.0},
            {'params': [self.opacity], 'name': 'opacity_scene', 'lr': self.opacity_lr},
            {'params': [self.scale], 'name': 'scale_scene', 'lr': self.scale_lr},
            {'params': [self.rotation], 'name': 'rotation_scene', 'lr': self.rotation_lr},
        ]

    # ---- per iteration -----------------------------------------------------------------------------------------------
    def set_sh_degree(self, itr):
        self._sh_degree = int(min(itr // self.increase_sh_degree_interval, self.max_sh_degree))
        self.active_sh_degree[:] = self._sh_degree

    def track_stats(self, mean_2d_grad, radius):
        """The statistics of one render, for every Gaussian with ``radius > 0``: the reference's ``track_stats`` and the
        ``radius_max`` update of ``avatar/main/model.py:279-285`` in one launch, no synchronisation.  ``radius``: the
        rasterizer's int32 radii."""
        track_densify_stats(mean_2d_grad, radius, self.xyz_grad_accum, self.track_cnt, self.radius_max)

    def forward(self, cam_param):
        return scene_assets(self.mean, self.opacity, self.scale, self.rotation, self.feature_dc, self.feature_rest,
                            self._sh_degree, cam_param)

    # ---- the optimizer's view of the parameters -----------------------------------------------------------------------------
    def _groups(self, what, optimizer, names=PARAMS):
        """name -> the optimizer group whose single member is that parameter."""
        groups = {}
        for name in names:
            p = getattr(self, name)
            for group in optimizer.param_groups:
                if any(q is p for q in group['params']):
                    if len(group['params']) != 1:
                        raise ValueError('%s: %s must be the single member of its optimizer group (the group has %d)' % (
                            what, name, len(group['params'])))
                    groups[name] = group
                    break
            else:
                raise ValueError('%s: %s is in no group of the optimizer' % (what, name))
        return groups

    @staticmethod
    def _moments(what, optimizer, p):
        """The (exp_avg, exp_avg_sq) of ``p`` when the optimizer holds state for it, else ()."""
        state = optimizer.state.get(p)
        if not state:
            return ()
        m, v = state.get('exp_avg'), state.get('exp_avg_sq')
        if not (isinstance(m, torch.Tensor) and isinstance(v, torch.Tensor) and m.shape == p.shape and v.shape == p.shape):
            raise ValueError('%s: the optimizer state of a parameter must hold exp_avg / exp_avg_sq of its shape' % what)
        return (m, v)

    def _install(self, optimizer, groups, new, moments):
        """Fresh parameters into the module and the groups; the state re-keyed, 'step' and every other key kept."""
        for name, group in groups.items():
            old = group['params'][0]
            fresh = nn.Parameter(new[name].requires_grad_(True))
            state = optimizer.state.pop(old, None)
            if state is not None:
                if name in moments:
                    state['exp_avg'], state['exp_avg_sq'] = moments[name]
                optimizer.state[fresh] = state
            group['params'][0] = fresh
            setattr(self, name, fresh)
        self.point_num[:] = new['mean'].shape[0]

    def _move(self, what, plan, optimizer, noise, carried):
        """One move of the six parameters, the moments of every group with state and the ``carried`` statistics."""
        groups = self._groups(what, optimizer)
        with torch.no_grad():
            held = {k: self._moments(what, optimizer, getattr(self, k)) for k in PARAMS}
            states = [t for k in PARAMS for t in held[k]] + [getattr(self, k) for k in carried]
            computed = noise is not False
            others = [k for k in PARAMS if not (computed and k in ('mean', 'scale', 'rotation'))]
            outs = densify_apply(plan, [getattr(self, k) for k in others],
                                 mean=self.mean if computed else None, scale=self.scale if computed else None,
                                 rotation=self.rotation if computed else None,
                                 noise=noise if computed else None, states=states)
            order = others + (['mean', 'scale', 'rotation'] if computed else [])
            new = dict(zip(order, outs))
            rest = outs[len(order):]
            moments, at = {}, 0
            for k in PARAMS:
                if held[k]:
                    moments[k] = (rest[at], rest[at + 1])
                    at += 2
            self._install(optimizer, groups, new, moments)
            return dict(zip(carried, rest[at:]))

    # ---- the operations that change P -------------------------------------------------------------------------------------
    def densify_and_prune(self, screen_size_max, optimizer, generator=None, noise=None):
        """Clone, split and prune in one pass (module docstring), the reference's result row for row.  ``screen_size_max``
        truthy also prunes world-space-large Gaussians, as in the reference.  ``noise`` [split_factor * n_cand, 3]: the
        standard normals of the split samples, row ``c * n_cand + k`` for copy ``c`` of the k-th candidate; drawn with
        ``torch.randn(..., generator=generator)`` when not given (``densify.synchronised_generator`` for replicas).
        Returns the :class:`densify.DensifyPlan`, whose counts say what happened."""
        what = 'SceneGaussian.densify_and_prune'
        self._groups(what, optimizer)
        plan = densify_plan(self.xyz_grad_accum, self.track_cnt, self.scale, self.opacity, self.cam_dist_radius,
                            grad_thr=self.densify_grad_thr, dense_percent=self.dense_percent_thr,
                            opacity_min=self.opacity_min, prune_big=bool(screen_size_max), split_factor=self.split_factor,
                            radius_max=self.radius_max, screen_size_max=screen_size_max,
                            reference_radius_reset=self.reference_radius_reset)
        rows = self.split_factor * plan.n_cand
        device = self.mean.device
        if noise is None:
            noise = torch.randn(rows, 3, generator=generator, device=device, dtype=torch.float32)
        elif tuple(noise.shape) != (rows, 3):
            raise ValueError('%s: noise must be [split_factor * n_cand, 3] = [%d, 3] (it has %s)' % (what, rows,
                                                                                                     tuple(noise.shape)))
        keep_radius = not self.reference_radius_reset
        carried = self._move(what, plan, optimizer, noise, ('radius_max',) if keep_radius else ())
        n = plan.n_out
        self.radius_max = carried['radius_max'] if keep_radius else torch.zeros(n, dtype=torch.float32, device=device)
        self.xyz_grad_accum = torch.zeros(n, 1, dtype=torch.float32, device=device)
        self.track_cnt = torch.zeros(n, 1, dtype=torch.float32, device=device)
        return plan

    def prune_points(self, do_prune, optimizer):
        """Remove the rows where the boolean ``do_prune`` [P] is set: parameters, moments and statistics keep the other
        rows in order (the reference's boolean indexing), through the same move."""
        what = 'SceneGaussian.prune_points'
        self._groups(what, optimizer)
        if isinstance(do_prune, torch.Tensor) and do_prune.dim() == 1 and do_prune.shape[0] != self.mean.shape[0]:
            raise ValueError('%s: do_prune has %d entries for %d points' % (what, do_prune.shape[0], self.mean.shape[0]))
        plan = prune_plan(do_prune)
        carried = self._move(what, plan, optimizer, False, STATS)
        for k in STATS:
            setattr(self, k, carried[k])
        return plan

    def reset_opacity(self, optimizer):
        """Opacities capped at 0.01 and their Adam moments zeroed (reference lines 247-251); torch, once per 3 000
        iterations."""
        what = 'SceneGaussian.reset_opacity'
        groups = self._groups(what, optimizer, ('opacity',))
        with torch.no_grad():
            new = torch.minimum(torch.sigmoid(self.opacity), torch.ones_like(self.opacity) * 0.01)
            new = torch.log(new / (1 - new))
            held = self._moments(what, optimizer, self.opacity)
            moments = {'opacity': (torch.zeros_like(new), torch.zeros_like(new))} if held else {}
            group = groups['opacity']
            old = group['params'][0]
            fresh = nn.Parameter(new.requires_grad_(True))
            state = optimizer.state.pop(old, None)
            if state is not None:
                if moments:
                    state['exp_avg'], state['exp_avg_sq'] = moments['opacity']
                optimizer.state[fresh] = state
            group['params'][0] = fresh
            self.opacity = fresh
