"""Fused densification statistics.

Host-side mirror of what the reference does with the rasterizer's outputs after every backward on the scene
Gaussians: ``avatar/main/train.py:49-54`` stacks ``mean_2d.grad``, ``avatar/main/model.py:279-285`` keeps the
per-Gaussian maximum screen radius, ``avatar/common/nets/module.py:155-157`` (``SceneGaussian.track_stats``)
accumulates ``||grad[:, :2]||`` and a visit count -- three boolean-mask statements per render, each of which
synchronises the host (``nonzero``).  Here it is one streaming HIP kernel on the tensors' own stream, no sync;
in a multi-GPU run the statistics are then combined with ``dist.reduce_densify_stats``.
"""
import torch

from . import _lib
from ._device import _ptr, _stream_ptr, _workspace, check_tensor, launch, need_rocm


def track_densify_stats(mean_2d_grad, radius, xyz_grad_accum=None, track_cnt=None, radius_max=None):
    """In place, for every Gaussian with ``radius > 0`` (the reference's ``is_vis``):
    ``xyz_grad_accum += ||mean_2d_grad[:, :2]||``, ``track_cnt += 1``, ``radius_max = max(radius_max, radius)``.

    ``mean_2d_grad``: float32 [P, 3] (``mean_2d.grad`` of one render); ``radius``: int32 [P] as returned by the
    rasterizer; the three statistics: float32 with P elements ([P] or [P, 1]), any of them may be ``None``.
    """
    lib = _lib.load()
    device = radius.device
    if device.type != 'cuda':
        raise RuntimeError('exavatar_release_amd: track_densify_stats runs on a ROCm device only (no CPU path)')
    P = int(radius.shape[0])
    if radius.dtype != torch.int32 or not radius.is_contiguous():
        raise ValueError('radius must be a contiguous int32 tensor (the rasterizer\'s `radii` output)')
    outs = []
    for name, t in (('xyz_grad_accum', xyz_grad_accum), ('track_cnt', track_cnt), ('radius_max', radius_max)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != P or t.device != device):
            raise ValueError('%s must be a contiguous float32 tensor with %d elements on %s' % (name, P, device))
        outs.append(t)
    g = None
    if xyz_grad_accum is not None:
        if mean_2d_grad is None or tuple(mean_2d_grad.shape) != (P, 3):
            raise ValueError('mean_2d_grad must have shape [%d, 3]' % P)
        g = mean_2d_grad.detach().to(device=device, dtype=torch.float32).contiguous()
    with torch.no_grad(), torch.cuda.device(device):
        _lib.check(lib.exa_raster_densify_stats(P, _ptr(g), _ptr(radius), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]),
                                                _stream_ptr(device)))


# ---- clone / split / prune of a Gaussian set, replicated-safe --------------------------------------------------------
def synchronised_generator(seed, device):
    """A ``torch.Generator`` on ``device`` seeded with ``seed``: created with the same seed on every rank of a
    data-parallel run (and advanced in lockstep: the replicas densify from the same REDUCED statistics), it makes the
    random samples of :func:`densify_and_prune` -- the reference draws them from the global CUDA RNG,
    ``torch.normal`` at ``avatar/common/nets/module.py:198`` -- identical on all ranks, so the topology of the replicated
    Gaussian set never diverges."""
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    return g


def _quat_to_matrix(q):
    q = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)
    w, x, y, z = q.unbind(1)
    return torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), 1).view(-1, 3, 3)


def densify_and_prune(params, optimizer, grad_accum, track_cnt, *, grad_thr, extent, dense_percent=0.01, opacity_min=0.005,
                      prune_big=False, split_factor=2, generator=None, rotation_to_matrix=None, radius_max=None,
                      screen_size_max=None, reference_radius_reset=True):
    """Clone / split / prune one set of Gaussians and carry the optimizer state along -- what the reference's
    ``SceneGaussian.densify_and_prune`` does with its Adam-state surgery (``avatar/common/nets/module.py:17-72,159-240``),
    restated for a plain dict of parameters and any ``torch.optim`` optimizer with per-parameter state tensors.

    ``params``: dict name -> ``nn.Parameter`` with first dimension P; needs ``'mean'`` [P, 3], ``'scale'`` [P, 3] (LOG
    scales, activation ``exp``), ``'rotation'`` ([P, 4] quaternion w, x, y, z -- or give ``rotation_to_matrix``) and
    ``'opacity'`` [P, 1] (logits, activation ``sigmoid``); every other entry (colours, SH) is carried along.  Each
    parameter must be the single member of an optimizer group.  ``grad_accum`` / ``track_cnt``: the statistics of
    :func:`track_densify_stats` (already reduced over the ranks: ``dist.reduce_densify_stats``).

    Order of events as in the reference: mean screen-space gradient ``>= grad_thr`` selects; small ones (max scale
    ``<= dense_percent * extent``) are CLONED, large ones SPLIT into ``split_factor`` samples of their own Gaussian (scale
    divided by ``0.8 * split_factor``) and removed; then everything with opacity ``< opacity_min`` (and, with
    ``prune_big``, max scale ``> 0.1 * extent``) is pruned.  Row order of the result: surviving originals, clones,
    split samples.  New rows start with zero optimizer state.  ``generator``: see :func:`synchronised_generator`.

    Screen-space prune (``prune_big`` with ``radius_max`` [P] and ``screen_size_max``; the reference passes 20 px once
    ``cur_itr > opacity_reset_interval``, ``avatar/main/model.py:288-289``): the reference tests ``self.radius_max >
    screen_size_max`` AFTER ``clone_points`` / ``split_points``, whose ``densify()`` has just replaced ``radius_max`` by zeros
    for EVERY row (module.py:223) -- the test can never fire there.  ``reference_radius_reset=True`` (default) reproduces
    that (topology identical to the reference's); ``False`` applies the criterion the code evidently intends (upstream
    3DGS): surviving originals keep their ``radius_max``, new rows start at zero.

    Returns ``(new_params, n_cloned, n_split, n_pruned)``; the caller allocates fresh statistics of the new length (the
    reference zeroes them in ``densify``, module.py:223-225)."""
    mean, scale, rot, opac = params['mean'], params['scale'], params['rotation'], params['opacity']
    P0 = mean.shape[0]
    with torch.no_grad():
        g = torch.nan_to_num(grad_accum.reshape(-1) / track_cnt.reshape(-1))
        big = torch.exp(scale).max(1).values > dense_percent * extent
        hot = g >= grad_thr
        clone_rows = torch.nonzero(hot & ~big).flatten()
        split_rows = torch.nonzero(hot & big).flatten()
        keep_rows = torch.nonzero(~(hot & big)).flatten()
        rep = split_rows.repeat(split_factor)
        std = torch.exp(scale[rep])
        noise = torch.randn(std.shape, generator=generator, device=std.device, dtype=std.dtype) * std
        R = (rotation_to_matrix or _quat_to_matrix)(rot[rep])
        new = {}
        for name, p in params.items():
            parts = [p[keep_rows], p[clone_rows]]
            if name == 'mean':
                parts.append(torch.bmm(R, noise[:, :, None])[:, :, 0] + p[rep])
            elif name == 'scale':
                parts.append(torch.log(torch.exp(p[rep]) / (0.8 * split_factor)))
            else:
                parts.append(p[rep])
            new[name] = torch.cat(parts)
        # rows of the ORIGINAL set each new row descends from with its optimizer state (-1: a new row, zero state)
        src = torch.cat((keep_rows, torch.full((clone_rows.numel() + rep.numel(),), -1, dtype=torch.long, device=keep_rows.device)))
        drop = torch.sigmoid(new['opacity'])[:, 0] < opacity_min
        if prune_big:
            drop |= torch.exp(new['scale']).max(1).values > 0.1 * extent
            if radius_max is not None and screen_size_max and not reference_radius_reset:
                r_new = torch.zeros(src.numel(), dtype=torch.float32, device=src.device)
                r_new[:keep_rows.numel()] = radius_max.reshape(-1).to(torch.float32)[keep_rows]
                drop |= r_new > float(screen_size_max)
        valid = ~drop
        src = src[valid]
        out = {}
        for group in optimizer.param_groups:
            if len(group['params']) != 1:
                continue
            old = group['params'][0]
            name = next((n for n, p in params.items() if p is old), None)
            if name is None:
                continue
            fresh = torch.nn.Parameter(new[name][valid].contiguous().requires_grad_(True))
            state = optimizer.state.pop(old, None)
            if state is not None:
                for k, v in list(state.items()):
                    if isinstance(v, torch.Tensor) and v.dim() > 0 and v.shape[0] == P0:
                        nv = torch.zeros((src.numel(),) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)
                        old_rows = src >= 0
                        nv[old_rows] = v[src[old_rows]]
                        state[k] = nv
                optimizer.state[fresh] = state
            group['params'][0] = fresh
            out[name] = fresh
        missing = [n for n in params if n not in out]
        if missing:
            raise ValueError('densify_and_prune: parameters %s are not single members of an optimizer group' % missing)
    return out, int(clone_rows.numel()), int(split_rows.numel()), int(drop.sum())


# ---- clone / split / prune in one pass over the source rows (csrc/densify.hip) ----------------------------------------
BLOCK = _lib.DENSIFY_BLOCK                # source rows per workgroup of the classification and of the move
SCAN_WIDTH = _lib.DENSIFY_SCAN            # count records per round of the one-workgroup scan
MAX_SEGMENTS = _lib.DENSIFY_MAX_SEGMENTS  # tensors per launch of the move
COPY, STATE, MEAN, SCALE = _lib.DENSIFY_COPY, _lib.DENSIFY_STATE, _lib.DENSIFY_MEAN, _lib.DENSIFY_SCALE


def workspace_size(P0):
    """Bytes of a plan's workspace (``exa_raster_densify_workspace_size``): the 16-byte record, 16 bytes of offsets per
    block of ``BLOCK`` rows and one code byte per row, the codes padded to 16."""
    return _lib.densify_workspace_size(int(P0))


class DensifyPlan:
    """The decisions of one densification over ``P0`` source rows: ``workspace`` (the device's codes and offsets, for
    :func:`densify_apply`) and the four totals read back from it -- ``n_keep`` surviving originals, ``n_clone`` surviving
    clones, ``n_split`` surviving split rows (``split_factor`` children each), ``n_cand`` split candidates (the rows the
    reference draws noise for) -- with ``n_out = n_keep + n_clone + split_factor * n_split``."""

    def __init__(self, workspace, P0, split_factor, totals, device):
        self.workspace, self.P0, self.split_factor, self.device = workspace, int(P0), int(split_factor), device
        self.n_keep, self.n_clone, self.n_split, self.n_cand = (int(x) for x in totals)

    @property
    def n_out(self):
        return self.n_keep + self.n_clone + self.split_factor * self.n_split

    def __repr__(self):
        return 'DensifyPlan(P0=%d, n_keep=%d, n_clone=%d, n_split=%d, n_cand=%d, split_factor=%d)' % (
            self.P0, self.n_keep, self.n_clone, self.n_split, self.n_cand, self.split_factor)


def _read_plan(ws, P0, split_factor, device):
    """The one read-back of a plan: the 16-byte record, after the one synchronisation of the stream."""
    if P0 == 0:
        return DensifyPlan(ws, 0, split_factor, (0, 0, 0, 0), device)
    totals = ws[:16].view(torch.int32).cpu().tolist()        # a blocking copy on the current stream: the sync
    return DensifyPlan(ws, P0, split_factor, totals, device)


def _rows(what, name, x, P0, tail=None):
    """``x`` as a detached contiguous float32 tensor of ``P0`` rows (of ``tail`` elements when given); the device is
    checked afterwards, by :func:`_same_device`, so that a wrong dtype or shape is named first."""
    check_tensor(what, name, x)
    if x.dim() < 1 or x.shape[0] != P0 or (tail is not None and x.numel() != P0 * tail):
        raise ValueError('%s: %s must hold %d rows%s (it has shape %s)' % (
            what, name, P0, '' if tail is None else ' of %d' % tail, tuple(x.shape)))
    return x.detach().contiguous()


def _same_device(what, named, anchor):
    for name, x in named:
        if x is not None:
            check_tensor(what, name, x, f32=False, rocm=True, on=anchor)


def densify_plan(grad_accum, track_cnt, scale, opacity, extent, *, grad_thr, dense_percent=0.01, opacity_min=0.005,
                 prune_big=False, split_factor=2, radius_max=None, screen_size_max=None, reference_radius_reset=True):
    """Classify every row of a Gaussian set for clone / split / prune in one launch and return the :class:`DensifyPlan`.

    ``grad_accum`` / ``track_cnt``: the statistics of :func:`track_densify_stats`, float32 with P0 elements; ``scale``
    [P0, 3] (logs), ``opacity`` [P0, 1] or [P0] (logits); ``extent``: a float32 DEVICE tensor with one element (the
    reference's ``cam_dist_radius``; the host never reads it).  The decision table is the reference's three passes
    restated per source row (``include/exa_raster.h``); ``prune_big`` is the reference's truthy ``screen_size_max``.
    ``radius_max`` [P0] with ``screen_size_max`` and ``reference_radius_reset=False`` also drops originals with
    ``radius_max > screen_size_max`` (see :func:`densify_and_prune`); the default reproduces the reference.

    Does the one read-back of the 16-byte record and the one stream synchronisation of a densification."""
    what = 'densify_plan'
    check_tensor(what, 'scale', scale)
    if scale.dim() != 2 or scale.shape[1] != 3:
        raise ValueError('%s: scale must be [P, 3] (it has %s)' % (what, tuple(scale.shape)))
    P0 = scale.shape[0]
    anchor = (scale, 'scale')
    scale = _rows(what, 'scale', scale, P0, 3)
    grad_accum = _rows(what, 'grad_accum', grad_accum, P0, 1)
    track_cnt = _rows(what, 'track_cnt', track_cnt, P0, 1)
    opacity = _rows(what, 'opacity', opacity, P0, 1)
    check_tensor(what, 'extent', extent)
    if extent.numel() != 1:
        raise ValueError('%s: extent must be a device tensor with one element (it has shape %s)' % (what, tuple(extent.shape)))
    extent = extent.detach().contiguous()
    split_factor = int(split_factor)
    if not 1 <= split_factor <= 8:
        raise ValueError('%s: split_factor must be in 1 .. 8 (it is %d)' % (what, split_factor))
    radius = None
    if prune_big and radius_max is not None and screen_size_max and not reference_radius_reset:
        radius = _rows(what, 'radius_max', radius_max, P0, 1)
    _same_device(what, (('scale', scale), ('grad_accum', grad_accum), ('track_cnt', track_cnt), ('opacity', opacity),
                        ('extent', extent), ('radius_max', radius)), anchor)
    device = scale.device
    ws = _workspace(workspace_size(P0), device)
    launch(_lib.RASTER, 'exa_raster_densify_plan', device, P0, _ptr(grad_accum), _ptr(track_cnt), _ptr(scale),
           _ptr(opacity), _ptr(radius), _ptr(extent), None, float(grad_thr), float(dense_percent), float(opacity_min),
           int(bool(prune_big)), split_factor, float(screen_size_max or 0.0), _ptr(ws), ws.numel())
    return _read_plan(ws, P0, split_factor, device)


def prune_plan(do_prune):
    """The plan that removes the rows where the boolean device tensor ``do_prune`` [P0] is set and keeps the others in
    order -- the reference's ``prune_points`` -- for the same :func:`densify_apply`."""
    what = 'prune_plan'
    if not isinstance(do_prune, torch.Tensor):
        raise TypeError('%s: do_prune must be a tensor' % what)
    need_rocm(do_prune.device, what)
    if do_prune.dtype != torch.bool or do_prune.dim() != 1:
        raise ValueError('%s: do_prune must be a boolean [P] tensor (it is %s %s)' % (what, do_prune.dtype,
                                                                                     tuple(do_prune.shape)))
    mask = do_prune.contiguous()
    P0, device = mask.shape[0], mask.device
    ws = _workspace(workspace_size(P0), device)
    launch(_lib.RASTER, 'exa_raster_densify_plan', device, P0, None, None, None, None, None, None, _ptr(mask), 0.0, 0.0,
           0.0, 0, 1, 0.0, _ptr(ws), ws.numel())
    return _read_plan(ws, P0, 1, device)


def densify_apply(plan, tensors, *, mean=None, scale=None, rotation=None, noise=None, states=()):
    """Carry out ``plan`` on every tensor given, in one launch per 64 of them, and return the new tensors in the order
    given: ``[*tensors, mean, scale, rotation, *states]`` (without the ones that are ``None``), each ``[plan.n_out, ...]``
    with every element written.

    Every tensor is float32 with ``plan.P0`` rows of any width >= 1.  ``tensors`` are copied row by row (the clones and
    the children are their source's rows); ``states`` (optimizer moments, statistics) keep the rows of surviving originals
    and are ``+0.0`` in every new row; ``mean`` [P0, 3] and ``scale`` [P0, 3] are computed for split children
    (``include/exa_raster.h``); ``rotation`` [P0, 6] is copied and is the children's rotation source.  ``noise``
    [split_factor * plan.n_cand, 3]: standard normals, row ``c * n_cand + k`` for copy ``c`` of the k-th split candidate
    (the reference's draw order); needed when ``mean`` is given and the plan has candidates.  No synchronisation."""
    what = 'densify_apply'
    if not isinstance(plan, DensifyPlan):
        raise TypeError('%s: plan must be a DensifyPlan' % what)
    P0, n_out = plan.P0, plan.n_out
    named = [('tensors[%d]' % i, t, COPY) for i, t in enumerate(tensors)]
    named += [(n, t, r) for n, t, r in (('mean', mean, MEAN), ('scale', scale, SCALE), ('rotation', rotation, COPY))
              if t is not None]
    named += [('states[%d]' % i, t, STATE) for i, t in enumerate(states)]
    ws = plan.workspace
    anchor = (ws, "the plan's workspace")
    srcs = []
    for name, t, role in named:
        tail = {'mean': 3, 'scale': 3, 'rotation': 6}.get(name)
        srcs.append(_rows(what, name, t, P0, tail))
        if P0 and srcs[-1].numel() == 0:
            raise ValueError('%s: %s has rows of no elements' % (what, name))
    if mean is not None and (scale is None or rotation is None):
        raise ValueError('%s: mean needs scale and rotation (the children are samples of their source)' % what)
    z = None
    if mean is not None and plan.n_cand:
        if noise is None:
            raise ValueError('%s: the plan has %d split candidates: noise [%d, 3] is needed' % (
                what, plan.n_cand, plan.split_factor * plan.n_cand))
        check_tensor(what, 'noise', noise)
        if tuple(noise.shape) != (plan.split_factor * plan.n_cand, 3):
            raise ValueError('%s: noise must be [split_factor * n_cand, 3] = [%d, 3] (it has %s)' % (
                what, plan.split_factor * plan.n_cand, tuple(noise.shape)))
        z = noise.detach().contiguous()
    _same_device(what, [(n, t) for (n, _, _), t in zip(named, srcs)] + [('noise', z)], anchor)
    outs = [torch.empty((n_out,) + tuple(t.shape[1:]), dtype=torch.float32, device=plan.device) for _, t, _ in named]
    if P0 == 0 or not named:
        return outs
    segs = [_lib.ExaRasterDensifySegment(s.data_ptr(), d.data_ptr() if n_out else None, s.numel() // P0, n_out, role, 0)
            for s, d, (_, _, role) in zip(srcs, outs, named)]
    by_name = {n: s for (n, _, _), s in zip(named, srcs)}
    launch(_lib.RASTER, 'exa_raster_densify_move', plan.device, P0, plan.split_factor, _ptr(ws), ws.numel(), plan.n_keep,
           plan.n_clone, plan.n_split, plan.n_cand, (_lib.ExaRasterDensifySegment * len(segs))(*segs), len(segs),
           _ptr(by_name.get('rotation')), _ptr(by_name.get('scale')), _ptr(z))
    return outs
