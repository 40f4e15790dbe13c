"""Float64 restatement of the per-pixel blend (oracle/raster_oracle.py steps 9/10) that takes its discrete decisions from
the CALLER instead of deriving them.

THIS IS TEST INFRASTRUCTURE, like tests/mesh_oracle.py.  Every parity test against oracle/raster_oracle.py compares two
implementations that each take their own decisions (alpha < 1/255, power > 0, T (1 - alpha) < 1e-4), so pixels near a
threshold are masked out and Gaussians near them get a loose floor.  A backward pass that disagrees with its OWN forward
exactly at such a pair is excused by construction.  Here the decisions are inputs:

  * ``visible``  bool [P]:  the Gaussians that take part (the HIP ``radius > 0``); the others get exactly zero gradient;
  * ``order``    long [Pv]: the blend order (default: float32 view depth, ties by index -- what the sort produces);
  * ``keep``     bool [P, H, W]: pair (i, pixel) is blended (``w > 0`` as read from the HIP forward: tests/helpers.py
    ``extract_weights``).

Everything continuous is ``raster_oracle.preprocess`` in float64 (projection, covariance, conic, ``mean_2d`` holder,
straight-through ``min(0.99, .)``), differentiated by autograd.  One decision is still taken inside: the +-1.3 tanfov
clamp of the EWA Jacobian (upstream's ``x_grad_mul``) is decided in float64 by ``preprocess``.

"""
import torch

from oracle import raster_oracle as ro

KEYS = ('mean_3d', 'scale', 'rotation', 'opacity', 'rgb')


def blend_order(assets, img_shape, cam, visible, sh_degree=0):
    """Indices of the visible Gaussians in the order of the HIP sort: float32 view depth (the float32 preprocess is
    bit-identical to the kernel's), ties by index."""
    s = ro.settings_from_camera(cam, img_shape, torch.zeros(3), sh_degree)
    with torch.no_grad():
        pre = ro.preprocess(assets['mean_3d'].detach().float(), None, None, assets['scale'].detach().float(),
                            assets['rotation'].detach().float(), None, s, torch.float32)
    idx = torch.nonzero(visible, as_tuple=False).flatten()
    o = torch.argsort(pre['depth'][idx], stable=True)
    return idx[o]


def render(assets, img_shape, cam, bg, keep, visible, order=None, sh=None, sh_degree=0):
    """Float64 render of ``assets`` (the keys of ``GaussianRenderer``; ``sh`` [P, M, 3] replaces ``rgb`` when given) with
    the caller's decisions.  Leaf tensors of ``assets`` / ``sh`` that require grad receive float64 gradients.
    Returns {img [3,H,W], depthmap [1,H,W], mask [1,H,W], w [P,H,W] (detached), mean_2d (leaf [P,3])}."""
    H, W = int(img_shape[0]), int(img_shape[1])
    P = assets['mean_3d'].shape[0]
    dt = torch.float64
    s = ro.settings_from_camera(cam, (H, W), bg, sh_degree)
    mean_2d = torch.zeros(P, 3, dtype=dt, requires_grad=True)
    holder = [visible.bool()]
    # culled Gaussians get exactly zero gradients, also where their float64 forward is not finite (raster_oracle)
    wrap = lambda t: ro._ZeroGradOfCulled.apply(t, holder) if (t is not None and t.requires_grad) else t     # noqa: E731
    m3, m2, op, sc, rot = (wrap(assets['mean_3d']), wrap(mean_2d), wrap(assets['opacity']), wrap(assets['scale']),
                           wrap(assets['rotation']))
    pre = ro.preprocess(m3, m2, op, sc, rot, None, s, dt)
    if sh is not None:
        colors = ro.eval_sh_color(int(sh_degree), wrap(sh).to(dt), m3.to(dt), s.campos.to(dt))
    else:
        colors = wrap(assets['rgb']).to(dt)
    if order is None:
        order = blend_order(assets, (H, W), cam, visible, sh_degree)
    keep = keep.bool()
    bgd = bg.to(dt)
    img = bgd.view(3, 1, 1).expand(3, H, W).clone()
    depth = torch.zeros(H, W, dtype=dt)
    mask = torch.zeros(H, W, dtype=dt)
    w_full = torch.zeros(P, H, W, dtype=dt)
    opd = op.to(dt).view(-1)
    px, py, conic, z = pre['px'], pre['py'], pre['conic'], pre['depth']
    # per 16 x 16 tile like raster_oracle (the same arithmetic per pixel and the same gradient accumulation: the
    # needles' gradients are sums of large cancelling terms), over the entries the tile's pixels take
    T = ro.TILE
    for ya in range(0, H, T):
        for xa in range(0, W, T):
            yb, xb = min(ya + T, H), min(xa + T, W)
            kt = keep[order, ya:yb, xa:xb].flatten(1)
            ids = order[kt.any(1)]
            if ids.numel() == 0:
                continue
            X = torch.arange(xa, xb, dtype=dt).repeat(yb - ya)
            Y = torch.arange(ya, yb, dtype=dt).repeat_interleave(xb - xa)
            dx = px[ids][:, None] - X[None, :]
            dy = py[ids][:, None] - Y[None, :]
            cn = conic[ids]
            power = -0.5 * (cn[:, 0:1] * dx * dx + cn[:, 2:3] * dy * dy) - cn[:, 1:2] * dx * dy
            a_raw = opd[ids][:, None] * torch.exp(power)
            a = a_raw + (a_raw.clamp(max=ro.ALPHA_MAX) - a_raw).detach()     # straight-through min(0.99, .)
            a_k = torch.where(kt[kt.any(1)], a, torch.zeros_like(a))
            T_in = torch.cumprod(1 - a_k, 0)
            T_ex = torch.cat((torch.ones(1, T_in.shape[1], dtype=dt), T_in[:-1]), 0)
            wgt = a_k * T_ex                                                  # [n, npix]
            Tf = T_in[-1]
            hh, ww = yb - ya, xb - xa
            img[:, ya:yb, xa:xb] = (wgt.t() @ colors[ids] + Tf[:, None] * bgd[None, :]).t().reshape(3, hh, ww)
            depth[ya:yb, xa:xb] = (wgt.t() @ z[ids]).reshape(hh, ww)
            mask[ya:yb, xa:xb] = (1 - Tf).reshape(hh, ww)
            w_full[ids, ya:yb, xa:xb] = wgt.detach().reshape(-1, hh, ww)
    return {'img': img, 'depthmap': depth[None], 'mask': mask[None], 'w': w_full, 'mean_2d': mean_2d}
