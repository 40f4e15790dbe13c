"""The Adam step of include/exa_raster.h (exa_raster_adam_step) restated in numpy float32, operation by operation, every
intermediate rounded to float32, with the host-double scalars the library's callers form -- what csrc/adam.hip must equal
bit for bit -- and the small copy of the reference's parameter grouping that the CPU and the GPU tests step through."""
import math

import numpy as np
import torch

F = np.float32


def scalars(t, lr, beta1, beta2):
    """``(step_size, bc2_sqrt)`` of update ``t`` (1 for the first): formed in double, rounded once to float32."""
    return F(lr / (1.0 - beta1 ** t)), F(math.sqrt(1.0 - beta2 ** t))


def step(p, g, m, v, *, t, lr, betas=(0.9, 0.999), eps=1e-8):
    """New ``(p, m, v)`` of float32 arrays ``p, g, m, v`` (the inputs stay as they are)."""
    assert p.dtype == g.dtype == m.dtype == v.dtype == np.float32
    beta1, beta2 = betas
    w1, b2, w2, e = F(1.0 - beta1), F(beta2), F(1.0 - beta2), F(eps)
    step_size, bc2_sqrt = scalars(t, lr, beta1, beta2)
    d0 = g - m
    m2 = m + w1 * d0 if w1 < F(0.5) else g - d0 * (F(1.0) - w1)
    v2 = v * b2 + (w2 * g) * g
    d = np.sqrt(v2) / bc2_sqrt + e
    p2 = p + (-step_size) * (m2 / d)
    for a in (m2, v2, d, p2):
        assert a.dtype == np.float32
    return p2, m2, v2


# ---- a small copy of the reference's grouping: every tensor the only member of its own group (module.py:141-150, 666-671)
SCENE = {'mean': (3,), 'feature_dc': (1, 3), 'feature_rest': (15, 3), 'opacity': (1,), 'scale': (3,), 'rotation': (6,)}
FRAME = {'root_pose': (6,), 'body_pose': (21, 6), 'jaw_pose': (6,), 'leye_pose': (6,), 'reye_pose': (6,),
         'lhand_pose': (15, 6), 'rhand_pose': (15, 6), 'expr': (50,), 'trans': (3,)}
P = 301                   # scene Gaussians: odd, feature_rest is more than one chunk of 4096 elements
STEPS = 5
EPS = 1e-15               # the reference's (base.py:85)
IDLE_FRAME = 1            # its nine tensors never get a gradient


def grouping_case():
    """``(init, lrs, grads)``: name -> float32 array; name -> learning rate; one dict name -> float32 gradient per step
    (without the idle frame's names).  The order of ``init`` is the order of the groups."""
    rs = np.random.RandomState(811)
    init, lrs = {}, {}
    for i, (n, s) in enumerate(SCENE.items()):
        init[n] = rs.randn(P, *s).astype(F)
        lrs[n] = (1.6e-4, 2.5e-3, 1.25e-4, 5e-2, 5e-3, 1e-3)[i]
    for f in range(2):
        for n, s in FRAME.items():
            init['smplx_%s_%d' % (n, f)] = (0.3 * rs.randn(*s)).astype(F)
            lrs['smplx_%s_%d' % (n, f)] = 1e-3
    live = [n for n in init if not n.endswith('_%d' % IDLE_FRAME)]
    grads = [{n: (rs.randn(*init[n].shape) * 10.0 ** rs.uniform(-4, 0)).astype(F) for n in live} for _ in range(STEPS)]
    return init, lrs, grads


def make_optimizer(cls, init, lrs, dtype, device):
    """``(params, optimizer)`` of ``cls`` over the case, constructed as the reference does (lr = 0.0 overridden per group)."""
    params = {n: torch.nn.Parameter(torch.from_numpy(a.copy()).to(device=device, dtype=dtype)) for n, a in init.items()}
    opt = cls([{'params': [p], 'name': n, 'lr': lrs[n]} for n, p in params.items()], lr=0.0, eps=EPS)
    return params, opt


def run(opt, params, grads, dtype):
    """Step ``opt`` through ``grads``; a parameter without an entry has ``.grad = None``."""
    for step_grads in grads:
        for n, p in params.items():
            g = step_grads.get(n)
            p.grad = None if g is None else torch.from_numpy(g).to(device=p.device, dtype=dtype)
        opt.step()


def oracle_run(init, lrs, grads, first_step=1, state=None):
    """The oracle through ``grads``: ``(params, state)`` with state name -> (m, v, t)."""
    params = {n: a.copy() for n, a in init.items()}
    state = dict(state or {})
    for step_grads in grads:
        for n, g in step_grads.items():
            m, v, t = state.get(n, (np.zeros_like(params[n]), np.zeros_like(params[n]), first_step - 1))
            params[n], m, v = step(params[n], g, m, v, t=t + 1, lr=lrs[n], eps=EPS)
            state[n] = (m, v, t + 1)
    return params, state


def max_err(a, ref64):
    return float(np.abs(np.asarray(a, np.float64) - ref64).max())
