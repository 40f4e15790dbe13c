"""HIP fused MLP: a drop-in for ExAvatar's ``make_linear_layers(..., use_gn=True)`` trunks and their linear heads.

* ``FusedMLP(trunk, heads=None)`` -- reference ``avatar/common/nets/layer.py:9-20`` built at
  ``avatar/common/nets/module.py:279-287`` and called at ``module.py:459-509, 524-528``: L trunk layers
  ``Linear -> GroupNorm -> ReLU`` (128 wide) and 1-4 plain ``Linear`` heads, in one HIP launch forward and three
  backward.  ``FusedMLP(geo_net, heads=(mean_offset_net, scale_net))(tri_feat)`` returns ``(mean_offset, scale)``;
  ``FusedMLP(rgb_net)(tri_feat)`` (a trailing Linear in the Sequential is the one head) returns ``rgb``.

The call takes column blocks whose concatenation, in order, is the first layer's input.  A block ``[N, c]`` is per row
and gets a gradient when it requires one.  A block ``[c]`` (or ``[1, c]`` when N > 1) is shared by every row and is
folded into the first layer's bias once per call; it gets no gradient (the reference detaches it), so one that requires
grad is refused.  The modules' own Parameters are used in place (no copies, nothing registered): the caller's optimizer
groups and state_dict are unchanged, and every Parameter gets its gradient through autograd.

The kernels are ``csrc/mlp.hip`` behind ``include/exa_mlp.h``; ROCm device tensors only, no CPU path.  The CPU
restatement that pins them is ``tests/mlp_oracle.py``.  The forward saves nothing beyond its inputs (the backward
recomputes it); the backward's workspace comes from the torch allocator (``config.poison`` fills it with 0xFF).  No call
synchronises the device, so forward and backward can be captured into a hipGraph.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from ._device import _addr, _ptrs, _workspace, check_tensor, grad_in, launch
from ._lib import ExaMlpNet

HIDDEN = 128              # EXA_MLP_HIDDEN
MAX_LAYERS = 4            # EXA_MLP_MAX_LAYERS
MAX_IN = 256              # EXA_MLP_MAX_IN
MAX_SHARED = 1024         # EXA_MLP_MAX_SHARED
MAX_HEADS = 4             # EXA_MLP_MAX_HEADS
MAX_OUT = 32              # EXA_MLP_MAX_OUT
CHUNK = 512               # EXA_MLP_CHUNK
GROUPS = (1, 2, 4)


def parse_structure(trunk, heads=None):
    """Check a ``make_linear_layers(..., use_gn=True)`` Sequential (and heads) against what the kernels support.
    Returns ``(layers, heads)``: a list of (Linear, GroupNorm) pairs and a tuple of head Linears.  Anything else raises
    ValueError naming the offending layer.  Pure Python: runs without a GPU."""
    if not isinstance(trunk, nn.Sequential):
        raise ValueError('FusedMLP: the trunk must be an nn.Sequential (it is %s)' % type(trunk).__name__)
    mods = list(trunk)
    layers, i = [], 0
    while i + 1 < len(mods) and isinstance(mods[i], nn.Linear) and isinstance(mods[i + 1], nn.GroupNorm):
        lin, gn = mods[i], mods[i + 1]
        if i + 2 >= len(mods) or not isinstance(mods[i + 2], nn.ReLU):
            raise ValueError('FusedMLP: layer %d of the trunk must be ReLU after Linear -> GroupNorm' % (i + 2))
        layers.append((lin, gn, i))
        i += 3
    rest = mods[i:]
    trailing = ()
    if len(rest) == 1 and isinstance(rest[0], nn.Linear):
        trailing = (rest[0],)
    elif rest:
        raise ValueError('FusedMLP: layer %d of the trunk (%s) is not part of a Linear -> GroupNorm -> ReLU block or a '
                         'trailing Linear' % (i, type(rest[0]).__name__))
    if not layers:
        raise ValueError('FusedMLP: the trunk needs at least one Linear -> GroupNorm -> ReLU layer')
    if len(layers) > MAX_LAYERS:
        raise ValueError('FusedMLP: at most %d trunk layers (got %d)' % (MAX_LAYERS, len(layers)))
    for n, (lin, gn, at) in enumerate(layers):
        if lin.bias is None:
            raise ValueError('FusedMLP: layer %d (Linear) has no bias' % at)
        if lin.out_features != HIDDEN:
            raise ValueError('FusedMLP: layer %d (Linear) is %d wide; only %d is supported' % (at, lin.out_features, HIDDEN))
        if n == 0 and not 1 <= lin.in_features <= MAX_IN + MAX_SHARED:
            raise ValueError('FusedMLP: layer %d (Linear) has %d inputs' % (at, lin.in_features))
        if n > 0 and lin.in_features != HIDDEN:
            raise ValueError('FusedMLP: layer %d (Linear) has %d inputs; only %d is supported'
                             % (at, lin.in_features, HIDDEN))
        if gn.num_channels != HIDDEN or gn.num_groups not in GROUPS:
            raise ValueError('FusedMLP: layer %d (GroupNorm) must have %d channels in 1, 2 or 4 groups (it has %d in %d)'
                             % (at + 1, HIDDEN, gn.num_channels, gn.num_groups))
        if not gn.affine:
            raise ValueError('FusedMLP: layer %d (GroupNorm) must be affine' % (at + 1))
        if gn.num_groups != layers[0][1].num_groups:     # the kernels take one group count for the whole trunk
            raise ValueError('FusedMLP: layer %d (GroupNorm) has %d groups; every GroupNorm of the trunk must have as '
                             'many as the first (%d)' % (at + 1, gn.num_groups, layers[0][1].num_groups))
    if trailing and heads:
        raise ValueError('FusedMLP: the trunk ends in a Linear and heads= is given as well')
    hs = trailing if trailing else tuple(heads or ())
    # make_linear_layers([128, n], relu_final=False) is a Sequential holding one Linear: take the Linear
    hs = tuple(hd[0] if isinstance(hd, nn.Sequential) and len(hd) == 1 else hd for hd in hs)
    if not 1 <= len(hs) <= MAX_HEADS:
        raise ValueError('FusedMLP: 1 .. %d heads (got %d)' % (MAX_HEADS, len(hs)))
    for k, hd in enumerate(hs):
        if not isinstance(hd, nn.Linear):
            raise ValueError('FusedMLP: head %d is %s, not a plain Linear' % (k, type(hd).__name__))
        if hd.in_features != HIDDEN or hd.bias is None:
            raise ValueError('FusedMLP: head %d must be Linear(%d, n) with a bias' % (k, HIDDEN))
    if sum(hd.out_features for hd in hs) > MAX_OUT:
        raise ValueError('FusedMLP: the heads are %d wide in total; at most %d' % (sum(h.out_features for h in hs), MAX_OUT))
    return [(lin, gn) for lin, gn, _ in layers], hs


def _net(layers, hs, K0, S, W0, Ws, p, Wh, bh, trunk):
    n = ExaMlpNet()
    n.n_layers, n.in_width, n.shared_width = len(layers), K0, S
    n.groups = layers[0][1].num_groups
    n.n_heads = len(hs)
    for k, hd in enumerate(hs):
        n.head_width[k] = hd.out_features
    n.ld_w0 = W0.stride(0)
    n.ld_ws = Ws.stride(0) if Ws is not None else 0
    for l, (lin, gn) in enumerate(layers):
        n.eps[l] = gn.eps
        b, g, be = trunk[4 * l + 0], trunk[4 * l + 1], trunk[4 * l + 2]
        n.W[l] = W0.data_ptr() if l == 0 else trunk[4 * l - 1].data_ptr()
        n.b[l], n.gamma[l], n.beta[l] = b.data_ptr(), g.data_ptr(), be.data_ptr()
    n.Ws = Ws.data_ptr() if Ws is not None else None
    n.shared = p.data_ptr() if p is not None else None
    n.Wh, n.bh = Wh.data_ptr(), bh.data_ptr()
    return n


class _MLP(torch.autograd.Function):
    """x [N, K0], p [S] or None, W0 [128, K0] (row stride >= K0), Ws [128, S] or None, Wh [nh, 128], bh [nh], then per
    layer l: b_l, gamma_l, beta_l and (l >= 1) W_l  ->  one [N, w_k] tensor per head."""

    @staticmethod
    def forward(ctx, meta, x, p, W0, Ws, Wh, bh, *trunk):
        layers, hs = meta
        N, K0 = x.shape
        S = 0 if p is None else p.shape[0]
        dev = x.device
        net = _net(layers, hs, K0, S, W0, Ws, p, Wh, bh, trunk)
        outs = [torch.empty((N, hd.out_features), dtype=torch.float32, device=dev) for hd in hs]
        launch(_lib.MLP, 'exa_mlp_forward', dev, ctypes.byref(net), N, x.data_ptr() if N else None, _ptrs(outs))
        ctx.meta = meta
        ctx.save_for_backward(x, p, W0, Ws, Wh, bh, *trunk)      # (p and Ws are None together: saved as None)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        x, p, W0, Ws, Wh, bh, *trunk = ctx.saved_tensors
        layers, hs = ctx.meta
        N, K0 = x.shape
        S = 0 if p is None else p.shape[0]
        dev = x.device
        need = ctx.needs_input_grad
        net = _net(layers, hs, K0, S, W0, Ws, p, Wh, bh, trunk)
        gouts = [grad_in(g) for g in grads]
        gx = torch.empty((N, K0), dtype=torch.float32, device=dev) if need[1] else None
        want_params = need[3] or need[5] or need[6] or any(need[7:])
        count = ctypes.c_int64()
        _lib.MLP.check(_lib.load().exa_mlp_param_count(ctypes.byref(net), ctypes.byref(count)))
        gp = torch.empty(int(count.value), dtype=torch.float32, device=dev) if want_params else None
        gws = torch.empty((HIDDEN, S), dtype=torch.float32, device=dev) if (S and need[4]) else None
        nbytes = _lib.size_query(_lib.MLP, 'exa_mlp_workspace_size', ctypes.byref(net), N)
        ws = _workspace(nbytes, dev) if nbytes and (gx is not None or gp is not None or gws is not None) else None
        if gx is not None or gp is not None or gws is not None:
            launch(_lib.MLP, 'exa_mlp_backward', dev, ctypes.byref(net), N, x.data_ptr() if N else None, _ptrs(gouts),
                   _addr(gx) if N else None, _addr(gp), _addr(gws), _addr(ws), nbytes)
        g_trunk = [None] * len(trunk)
        gW0 = gWh = gbh = None
        if gp is not None:
            off, H = 0, HIDDEN
            for l in range(len(layers)):
                K = K0 if l == 0 else H
                gW = gp[off:off + H * K].view(H, K)
                off += H * K
                gb, gg, gbe = gp[off:off + H], gp[off + H:off + 2 * H], gp[off + 2 * H:off + 3 * H]
                off += 3 * H
                if l == 0:
                    gW0 = gW
                else:
                    g_trunk[4 * l - 1] = gW
                g_trunk[4 * l + 0], g_trunk[4 * l + 1], g_trunk[4 * l + 2] = gb, gg, gbe
            nh = Wh.shape[0]
            gWh = gp[off:off + nh * H].view(nh, H)
            gbh = gp[off + nh * H:off + nh * H + nh]
        return (None, gx, None, gW0, gws, gWh, gbh) + tuple(g_trunk)


def _columns(W, segs):
    """W's columns of the given [a, b) segments: a view when they are adjacent, else a concatenation (autograd routes
    the gradient back into W either way)."""
    merged = [list(segs[0])]
    for a, b in segs[1:]:
        if a == merged[-1][1]:
            merged[-1][1] = b
        else:
            merged.append([a, b])
    segs = merged
    if len(segs) == 1:
        a, b = segs[0]
        return W[:, a:b]
    return torch.cat([W[:, a:b] for a, b in segs], 1)


class FusedMLP:
    """One ``make_linear_layers(..., use_gn=True)`` trunk and its linear head(s) in HIP (module docstring).

    ``trunk``: the nn.Sequential; ``heads``: a sequence of 1-4 plain Linears (total width <= 32), or None when the
    Sequential ends in a plain Linear (that Linear is the one head).  The modules are held, not copied or registered."""

    def __init__(self, trunk, heads=None):
        self.layers, self.heads = parse_structure(trunk, heads)
        self.trunk = trunk

    def __call__(self, *blocks):
        if not blocks:
            raise ValueError('FusedMLP: give at least one input block')
        for k, x in enumerate(blocks):
            check_tensor('FusedMLP', 'input block %d' % k, x)
            if x.device.type != 'cuda':      # (need_rocm's message, and which block it is)
                raise RuntimeError('exavatar_release_amd: FusedMLP runs on a ROCm device only (no CPU path); input block %d '
                                   'is on %s' % (k, x.device))
            if x.dim() not in (1, 2):
                raise ValueError('FusedMLP: input block %d must be [N, c] or [c] (it is %s)' % (k, tuple(x.shape)))
        N = max([x.shape[0] for x in blocks if x.dim() == 2], default=None)
        if N is None:
            raise ValueError('FusedMLP: at least one input block must be per row ([N, c])')
        lin0 = self.layers[0][0]
        dev = lin0.weight.device
        rows, shared, col = [], [], 0
        for k, x in enumerate(blocks):
            is_shared = x.dim() == 1 or (x.shape[0] == 1 and N != 1)
            check_tensor('FusedMLP', 'input block %d' % k, x, f32=False, on=(lin0.weight, 'the weights'))
            c = x.shape[-1]
            if is_shared:
                if x.requires_grad:
                    raise ValueError('FusedMLP: input block %d is shared by every row and requires grad; the reference '
                                     'detaches it' % k)
                shared.append((x.reshape(c), (col, col + c)))
            else:
                if x.shape[0] != N:
                    raise ValueError('FusedMLP: input block %d has %d rows, not %d' % (k, x.shape[0], N))
                rows.append((x, (col, col + c)))
            col += c
        if col != lin0.in_features:
            raise ValueError('FusedMLP: the input blocks have %d columns in total; layer 0 (Linear) takes %d'
                             % (col, lin0.in_features))
        K0 = sum(s[1] - s[0] for _, s in rows)
        if not rows or not 1 <= K0 <= MAX_IN:
            raise ValueError('FusedMLP: the per-row input must be 1 .. %d columns wide (it is %d)' % (MAX_IN, K0))
        S = sum(s[1] - s[0] for _, s in shared)
        if S > MAX_SHARED:
            raise ValueError('FusedMLP: the shared blocks are %d columns wide; at most %d' % (S, MAX_SHARED))
        params = [lin0.weight, lin0.bias] + [t for lin, gn in self.layers for t in (lin.weight, lin.bias, gn.weight,
                                                                                   gn.bias)] + \
            [t for hd in self.heads for t in (hd.weight, hd.bias)]
        for t in params:
            if t.dtype != torch.float32 or t.device != dev:
                raise ValueError('FusedMLP: every parameter must be float32 on %s' % dev)
        x = rows[0][0] if len(rows) == 1 else torch.cat([r for r, _ in rows], 1)
        x = x.contiguous()
        W0 = _columns(lin0.weight, [s for _, s in rows])
        if W0.stride(1) != 1:
            W0 = W0.contiguous()
        p = Ws = None
        if shared:
            p = (shared[0][0] if len(shared) == 1 else torch.cat([v for v, _ in shared])).contiguous()
            Ws = _columns(lin0.weight, [s for _, s in shared])
            if Ws.stride(1) != 1:
                Ws = Ws.contiguous()
        if len(self.heads) == 1:
            Wh, bh = self.heads[0].weight, self.heads[0].bias
        else:
            Wh = torch.cat([hd.weight for hd in self.heads])
            bh = torch.cat([hd.bias for hd in self.heads])
        trunk = []
        for l, (lin, gn) in enumerate(self.layers):
            if l > 0:
                trunk.append(lin.weight.contiguous())
            trunk += [lin.bias.contiguous(), gn.weight.contiguous(), gn.bias.contiguous()]
        outs = _MLP.apply((self.layers, self.heads), x, p, W0, Ws, Wh.contiguous(), bh.contiguous(), *trunk)
        return outs if len(outs) > 1 else outs[0]
