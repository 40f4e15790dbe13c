"""What every feature module needs to hand torch tensors to the C ABIs: data pointers, the current stream, workspaces
from the torch allocator, the launch of a stream-taking call, the warm-up before a stream capture, incoming gradients, the
argument checks the features share and the package's run-time ``config``."""
import ctypes

import torch

from . import _lib


class _Config:
    mode = 'auto'             # 'auto' | 'exact' | 'capacity'
    capacity_growth = 1.5     # capacity mode: head-room over the largest D seen so far
    min_capacity = 1 << 16
    fixed_capacity = None     # capacity mode: use exactly this many instances (e.g. calibrated by a warm-up); a list /
    #                           tuple names one capacity per job of a batched call
    keep_debug = False        # developer probes: keep the workspaces of the most recent forward reachable
    on_overflow = 'retry'     # 'retry' | 'raise' (rasterizer module docstring)
    overlap_composites = True     # INSIDE a stream capture: the composites' list merges run on a second stream while their sources
    #                               blend (the calls are split at EXA_RASTER_STAGE_NO_BLEND; fork / join become graph edges).
    #                               Eager calls never do this: the stream switches cost the host more than the overlap gives
    fold_composite_grads = True   # a composite's gradients for source B are handed to B's own render, whose backward adds them
    #                               inside its per-Gaussian kernel (ExaRasterBackwardJob.accumulate) instead of autograd
    #                               summing the two with one kernel per tensor (developer A/B knob; same values bit for bit)
    compose_reuse_source = True   # composite renders copy source A's pixels where source B has no entry (developer A/B knob)
    upstream_scale_grad = False   # True: dL/dscale as upstream returns it (w.r.t. scale_modifier * scale, i.e. divided
    #                               by scale_modifier); identical for the reference, which passes 1.0 (module.py:615)
    knn_cull = True               # knn_points: cull ref chunks by their boxes (False: visit every ref; the same bits either way)
    poison = False                # debug: fill every workspace with 0xFF before the kernels see it (the library promises to write
    #                               every section before it reads it; tests run under it with EXA_TEST_POISON=1)
    compiled_node = 'auto'        # single renders through the compiled autograd node (csrc/torch_binding.cpp -> _exa_torch.so: the
    #                               same C-ABI calls, arena layouts and overflow protocol as rasterizer._Rasterize at a quarter of
    #                               the host time): 'auto' = when it is built and the call is one it covers, 'off' = always the
    #                               Python node, 'require' = raise if the extension is missing


config = _Config()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _ptrs(tensors):
    """Host array of device pointers (NULL for None)."""
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


def _addr(t):
    return t.data_ptr() if t is not None else None


def _stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _workspace(nbytes, device):
    """Uninitialised byte workspace (``config.poison``: filled with 0xFF, so that a kernel reading a section nobody
    wrote sees the worst garbage instead of whatever the allocator left there)."""
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    if config.poison:
        ws.fill_(255)
    return ws


class _NoCtx:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_CTX = _NoCtx()


def _on_device(device):
    """``torch.cuda.device(device)`` only when it is not the current device already (the context manager costs ~10 us
    per entry, twice per render, in an eager training loop)."""
    return _NO_CTX if torch.cuda.current_device() == device.index else torch.cuda.device(device)


def warm_up(device, fn):
    """The warm-up ``torch.cuda.graph`` asks for before a capture: ``fn()`` on a fresh side stream, joined at both ends; a device wait."""
    side, main = torch.cuda.Stream(device=device), torch.cuda.current_stream(device)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        fn()
    main.wait_stream(side)
    torch.cuda.synchronize(device)


def launch(abi, name, device, *args):
    """One stream-taking call of a C ABI: ``device`` is made current, ``name(*args, stream)`` is enqueued on its current
    stream and the status goes to ``abi.check``."""
    with _on_device(device):
        abi.check(getattr(_lib.load(), name)(*args, _stream_ptr(device)))


def grad_in(g):
    """An incoming gradient as a contiguous float32 tensor (``g`` itself when it is one already); None stays None."""
    return None if g is None else g.to(torch.float32).contiguous()


def need_rocm(device, what):
    if device.type != 'cuda':
        raise RuntimeError('exavatar_release_amd: %s runs on a ROCm device only (no CPU path)' % what)


def check_tensor(what, name, x, f32=True, rocm=False, on=None):
    """The argument checks the features share, in this order: ``x`` is a tensor; with ``rocm``, it is on a ROCm device;
    with ``f32``, it is float32; with ``on`` = (anchor tensor, its name), it is on the anchor's device."""
    if not isinstance(x, torch.Tensor):
        raise TypeError('%s: %s must be a tensor' % (what, name))
    if rocm:
        need_rocm(x.device, what)
    if f32 and x.dtype != torch.float32:
        raise ValueError('%s: %s must be float32 (it is %s)' % (what, name, x.dtype))
    if on is not None and x.device != on[0].device:
        raise ValueError('%s: %s is not on the device of %s' % (what, name, on[1]))


def check_shape(what, name, x, shape, text, shared=False):
    """None in ``shape``: any extent.  ``shared``: the first extent may also be 1 (data that the whole batch shares)."""
    check_tensor(what, name, x)
    if x.dim() != len(shape) or any(s is not None and x.shape[i] != s and not (shared and i == 0 and x.shape[0] == 1)
                                    for i, s in enumerate(shape)):
        raise ValueError('%s: %s must be %s (it is %s)' % (what, name, text, tuple(x.shape)))


def check_rows(what, name, x, V, shapes=None, text='[V], [V, 1] or [1, V, 1]'):
    """Per-vertex data (by default a weight): a float32 tensor without a gradient in one of ``shapes``, which the message
    names as ``text``; returns it contiguous in the first of them."""
    check_tensor(what, name, x)
    check_no_grad(what, name, x)
    shapes = shapes or ((V,), (V, 1), (1, V, 1))
    if tuple(x.shape) not in shapes:
        raise ValueError('%s: %s must be %s with V = %d (it is %s)' % (what, name, text, V, tuple(x.shape)))
    return x.reshape(shapes[0]).contiguous()


def check_mask(what, name, m, V):
    if not isinstance(m, torch.Tensor) or m.dtype != torch.bool or m.dim() != 1 or m.shape[0] != V:
        raise ValueError('%s: %s must be a bool [V] tensor with V = %d (it is %s)' % (
            what, name, V, '%s %s' % (m.dtype, tuple(m.shape)) if isinstance(m, torch.Tensor) else type(m).__name__))


def check_devices(what, anchor_name, anchor, **others):
    """The anchor is on a ROCm device (a ValueError here, unlike ``need_rocm``), the others (None passes) on the anchor's."""
    if anchor.device.type != 'cuda':
        raise ValueError('%s: %s must be on a ROCm device (it is on %s; there is no CPU path)'
                         % (what, anchor_name, anchor.device))
    for name, x in others.items():
        if x is not None and x.device != anchor.device:
            raise ValueError('%s: %s is not on the device of %s' % (what, name, anchor_name))


def check_reduce(what, reduce):
    if reduce not in (None, 'mean'):
        raise ValueError("%s: reduce must be None or 'mean' (it is %r)" % (what, reduce))


def check_no_grad(what, name, x, kind='data'):
    """What the reference holds as ``kind`` (data, a buffer, camera data) gets no gradient: a tensor that requires one is
    refused.  Anything else passes (None included)."""
    if isinstance(x, torch.Tensor) and x.requires_grad:
        raise ValueError('%s: %s is %s in the reference and gets no gradient; detach it' % (what, name, kind))
