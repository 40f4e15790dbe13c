"""HIP Adam: a drop-in for the reference's ``torch.optim.Adam(params, lr=0.0, eps=1e-15)`` (``avatar/common/base.py:83-85``,
stepped at ``avatar/main/train.py:57``) that updates every tensor with a gradient in ONE launch per 64 tensors, whatever
groups they are in.

* ``adam_step(params, grads, exp_avgs, exp_avg_sqs, steps, *, lr, betas, eps)`` -- the functional form, for gradients held
  in plain arrays (``StaticRender.grads``) and hand-written loops.
* ``Adam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8)`` -- a ``torch.optim.Optimizer`` with torch's own per-parameter
  state (``'step'`` a 0-dim float32 host tensor, ``'exp_avg'``, ``'exp_avg_sq'``), so ``state_dict()`` /
  ``load_state_dict()`` interchange with ``torch.optim.Adam`` both ways and ``densify.densify_and_prune`` and the
  reference's ``cat_params_to_optimizer`` / ``prune_params_from_optimizer`` / ``replace_param_from_optimizer`` work on it
  as they are.

The reference makes almost every parameter the only member of its own group (six scene groups, twelve human groups, nine
per frame of the capture) and torch fuses within a group only; here the tensors of all groups travel together.  The kernel
is ``csrc/adam.hip`` behind ``exa_raster_adam_step`` (``include/exa_raster.h``), which writes out every operation; the
segments travel by value, there is no workspace and no state.  float32 ROCm tensors only, no CPU path for the step itself;
construction and the state dicts work on any device.  The CPU restatement that pins the arithmetic is
``tests/adam_oracle.py``.

The scalars of a step (``lr / (1 - beta1^t)``, ``sqrt(1 - beta2^t)``) are formed on the host in double and travel by value:
a stream capture would bake them in, so ``Adam.step`` and ``adam_step`` refuse to run under one.
"""
import math
from itertools import chain
from operator import itemgetter

import torch

from . import _lib
from ._device import check_tensor, launch

MAX_SEGMENTS = 64         # EXA_RASTER_ADAM_MAX_SEGMENTS: tensors per launch
CHUNK = 4096              # EXA_RASTER_ADAM_CHUNK: elements per workgroup

# torch.optim.Adam's options this optimizer does not implement, with the one value each may have
UNSUPPORTED = {'weight_decay': 0, 'amsgrad': False, 'maximize': False, 'foreach': None, 'capturable': False,
               'differentiable': False, 'fused': None, 'decoupled_weight_decay': False}


def _hyper(what, betas, eps):
    beta1, beta2 = (float(b) for b in betas)
    eps = float(eps)
    if not 0.0 <= beta1 < 1.0 or not 0.0 <= beta2 < 1.0:
        raise ValueError('%s: betas must be in [0, 1) (they are %r)' % (what, (beta1, beta2)))
    if not 0.0 <= eps < math.inf:
        raise ValueError('%s: eps must be finite and >= 0 (it is %r)' % (what, eps))
    return beta1, beta2, eps


def _segment(p, g, m, v, step, lr, beta1, beta2):
    """The tensor's record: its arrays and the two scalars of its step, formed in double as torch forms them."""
    return _lib.ExaRasterAdamSegment(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(),
                                     lr / (1.0 - beta1 ** step), math.sqrt(1.0 - beta2 ** step))


def _refuse_capture(what):
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError('%s: the step count and the learning rate travel by value and a stream capture would bake them '
                           'in; step outside the capture' % what)


def _launch(device, segments, beta1, beta2, eps):
    launch(_lib.RASTER, 'exa_raster_adam_step', device, (_lib.ExaRasterAdamSegment * len(segments))(*segments),
           len(segments), beta1, beta2, eps)


def _check_disjoint(what, written, read):
    """No written array may overlap any other array of the call."""
    spans = [(t.data_ptr(), t.data_ptr() + 4 * t.numel(), True, n) for n, t in written if t.numel()]
    spans += [(t.data_ptr(), t.data_ptr() + 4 * t.numel(), False, n) for n, t in read if t.numel()]
    spans.sort(key=lambda s: (s[0], s[1]))
    w_end, w_name, r_end, r_name = 0, None, 0, None          # the furthest end of the written / read arrays so far
    for lo, hi, is_written, name in spans:
        if lo < w_end:
            raise ValueError('%s: %s and %s share memory' % (what, w_name, name))
        if is_written and lo < r_end:
            raise ValueError('%s: %s and %s share memory' % (what, r_name, name))
        if is_written and hi > w_end:
            w_end, w_name = hi, name
        if not is_written and hi > r_end:
            r_end, r_name = hi, name


def adam_step(params, grads, exp_avgs, exp_avg_sqs, steps, *, lr, betas=(0.9, 0.999), eps=1e-8):
    """One Adam update of ``params[i]`` from ``grads[i]`` with the moments ``exp_avgs[i]`` / ``exp_avg_sqs[i]``, all in
    place, in one launch per 64 tensors.  ``steps[i]`` is the host-side count ``t >= 1`` of THIS update of tensor i (1 for
    its first); ``lr`` is a float or one float per tensor.  Every tensor is a float32 ROCm tensor of one device; parameters
    and moments must be contiguous (they are updated where they are), a non-contiguous gradient is made contiguous.
    ``lr = 0`` leaves the parameter bit-unchanged and still advances the moments.  Returns None."""
    what = 'adam_step'
    lists = [list(x) for x in (params, grads, exp_avgs, exp_avg_sqs, steps)]
    n = len(lists[0])
    for name, x in zip(('grads', 'exp_avgs', 'exp_avg_sqs', 'steps'), lists[1:]):
        if len(x) != n:
            raise ValueError('%s: %s has %d entries for %d params' % (what, name, len(x), n))
    params, grads, exp_avgs, exp_avg_sqs, steps = lists
    lrs = [float(x) for x in lr] if isinstance(lr, (list, tuple)) else [float(lr)] * n
    if len(lrs) != n:
        raise ValueError('%s: lr has %d entries for %d params' % (what, len(lrs), n))
    beta1, beta2, eps = _hyper(what, betas, eps)
    named = [[('%s[%d]' % (name, i), t) for i, t in enumerate(x)]
             for name, x in (('params', params), ('grads', grads), ('exp_avgs', exp_avgs), ('exp_avg_sqs', exp_avg_sqs))]
    for column in named:
        for name, t in column:
            check_tensor(what, name, t)
            if t.is_sparse:
                raise ValueError('%s: %s is sparse; sparse gradients are not supported' % (what, name))
    for i, (p, g, m, v) in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs)):
        for name, t in (('grads', g), ('exp_avgs', m), ('exp_avg_sqs', v)):
            if t.shape != p.shape:
                raise ValueError('%s: %s[%d] has shape %s, params[%d] has %s' % (what, name, i, tuple(t.shape), i,
                                                                                 tuple(p.shape)))
        for name, t in (('params', p), ('exp_avgs', m), ('exp_avg_sqs', v)):
            if not t.is_contiguous():
                raise ValueError('%s: %s[%d] must be contiguous: it is updated in place' % (what, name, i))
    steps = [float(s) for s in steps]
    for i, (s, x) in enumerate(zip(steps, lrs)):
        if not s >= 1.0 or not math.isfinite(s):
            raise ValueError('%s: steps[%d] must be the count of this update, >= 1 (it is %r)' % (what, i, s))
        if not math.isfinite(x):
            raise ValueError('%s: lr[%d] must be finite (it is %r)' % (what, i, x))
    for column in named:
        for name, t in column:
            check_tensor(what, name, t, f32=False, rocm=True, on=(params[0], 'params[0]'))
    if n == 0:
        return
    _refuse_capture(what)
    grads = [g.contiguous() for g in grads]
    _check_disjoint(what, named[0] + named[2] + named[3], [('grads[%d]' % i, g) for i, g in enumerate(grads)])
    _launch(params[0].device, [_segment(p, g, m, v, s, x, beta1, beta2) for p, g, m, v, s, x in
                                     zip(params, grads, exp_avgs, exp_avg_sqs, steps, lrs)], beta1, beta2, eps)


class Adam(torch.optim.Optimizer):
    """``torch.optim.Adam`` without weight decay and amsgrad, stepped by ``exa_raster_adam_step``: every parameter with a
    gradient, across ALL groups, in one launch per 64 tensors.

    ``params`` as torch takes them: tensors, or dicts with ``'params'``, optionally ``'lr'`` / ``'betas'`` / ``'eps'`` and
    any further keys (the reference's ``'name'``), which stay in ``param_groups`` -- ``Trainer.set_lr`` works unchanged.
    The per-parameter state and the group keys are torch's, so state dicts go both ways between the two classes.  Every
    other option of ``torch.optim.Adam`` (``UNSUPPORTED``) may only have its default value; anything else raises
    ``ValueError`` naming the option, at construction, in ``add_param_group`` and in ``load_state_dict``.

    ``step()`` needs float32 ROCm parameters with dense float32 gradients; parameters without a gradient are untouched
    and their ``'step'`` does not advance; the step counts advance, and new state is kept, only after the C call that
    used them has returned without an error.  The walk over the groups is one flat list of ``(parameter, group)`` that is
    rebuilt when a group dict or a member of a ``'params'`` list is another object than before (``load_state_dict``
    replaces the dicts, state surgery the parameters)."""

    _flat, _flat_ids = [], None       # class defaults: Optimizer.__getstate__ pickles defaults, state and param_groups only

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, **options):
        for name in options:
            if name not in UNSUPPORTED:
                raise TypeError("Adam: unexpected keyword argument '%s'" % name)
        defaults = dict(lr=lr, betas=betas, eps=eps)
        for name, value in UNSUPPORTED.items():              # torch's keys in torch's order: the state dicts interchange
            defaults[name] = options.get(name, value)
        super().__init__(params, defaults)

    @staticmethod
    def _check_group(group):
        what = 'Adam'
        for name, value in UNSUPPORTED.items():
            got = group.get(name, value)
            if not (got is value or (value is not None and type(got) in (bool, int, float) and got == value)):
                raise ValueError('%s: %s=%r is not supported (only %r)' % (what, name, got, value))
        if not math.isfinite(float(group['lr'])):
            raise ValueError('%s: lr must be finite (it is %r)' % (what, group['lr']))
        _hyper(what, group['betas'], group['eps'])
        for p in group['params']:
            if isinstance(p, torch.Tensor) and p.is_complex():
                raise ValueError('%s: complex parameters are not supported' % what)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        try:
            self._check_group(self.param_groups[-1])
        except ValueError:
            self.param_groups.pop()
            raise

    def load_state_dict(self, state_dict):
        for group in state_dict['param_groups']:
            self._check_group(dict(group, params=[]))
        super().load_state_dict(state_dict)

    def _members(self):
        return chain.from_iterable(map(itemgetter('params'), self.param_groups))

    def _flat_params(self):
        """``[(parameter, group)]`` over all groups in order; rebuilt when the identity of any group dict or of any member
        changed (``load_state_dict`` replaces every group dict, state surgery replaces members).  The list holds the objects
        whose ids it compares, so no id can be reused while it is current."""
        ids = list(map(id, self.param_groups)) + list(map(id, self._members()))
        if ids != self._flat_ids:
            self._flat = [(p, group) for group in self.param_groups for p in group['params']]
            self._flat_ids = ids
        return self._flat

    @torch.no_grad()
    def step(self, closure=None):
        what = 'Adam.step'
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        live = [(p, group) for p, group in self._flat_params() if p.grad is not None]
        if not live:
            return loss
        for p, _ in live:
            check_tensor(what, 'a parameter', p, rocm=True)
            g = p.grad
            if g.is_sparse:
                raise ValueError('%s: sparse gradients are not supported' % what)
            if g.dtype != torch.float32 or g.device != p.device:
                raise ValueError('%s: a gradient must be float32 on its parameter\'s device (it is %s on %s)' % (
                    what, g.dtype, g.device))
            if not p.is_contiguous():
                raise ValueError('%s: a parameter must be contiguous: it is updated in place' % what)
            state = self.state.get(p)
            if state:                                        # state that was loaded or operated on: as torch lays it out
                m, v = state['exp_avg'], state['exp_avg_sq']
                if not (m.is_contiguous() and v.is_contiguous() and m.shape == p.shape and v.shape == p.shape
                        and m.dtype == v.dtype == torch.float32 and m.device == v.device == p.device):
                    raise ValueError('%s: exp_avg / exp_avg_sq must be contiguous float32 tensors of the parameter\'s '
                                     'shape and device' % what)
        _refuse_capture(what)
        calls = {}                      # (device, beta1, beta2, eps) -> (segments, what to commit): one C call each
        for p, group in live:
            state = self.state.get(p) or {'step': torch.tensor(0.0, dtype=torch.float32),
                                          'exp_avg': torch.zeros_like(p, memory_format=torch.preserve_format),
                                          'exp_avg_sq': torch.zeros_like(p, memory_format=torch.preserve_format)}
            beta1, beta2, eps = _hyper(what, group['betas'], group['eps'])
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()     # a copy lives until its launch is enqueued
            segments, commits = calls.setdefault((p.device, beta1, beta2, eps), ([], []))
            segments.append(_segment(p, g, state['exp_avg'], state['exp_avg_sq'], float(state['step']) + 1.0,
                                     float(group['lr']), beta1, beta2))
            commits.append((p, state, g))
        for (device, beta1, beta2, eps), (segments, commits) in calls.items():
            _launch(device, segments, beta1, beta2, eps)
            for p, state, _ in commits:                      # a call that raised advances no step count and adds no state
                state['step'] += 1
                self.state[p] = state
        return loss
