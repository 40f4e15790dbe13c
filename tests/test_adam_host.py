"""CPU tests of the Adam step's host side: the names are exported and bound and the ABI version stays 139, every invalid
argument of ``exa_raster_adam_step`` fails with its negative status and its message before any GPU work, ``Adam`` refuses
every option it does not implement, its state dicts interchange with ``torch.optim.Adam`` both ways, extra group keys
survive, the flat list of parameters follows state surgery, and the float32 oracle (tests/adam_oracle.py) stays within 4 x
torch's own float32 error of torch's float64 run.  The ABI itself (the header against its binding) is tests/test_abi.py's."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import _lib, build, optim
from tests import adam_oracle as ao

BAD = 0x1000      # never dereferenced: every call below fails validation, or has nothing to do, first
INVALID, NULLPTR = -1, -2
FACTOR = 4.0
Seg = _lib.ExaRasterAdamSegment


def test_the_names_are_exported_and_bound():
    lib = _lib.load()
    assert 'exa_raster_adam_step' in _lib.RASTER.signatures
    fn = lib.exa_raster_adam_step
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 6
    assert lib.exa_raster_version() == 139 and _lib.RASTER.version == 139
    assert _lib.RASTER.structs['ExaRasterAdamSegment'] is Seg and ctypes.sizeof(Seg) == 48
    assert build.SOURCES['adam.hip'] == ['-ffp-contract=off']
    for name in ('Adam', 'adam_step'):
        assert name in exa.__all__ and getattr(exa, name) is getattr(optim, name)
    assert optim.MAX_SEGMENTS == 64 and optim.CHUNK == 4096
    assert issubclass(exa.Adam, torch.optim.Optimizer)


def _call(segs, n_seg=None, beta1=0.9, beta2=0.999, eps=1e-8):
    arr = (Seg * len(segs))(*segs) if segs is not None else None
    return _lib.load().exa_raster_adam_step(arr, len(segs) if n_seg is None else n_seg, beta1, beta2, eps, None)


def _seg(n=8, param=BAD, grad=BAD, exp_avg=BAD, exp_avg_sq=BAD, step_size=1e-3, bc2_sqrt=0.03):
    return Seg(param, grad, exp_avg, exp_avg_sq, n, step_size, bc2_sqrt)


def test_every_argument_error_comes_back_on_the_host():
    err = _lib.load().exa_raster_last_error
    assert _call(None, n_seg=2) == NULLPTR and err().startswith(b'exa_raster: ') and b'segs is NULL' in err()
    assert _call([_seg()], n_seg=-1) == INVALID and b'negative n_seg' in err()
    assert _call([_seg(), _seg(n=-1)]) == INVALID and b'negative n in a segment' in err()
    assert _call([_seg(n=(1 << 36) + 1)]) == INVALID and b'more than 2^36 elements' in err()
    for field in ('param', 'grad', 'exp_avg', 'exp_avg_sq'):
        assert _call([_seg(), _seg(**{field: None})]) == NULLPTR and b'holds a NULL pointer' in err()
    for beta in (-0.1, 1.0, 1.5):
        assert _call([_seg()], beta1=beta) == INVALID and b'beta1 and beta2 must be in [0, 1)' in err()
        assert _call([_seg()], beta2=beta) == INVALID and b'beta1 and beta2 must be in [0, 1)' in err()
    assert _call([_seg()], eps=-1e-8) == INVALID and b'eps must be >= 0' in err()
    for bad in (math.nan, math.inf, -math.inf):
        for key in ('beta1', 'beta2', 'eps'):
            assert _call([_seg()], **{key: bad}) == INVALID and b'must be finite' in err()
        assert _call([_seg(step_size=bad)]) == INVALID and b'step_size and bc2_sqrt must be finite' in err()
        assert _call([_seg(bc2_sqrt=bad)]) == INVALID and b'step_size and bc2_sqrt must be finite' in err()
    for bad in (0.0, -0.5):
        assert _call([_seg(bc2_sqrt=bad)]) == INVALID and b'bc2_sqrt must be > 0' in err()
    # a bad segment behind 64 good ones is found before the first launch would go out
    assert _call([_seg()] * 64 + [_seg(n=-3)]) == INVALID and b'negative n' in err()
    with pytest.raises(RuntimeError, match='exa_raster: adam: segs is NULL'):
        _lib.RASTER.check(_call(None, n_seg=1))


def test_nothing_to_do_launches_nothing_and_returns_0():
    assert _call(None, n_seg=0) == 0
    assert _call([], n_seg=0) == 0
    assert _call([_seg(n=0)] * 3) == 0
    # an empty segment's pointers and scalars are not looked at
    assert _call([_seg(n=0, param=None, grad=None, exp_avg=None, exp_avg_sq=None, bc2_sqrt=0.0, step_size=math.nan)] * 70) == 0


def test_unsupported_options_are_refused_by_name():
    p = [torch.nn.Parameter(torch.zeros(3))]
    for name, value in (('weight_decay', 0.1), ('amsgrad', True), ('maximize', True), ('capturable', True),
                        ('differentiable', True), ('foreach', True), ('foreach', False), ('fused', True), ('fused', False),
                        ('decoupled_weight_decay', True)):
        with pytest.raises(ValueError, match='Adam: %s=%r is not supported' % (name, value)):
            exa.Adam(p, **{name: value})
        with pytest.raises(ValueError, match='Adam: %s=' % name):
            exa.Adam([{'params': p, name: value}])
        opt = exa.Adam(p)
        with pytest.raises(ValueError, match='Adam: %s=' % name):
            opt.add_param_group({'params': [torch.nn.Parameter(torch.zeros(2))], name: value})
        assert len(opt.param_groups) == 1
        sd = torch.optim.Adam(p).state_dict()
        sd['param_groups'][0][name] = value
        with pytest.raises(ValueError, match='Adam: %s=' % name):
            opt.load_state_dict(sd)
    exa.Adam(p, weight_decay=0.0, amsgrad=False, foreach=None, fused=None)        # the defaults pass
    with pytest.raises(TypeError, match="unexpected keyword argument 'momentum'"):
        exa.Adam(p, momentum=0.9)
    with pytest.raises(ValueError, match='complex parameters are not supported'):
        exa.Adam([torch.nn.Parameter(torch.zeros(3, dtype=torch.complex64))])
    for betas in ((1.0, 0.999), (0.9, -0.1)):
        with pytest.raises(ValueError, match=r'betas must be in \[0, 1\)'):
            exa.Adam(p, betas=betas)
    with pytest.raises(ValueError, match='eps must be finite and >= 0'):
        exa.Adam(p, eps=-1.0)
    with pytest.raises(ValueError, match='lr must be finite'):
        exa.Adam(p, lr=math.inf)


def _groups(params):
    return [{'params': [p], 'name': n, 'lr': 1e-3 * (i + 1)} for i, (n, p) in enumerate(params.items())]


def _small(dtype=torch.float32):
    rs = np.random.RandomState(5)
    return {n: torch.nn.Parameter(torch.from_numpy(rs.randn(*s)).to(dtype)) for n, s in
            (('mean', (7, 3)), ('opacity', (7, 1)), ('trans', (3,)), ('idle', (4,)))}


def _cpu_steps(opt, params, k, seed):
    rs = np.random.RandomState(seed)
    for _ in range(k):
        for n, p in params.items():
            p.grad = None if n == 'idle' else torch.from_numpy(rs.randn(*p.shape)).to(p.dtype)
        opt.step()


def _assert_state_dicts_equal(a, b):
    assert [list(g) for g in a['param_groups']] == [list(g) for g in b['param_groups']]
    assert a['param_groups'] == b['param_groups']
    assert list(a['state']) == list(b['state'])
    for k in a['state']:
        assert list(a['state'][k]) == list(b['state'][k]) == ['step', 'exp_avg', 'exp_avg_sq']
        for name in a['state'][k]:
            x, y = a['state'][k][name], b['state'][k][name]
            assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device and torch.equal(x, y), (k, name)


def test_a_state_dict_goes_torch_to_adam_to_torch():
    params = _small()
    first = torch.optim.Adam(_groups(params), lr=0.0, eps=1e-15)
    _cpu_steps(first, params, 3, seed=1)
    sd = copy.deepcopy(first.state_dict())                      # as torch.save / torch.load hand it over: load_state_dict
    #                                                             keeps tensors of the right dtype and device as they are
    assert sorted(sd['state']) == [0, 1, 2]                      # the idle parameter has no state
    ours = exa.Adam(_groups(params), lr=0.0, eps=1e-15)          # constructed on the CPU
    assert list(ours.state_dict()['param_groups'][0]) == list(sd['param_groups'][0])
    ours.load_state_dict(copy.deepcopy(sd))
    _assert_state_dicts_equal(ours.state_dict(), sd)
    st = ours.state[params['mean']]
    assert st['step'].dtype == torch.float32 and st['step'].dim() == 0 and st['step'].device.type == 'cpu'
    assert float(st['step']) == 3.0
    # and back: a fresh torch optimizer that loads ours continues exactly as the first one does
    clone = {n: torch.nn.Parameter(p.detach().clone()) for n, p in params.items()}
    back = torch.optim.Adam(_groups(clone), lr=0.0, eps=1e-15)
    back.load_state_dict(copy.deepcopy(ours.state_dict()))
    _assert_state_dicts_equal(back.state_dict(), sd)
    _cpu_steps(first, params, 2, seed=2)
    _cpu_steps(back, clone, 2, seed=2)
    for n in params:
        assert torch.equal(params[n], clone[n]), n
    _assert_state_dicts_equal(back.state_dict(), first.state_dict())
    _assert_state_dicts_equal(ours.state_dict(), sd)             # untouched by either


def test_name_and_other_group_keys_survive():
    params = _small()
    groups = _groups(params)
    groups[1]['frozen'] = ('anything', 3)
    opt = exa.Adam(groups, lr=0.0, eps=1e-15)
    assert [g['name'] for g in opt.param_groups] == list(params)
    assert opt.param_groups[1]['frozen'] == ('anything', 3)
    assert [g['lr'] for g in opt.param_groups] == [1e-3, 2e-3, 3e-3, 4e-3] and opt.defaults['lr'] == 0.0
    assert all(g['eps'] == 1e-15 and g['betas'] == (0.9, 0.999) for g in opt.param_groups)
    sd = opt.state_dict()
    assert sd['param_groups'][1]['frozen'] == ('anything', 3) and sd['param_groups'][2]['name'] == 'trans'
    for g in opt.param_groups:                                  # what Trainer.set_lr does
        g['lr'] = 0.5
    assert all(g['lr'] == 0.5 for g in opt.param_groups)
    exa.Adam(list(params.values()))                             # plain tensors, as torch takes them
    opt.zero_grad()


def test_the_flat_list_follows_state_surgery():
    params = _small()
    opt = exa.Adam(_groups(params), lr=0.0, eps=1e-15)
    flat = opt._flat_params()
    assert [p for p, _ in flat] == list(params.values()) and [g['name'] for _, g in flat] == list(params)
    assert opt._flat_params() is flat                           # unchanged groups: the same list, not a rebuilt one
    # replace_param_from_optimizer of the reference (module.py:58-72), for 'opacity'
    group = opt.param_groups[1]
    opt.state[group['params'][0]] = {'step': torch.tensor(2.0), 'exp_avg': torch.ones(7, 1), 'exp_avg_sq': torch.ones(7, 1)}
    stored = opt.state.get(group['params'][0], None)
    fresh_value = torch.zeros(9, 1)
    stored['exp_avg'], stored['exp_avg_sq'] = torch.zeros_like(fresh_value), torch.zeros_like(fresh_value)
    del opt.state[group['params'][0]]
    group['params'][0] = torch.nn.Parameter(fresh_value.requires_grad_(True))
    opt.state[group['params'][0]] = stored
    again = opt._flat_params()
    assert again is not flat and again[1][0] is group['params'][0] and again[1][1] is group
    assert [p for p, _ in again][0] is params['mean'] and len(again) == 4
    assert opt._flat_params() is again
    # a new group and a second member of a group are seen as well
    extra = torch.nn.Parameter(torch.zeros(2))
    opt.add_param_group({'params': [extra], 'name': 'extra'})
    assert opt._flat_params()[-1][0] is extra and len(opt._flat_params()) == 5
    opt.param_groups[0]['params'].append(torch.nn.Parameter(torch.zeros(1)))
    assert len(opt._flat_params()) == 6 and opt._flat_params()[1][1] is opt.param_groups[0]


def test_the_flat_list_follows_replaced_group_dicts():
    """``load_state_dict`` replaces every dict of ``param_groups`` (the 'params' lists stay): the flat list must hand out
    the live dicts, or a step reads 'lr' from discarded ones and ``Trainer.set_lr`` is lost."""
    params = _small()
    opt = exa.Adam(_groups(params), lr=0.0, eps=1e-15)
    flat = opt._flat_params()
    old_groups = list(opt.param_groups)
    sd = copy.deepcopy(opt.state_dict())
    sd['param_groups'][0]['lr'] = 0.5
    opt.load_state_dict(sd)
    assert all(a is not b for a, b in zip(old_groups, opt.param_groups))          # torch made new dicts
    again = opt._flat_params()
    assert again is not flat and len(again) == 4
    for i, (p, group) in enumerate(again):
        assert group is opt.param_groups[i] and p is group['params'][0]
    assert again[0][1]['lr'] == 0.5
    for g in opt.param_groups:                                  # what Trainer.set_lr does
        g['lr'] = 0.25
    assert all(group['lr'] == 0.25 for _, group in opt._flat_params()) and opt._flat_params() is again
    # a caller that assigns a group dict
    opt.param_groups[2] = dict(opt.param_groups[2], lr=0.125)
    third = opt._flat_params()
    assert third is not again and third[2][1] is opt.param_groups[2] and third[2][1]['lr'] == 0.125
    # unpickling goes through __setstate__
    clone = copy.deepcopy(opt)
    assert all(group is clone.param_groups[i] for i, (_, group) in enumerate(clone._flat_params()))


def test_step_needs_rocm_and_leaves_the_state_alone_when_it_raises():
    params = _small()
    opt = exa.Adam(_groups(params), lr=0.0, eps=1e-15)
    assert opt.step() is None                                   # no gradient anywhere: nothing to do, on any device
    assert opt.step(lambda: 1.5) == 1.5
    before = {n: p.detach().clone() for n, p in params.items()}
    params['trans'].grad = torch.ones(3)
    with pytest.raises(RuntimeError, match=r'Adam.step runs on a ROCm device only \(no CPU path\)'):
        opt.step()
    assert len(opt.state) == 0 and all(torch.equal(before[n], params[n]) for n in params)
    params['trans'].grad = torch.sparse_coo_tensor([[0]], [1.0], (3,))
    with pytest.raises((RuntimeError, ValueError), match='ROCm device only|sparse gradients are not supported'):
        opt.step()
    assert len(opt.state) == 0


def test_adam_step_refuses_what_it_does_not_support():
    ok = lambda: torch.zeros(4, 3)      # noqa: E731
    step = exa.adam_step
    assert step([], [], [], [], [], lr=1e-3) is None
    with pytest.raises(RuntimeError, match=r'adam_step runs on a ROCm device only \(no CPU path\)'):
        step([ok()], [ok()], [ok()], [ok()], [1], lr=1e-3)
    with pytest.raises(TypeError, match=r'adam_step: grads\[0\] must be a tensor'):
        step([ok()], [ok().numpy()], [ok()], [ok()], [1], lr=1e-3)
    with pytest.raises(ValueError, match=r'adam_step: exp_avgs\[1\] must be float32 \(it is torch.float64\)'):
        step([ok(), ok()], [ok(), ok()], [ok(), ok().double()], [ok(), ok()], [1, 1], lr=1e-3)
    with pytest.raises(ValueError, match=r'adam_step: params\[0\] must be float32'):
        step([ok().half()], [ok()], [ok()], [ok()], [1], lr=1e-3)
    with pytest.raises(ValueError, match=r'adam_step: grads\[0\] is sparse; sparse gradients are not supported'):
        step([ok()], [ok().to_sparse()], [ok()], [ok()], [1], lr=1e-3)
    with pytest.raises(ValueError, match=r'adam_step: grads\[0\] has shape \(3, 4\), params\[0\] has \(4, 3\)'):
        step([ok()], [ok().t()], [ok()], [ok()], [1], lr=1e-3)
    with pytest.raises(ValueError, match=r'adam_step: exp_avg_sqs\[0\] must be contiguous'):
        step([ok()], [ok()], [ok()], [torch.zeros(3, 4).t()], [1], lr=1e-3)
    with pytest.raises(ValueError, match=r'adam_step: params\[0\] must be contiguous'):
        step([torch.zeros(3, 4).t()], [ok()], [ok()], [ok()], [1], lr=1e-3)
    with pytest.raises(ValueError, match='adam_step: steps has 2 entries for 1 params'):
        step([ok()], [ok()], [ok()], [ok()], [1, 2], lr=1e-3)
    with pytest.raises(ValueError, match='adam_step: lr has 2 entries for 1 params'):
        step([ok()], [ok()], [ok()], [ok()], [1], lr=[1e-3, 1e-3])
    with pytest.raises(ValueError, match=r'adam_step: steps\[0\] must be the count of this update, >= 1'):
        step([ok()], [ok()], [ok()], [ok()], [0], lr=1e-3)
    with pytest.raises(ValueError, match=r'adam_step: lr\[0\] must be finite'):
        step([ok()], [ok()], [ok()], [ok()], [1], lr=math.nan)
    with pytest.raises(ValueError, match=r'adam_step: betas must be in \[0, 1\)'):
        step([ok()], [ok()], [ok()], [ok()], [1], lr=1e-3, betas=(0.9, 1.0))
    with pytest.raises(ValueError, match='adam_step: eps must be finite and >= 0'):
        step([ok()], [ok()], [ok()], [ok()], [1], lr=1e-3, eps=-1e-8)


def test_the_scalars_are_torchs():
    """step_size and bc2_sqrt as torch's single-tensor Adam forms them (double), rounded once."""
    for t, lr, b1, b2 in ((1, 1e-3, 0.9, 0.999), (2, 0.0, 0.9, 0.999), (1000, 1.6e-4, 0.4, 0.9)):
        seg = optim._segment(torch.zeros(5), torch.zeros(5), torch.zeros(5), torch.zeros(5), float(t), lr, b1, b2)
        bias_correction1, bias_correction2 = 1 - b1 ** t, 1 - b2 ** t
        want = ao.scalars(t, lr, b1, b2)
        assert seg.step_size == np.float32(lr / bias_correction1) == want[0]
        assert seg.bc2_sqrt == np.float32(bias_correction2 ** 0.5) == want[1] and seg.n == 5


@pytest.fixture(scope='module')
def cpu_runs():
    """The grouping case through torch.optim.Adam on the CPU in float64 and float32, and through the oracle."""
    init, lrs, grads = ao.grouping_case()
    out = {}
    for dtype in (torch.float64, torch.float32):
        params, opt = ao.make_optimizer(torch.optim.Adam, init, lrs, dtype, 'cpu')
        ao.run(opt, params, grads, dtype)
        out[dtype] = ({n: p.detach().numpy() for n, p in params.items()}, opt)
    out['oracle'] = ao.oracle_run(init, lrs, grads)
    return init, out


def test_the_oracle_is_within_4_e32_of_torchs_float64_run(cpu_runs):
    init, out = cpu_runs
    ref64, t32, (oracle, state) = out[torch.float64][0], out[torch.float32][0], out['oracle']
    worst = 0.0
    for n in init:
        if n.endswith('_%d' % ao.IDLE_FRAME):
            assert np.array_equal(oracle[n], init[n]) and np.array_equal(t32[n], init[n]) and n not in state
            continue
        e32, err = ao.max_err(t32[n], ref64[n]), ao.max_err(oracle[n], ref64[n])
        print('%-24s e32 %.3e  oracle %.3e  ratio %.3f' % (n, e32, err, err / e32 if e32 else math.inf))
        assert e32 > 0.0 and err <= FACTOR * e32, (n, e32, err)
        worst = max(worst, err / e32)
        assert state[n][2] == ao.STEPS
    print('largest ratio %.3f' % worst)
    opt64 = out[torch.float64][1]
    for group in opt64.param_groups:                             # the moments against the float64 run, by the same bound
        n, p = group['name'], group['params'][0]
        if n not in state:
            assert p not in opt64.state
            continue
        st32 = out[torch.float32][1].state[out[torch.float32][1].param_groups[list(init).index(n)]['params'][0]]
        for key, mine in (('exp_avg', state[n][0]), ('exp_avg_sq', state[n][1])):
            ref = opt64.state[p][key].numpy()
            e32, err = ao.max_err(st32[key].numpy(), ref), ao.max_err(mine, ref)
            assert err <= FACTOR * e32, (n, key, e32, err)
