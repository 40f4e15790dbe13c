"""GPU tests of the Adam step (csrc/adam.hip, exavatar_release_amd/optim.py).  The kernel is BIT-equal to the float32 oracle
(tests/adam_oracle.py) at every segment length, alignment and segment count at which it branches, for every step count,
eps, lerp branch and learning rate the issue names, leaves every guard element around every view alone and gives the same
bits twice; ``Adam.step()`` stays within 4 x torch's own float32 error of torch's float64 CPU run on a small copy of the
reference's grouping and exchanges state dicts with ``torch.optim.Adam`` mid-run; ``densify_and_prune`` carries its state;
the raw C ABI works from plain pointers; a stream capture is refused and stays usable."""
import ctypes

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import _lib, densify, optim
from tests import adam_oracle as ao

pytestmark = pytest.mark.gpu

C = optim.CHUNK
GUARD = np.float32(-12345.678)
PAD = 8                   # guard floats behind every view
FACTOR = 4.0
ROLES = ('param', 'grad', 'exp_avg', 'exp_avg_sq')
ALIGNED = dict.fromkeys(ROLES, 4)      # a view 16 bytes into its allocation: aligned, with guards in front


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _values(rs, n, zero=False):
    """Initial (param, grad, exp_avg, exp_avg_sq) of one tensor: a state as after some steps, or all-zero moments under
    a gradient with exact zeros in it."""
    p, g = rs.randn(n).astype(np.float32), (rs.randn(n) * 10.0 ** rs.uniform(-3, 0)).astype(np.float32)
    if zero:
        g[::2] = 0.0
        return p, g, np.zeros(n, np.float32), np.zeros(n, np.float32)
    return p, g, (0.1 * rs.randn(n)).astype(np.float32), (0.01 * rs.randn(n) ** 2).astype(np.float32)


class Case:
    """Tensors as views into guarded allocations: ``specs`` = [(n, {role: offset in floats})]."""

    def __init__(self, dev, specs, seed=0, zero=False):
        rs = np.random.RandomState(seed)
        self.host = [dict(zip(ROLES, _values(rs, n, zero))) for n, _ in specs]
        self.base, self.view = [], []
        for (n, off), h in zip(specs, self.host):
            bases = {r: torch.full((off[r] + n + PAD,), float(GUARD), dtype=torch.float32, device=dev) for r in ROLES}
            views = {r: bases[r][off[r]:off[r] + n] for r in ROLES}
            for r in ROLES:
                views[r].copy_(torch.from_numpy(h[r]))
                assert n == 0 or views[r].data_ptr() % 16 == (4 * off[r]) % 16
            self.base.append(bases)
            self.view.append(views)
        self.specs = specs

    def column(self, role):
        return [v[role] for v in self.view]

    def step(self, steps, lrs, betas, eps):
        exa.adam_step(self.column('param'), self.column('grad'), self.column('exp_avg'), self.column('exp_avg_sq'), steps,
                      lr=lrs, betas=betas, eps=eps)
        for h, t, lr in zip(self.host, steps, lrs):
            h['param'], h['exp_avg'], h['exp_avg_sq'] = ao.step(h['param'], h['grad'], h['exp_avg'], h['exp_avg_sq'], t=t,
                                                                 lr=lr, betas=betas, eps=eps)

    def snapshot(self):
        return [{r: b[r].cpu().numpy() for r in ROLES} for b in self.base]

    def check(self):
        """Bit-equality with the oracle and untouched guards, tensor by tensor."""
        for i, ((n, off), h, got) in enumerate(zip(self.specs, self.host, self.snapshot())):
            for r in ROLES:
                a = got[r]
                inner, guard = a[off[r]:off[r] + n], np.concatenate((a[:off[r]], a[off[r] + n:]))
                assert np.array_equal(guard.view(np.uint32), np.full(guard.size, GUARD).view(np.uint32)), (i, n, r, 'guard')
                assert np.all(np.isfinite(inner)), (i, n, r)
                bad = np.nonzero(inner.view(np.uint32) != h[r].view(np.uint32))[0]
                assert bad.size == 0, 'tensor %d (n = %d) %s: %d elements differ from the oracle, first at %d: %r vs %r' % (
                    i, n, r, bad.size, bad[0], inner[bad[0]], h[r][bad[0]])


LENGTHS = (0, 1, 3, 4, 5, C - 1, C, C + 1, 3 * C + 3)


def test_every_length_alone_and_all_together_bit_equal_to_the_oracle(dev):
    for n in LENGTHS:
        case = Case(dev, [(n, ALIGNED)], seed=n)
        case.step([1], [1e-3], (0.9, 0.999), 1e-8)
        case.step([2], [1e-3], (0.9, 0.999), 1e-8)
        case.check()
    case = Case(dev, [(n, ALIGNED) for n in LENGTHS], seed=77)
    for t in (1, 2, 3):
        case.step([t] * len(LENGTHS), [1e-3] * len(LENGTHS), (0.9, 0.999), 1e-8)
        case.check()


@pytest.mark.parametrize('role', ROLES + ('all',))
def test_a_view_one_float_into_its_allocation_takes_the_scalar_path(dev, role):
    off = dict.fromkeys(ROLES, 1) if role == 'all' else dict(ALIGNED, **{role: 1})
    specs = [(n, off) for n in LENGTHS] + [(C + 7, ALIGNED), (2 * C + 1, off)]
    case = Case(dev, specs, seed=3)
    for t in (1, 2):
        case.step([t] * len(specs), [2e-3] * len(specs), (0.9, 0.999), 1e-15)
        case.check()


def _mixed(count):
    """``count`` tensors, short ones (and empty ones) between long ones, some of them misaligned."""
    pattern = (C + 1, 3, 0, 2 * C + 5, 1, 128, 0, 5, C, 4, C - 1, 55)
    specs = []
    for i in range(count):
        off = dict(ALIGNED, **({ROLES[i % 4]: 4 + (i % 3) + 1} if i % 5 == 2 else {}))
        specs.append((pattern[i % len(pattern)], off))
    return specs


@pytest.mark.parametrize('count', (1, 63, 64, 65, 130))
def test_segment_counts_across_the_launch_boundary(dev, count):
    specs = _mixed(count)
    case = Case(dev, specs, seed=count)
    lrs = [(1e-3, 0.0, 5e-2)[i % 3] for i in range(count)]
    steps = [(1, 2, 1000, 7)[i % 4] for i in range(count)]
    case.step(steps, lrs, (0.9, 0.999), 1e-15)
    case.step([t + 1 for t in steps], lrs, (0.9, 0.999), 1e-15)
    case.check()


@pytest.mark.parametrize('betas', ((0.9, 0.999), (0.4, 0.9)))
@pytest.mark.parametrize('eps', (1e-15, 1e-8))
def test_steps_eps_betas_and_learning_rates(dev, betas, eps):
    specs = [(C + 3, ALIGNED), (130, ALIGNED), (2 * C, dict(ALIGNED, grad=1)), (7, ALIGNED)]
    for t in (1, 2, 1000):
        case = Case(dev, specs, seed=t)
        before = [h['param'].copy() for h in case.host]
        moments = [h['exp_avg'].copy() for h in case.host]
        lrs = [1e-3, 0.0, 0.0, 1.6e-4]
        case.step([t, t, t + 1, 1], lrs, betas, eps)
        case.check()
        got = case.snapshot()
        for i in (1, 2):                # lr = 0: the parameter keeps its bits, the moments still move
            off, n = specs[i][1], specs[i][0]
            assert np.array_equal(got[i]['param'][off['param']:off['param'] + n].view(np.uint32), before[i].view(np.uint32))
            assert not np.array_equal(got[i]['exp_avg'][off['exp_avg']:off['exp_avg'] + n], moments[i])


@pytest.mark.parametrize('eps', (1e-15, 1e-8))
def test_zero_gradients_over_zero_moments_stay_finite(dev, eps):
    specs = [(C + 2, ALIGNED), (9, dict(ALIGNED, param=1))]
    case = Case(dev, specs, seed=11, zero=True)
    before = [h['param'].copy() for h in case.host]
    case.step([1, 1], [1e-2, 1e-2], (0.9, 0.999), eps)
    case.check()
    for h, b in zip(case.host, before):                          # what the oracle (= the kernel, bit for bit) made of them
        z = h['grad'] == 0
        assert z.any() and np.all(h['exp_avg'][z] == 0) and np.all(h['exp_avg_sq'][z] == 0)
        assert np.array_equal(h['param'][z], b[z]) and not np.array_equal(h['param'][~z], b[~z])
    case.step([2, 2], [1e-2, 1e-2], (0.9, 0.999), eps)
    case.check()


def test_two_runs_from_the_same_state_give_the_same_bits(dev):
    specs = _mixed(70)
    runs = []
    for _ in range(2):
        case = Case(dev, specs, seed=5)
        exa.adam_step(case.column('param'), case.column('grad'), case.column('exp_avg'), case.column('exp_avg_sq'),
                      [3] * 70, lr=[1e-3] * 70, eps=1e-15)
        runs.append(case.snapshot())
    for a, b in zip(*runs):
        for r in ROLES:
            assert np.array_equal(a[r].view(np.uint32), b[r].view(np.uint32))


def test_adam_step_makes_a_strided_gradient_contiguous_and_refuses_aliases(dev):
    rs = np.random.RandomState(2)
    p, g, m, v = (torch.from_numpy(a).to(dev) for a in _values(rs, 12))
    p, m, v = p.view(4, 3), m.view(4, 3), v.view(4, 3)
    gt = g.view(3, 4).t()                                        # [4, 3], not contiguous
    want = ao.step(p.cpu().numpy(), gt.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), t=1, lr=1e-3)
    exa.adam_step([p], [gt], [m], [v], [1], lr=1e-3)
    for got, w in zip((p, m, v), want):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), np.ascontiguousarray(w).view(np.uint32))
    big = torch.zeros(64, device=dev)
    ok = lambda: torch.zeros(16, device=dev)      # noqa: E731
    before = big.clone()
    with pytest.raises(ValueError, match=r'adam_step: params\[0\] and exp_avgs\[0\] share memory'):
        exa.adam_step([big[:16]], [ok()], [big[8:24]], [ok()], [1], lr=1e-3)
    with pytest.raises(ValueError, match=r'adam_step: params\[0\] and params\[1\] share memory'):
        exa.adam_step([big[:16], big[:16]], [ok(), ok()], [ok(), ok()], [ok(), ok()], [1, 1], lr=1e-3)
    with pytest.raises(ValueError, match=r'share memory'):
        exa.adam_step([ok()], [big[:16]], [ok()], [big[15:31]], [1], lr=1e-3)
    assert torch.equal(big, before)
    exa.adam_step([big[:16], big[16:32]], [big[32:48], big[32:48]], [ok(), ok()], [ok(), ok()], [1, 1], lr=1e-3)   # a shared
    #                                                                         gradient is only read: allowed
    with pytest.raises(RuntimeError, match=r'adam_step runs on a ROCm device only'):
        exa.adam_step([ok()], [torch.zeros(16)], [ok()], [ok()], [1], lr=1e-3)


# ---- Adam.step() on the small copy of the reference's grouping
@pytest.fixture(scope='module')
def grouping():
    init, lrs, grads = ao.grouping_case()
    runs = {}
    for dtype in (torch.float64, torch.float32):
        params, opt = ao.make_optimizer(torch.optim.Adam, init, lrs, dtype, 'cpu')
        ao.run(opt, params, grads, dtype)
        runs[dtype] = {n: p.detach().numpy() for n, p in params.items()}
    e32 = {n: ao.max_err(runs[torch.float32][n], runs[torch.float64][n]) for n in init}
    return init, lrs, grads, runs[torch.float64], e32


def _within(params, grouping, label):
    init, _, _, ref64, e32 = grouping
    for n, p in params.items():
        got = p.detach().cpu().numpy()
        if n.endswith('_%d' % ao.IDLE_FRAME):
            assert np.array_equal(got.view(np.uint32), init[n].view(np.uint32)), (label, n)
            continue
        err = ao.max_err(got, ref64[n])
        print('%-10s %-24s e32 %.3e  err %.3e  ratio %.3f' % (label, n, e32[n], err, err / e32[n]))
        assert err <= FACTOR * e32[n], (label, n, err, e32[n])


def test_adam_step_against_torch_on_the_references_grouping(dev, grouping):
    init, lrs, grads, _, _ = grouping
    params, opt = ao.make_optimizer(exa.Adam, init, lrs, torch.float32, dev)
    ctrl_params, ctrl = ao.make_optimizer(torch.optim.Adam, init, lrs, torch.float32, dev)
    ao.run(opt, params, grads, torch.float32)
    ao.run(ctrl, ctrl_params, grads, torch.float32)
    _within(params, grouping, 'hip')
    _within(ctrl_params, grouping, 'torch')
    oracle, _ = ao.oracle_run(init, lrs, grads)
    for (n, p), group, cgroup in zip(params.items(), opt.param_groups, ctrl.param_groups):
        assert group['name'] == n and group['params'][0] is p
        if n.endswith('_%d' % ao.IDLE_FRAME):
            assert p not in opt.state and cgroup['params'][0] not in ctrl.state       # no state, no 'step'
            continue
        assert np.array_equal(p.detach().cpu().numpy().view(np.uint32), oracle[n].view(np.uint32)), n
        st, cst = opt.state[p], ctrl.state[cgroup['params'][0]]
        assert list(st) == list(cst) == ['step', 'exp_avg', 'exp_avg_sq']
        assert st['step'].dtype == cst['step'].dtype == torch.float32 and st['step'].device.type == 'cpu'
        assert float(st['step']) == float(cst['step']) == ao.STEPS
        assert st['exp_avg'].device == p.device and st['exp_avg'].shape == p.shape


def test_state_dicts_cross_between_the_classes_mid_run(dev, grouping):
    init, lrs, grads, _, _ = grouping
    for first_cls, second_cls, label in ((exa.Adam, torch.optim.Adam, 'hip>torch'), (torch.optim.Adam, exa.Adam, 'torch>hip')):
        params, opt = ao.make_optimizer(first_cls, init, lrs, torch.float32, dev)
        ao.run(opt, params, grads[:2], torch.float32)
        sd = opt.state_dict()
        assert len(sd['state']) == len(init) - len(ao.FRAME)
        values = {n: p.detach().cpu().numpy() for n, p in params.items()}
        params2, opt2 = ao.make_optimizer(second_cls, values, lrs, torch.float32, dev)
        opt2.load_state_dict(sd)
        ao.run(opt2, params2, grads[2:], torch.float32)
        _within(params2, grouping, label)
        for group in opt2.param_groups:
            p = group['params'][0]
            if group['name'].endswith('_%d' % ao.IDLE_FRAME):
                assert p not in opt2.state
            else:
                assert float(opt2.state[p]['step']) == ao.STEPS


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def test_a_step_after_load_state_dict_reads_the_live_groups(dev):
    """Step, load a state dict (torch replaces every group dict), change ``group['lr']`` as ``Trainer.set_lr`` does: the
    next step uses that learning rate and the loaded step count -- bit for bit the oracle's."""
    rs = np.random.RandomState(21)
    init = {'a': rs.randn(C + 3).astype(np.float32), 'b': rs.randn(7, 3).astype(np.float32)}
    grads = [{n: rs.randn(*a.shape).astype(np.float32) for n, a in init.items()} for _ in range(3)]
    lrs = {'a': 1e-3, 'b': 2e-3}
    params, opt = ao.make_optimizer(exa.Adam, init, lrs, torch.float32, dev)
    ao.run(opt, params, grads[:2], torch.float32)
    sd = opt.state_dict()
    old_groups = list(opt.param_groups)
    opt.load_state_dict(sd)
    assert all(a is not b for a, b in zip(old_groups, opt.param_groups))
    new_lrs = {'a': 0.25, 'b': 0.0}
    for group in opt.param_groups:
        group['lr'] = new_lrs[group['name']]
    ao.run(opt, params, grads[2:], torch.float32)
    mid, state = ao.oracle_run(init, lrs, grads[:2])
    want, state = ao.oracle_run(mid, new_lrs, grads[2:], state=state)
    for n, p in params.items():
        assert np.array_equal(_bits(p), want[n].view(np.uint32)), n
        assert np.array_equal(_bits(opt.state[p]['exp_avg']), state[n][0].view(np.uint32))
        assert float(opt.state[p]['step']) == 3.0
    assert np.array_equal(_bits(params['b']), mid['b'].view(np.uint32))             # lr = 0 was read, not the stale 2e-3


def test_adam_step_method_with_a_strided_grad_and_a_failing_launch(dev, monkeypatch):
    rs = np.random.RandomState(22)
    p0 = rs.randn(4, 3).astype(np.float32)
    g = rs.randn(3, 4).astype(np.float32)
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(dev))
    q = torch.nn.Parameter(torch.ones(5, device=dev))           # a second tensor whose state does not exist yet
    opt = exa.Adam([{'params': [p], 'lr': 1e-2}, {'params': [q], 'lr': 1e-2}], lr=0.0, eps=1e-15)
    p.grad = torch.from_numpy(g).to(dev).t()                    # [4, 3], not contiguous
    assert not p.grad.is_contiguous()
    opt.step()
    want = ao.step(p0, np.ascontiguousarray(g.T), np.zeros_like(p0), np.zeros_like(p0), t=1, lr=1e-2, eps=1e-15)
    for got, w in zip((p, opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq']), want):
        assert np.array_equal(_bits(got), w.view(np.uint32))
    assert not p.grad.is_contiguous() and q not in opt.state
    # a C call that raises: no step count advances, no state appears, nothing is written
    def refuse(*args):
        raise RuntimeError('exa_raster: adam: refused')
    monkeypatch.setattr(optim, '_launch', refuse)
    q.grad = torch.ones(5, device=dev)
    before = _bits(p).copy()
    with pytest.raises(RuntimeError, match='adam: refused'):
        opt.step()
    assert float(opt.state[p]['step']) == 1.0 and q not in opt.state and len(opt.state) == 1
    assert np.array_equal(_bits(p), before) and bool((q.detach() == 1).all())
    monkeypatch.undo()
    opt.step()
    assert float(opt.state[p]['step']) == 2.0 and float(opt.state[q]['step']) == 1.0 and bool((q.detach() < 1).all())


# ---- densify_and_prune carries the state of either optimizer class
P0, N_CLONE, N_SPLIT, N_PRUNE = 2000, 100, 50, 20


@pytest.mark.parametrize('cls', (exa.Adam, torch.optim.Adam), ids=('hip', 'torch'))
def test_densify_and_prune_carries_the_state(dev, cls):
    rs = np.random.RandomState(9)
    f = lambda a: torch.nn.Parameter(torch.from_numpy(np.asarray(a, np.float32)).to(dev))      # noqa: E731
    scale = np.full((P0, 3), -6.0)
    scale[N_CLONE:N_CLONE + N_SPLIT] = 0.0                        # big: exp(0) = 1 > 0.01 * extent
    opacity = np.full((P0, 1), 3.0)
    opacity[200:200 + N_PRUNE] = -9.0                             # sigmoid < 0.005
    quat = rs.randn(P0, 4)
    params = {'mean': f(rs.randn(P0, 3)), 'scale': f(scale), 'rotation': f(quat / np.linalg.norm(quat, axis=1, keepdims=True)),
              'opacity': f(opacity), 'feature_rest': f(rs.randn(P0, 15, 3)), 'tag': f(np.arange(P0)[:, None])}
    opt = cls([{'params': [p], 'name': n, 'lr': 0.0 if n in ('tag', 'scale', 'opacity') else 1e-3} for n, p in params.items()],
              lr=0.0, eps=1e-15)
    for p in params.values():
        p.grad = torch.from_numpy(rs.randn(*p.shape).astype(np.float32)).to(dev) + 0.5
    opt.step()
    assert torch.equal(params['tag'].detach().cpu(), torch.arange(P0, dtype=torch.float32)[:, None])      # lr = 0
    old = {n: {k: opt.state[p][k].clone() for k in ('exp_avg', 'exp_avg_sq')} for n, p in params.items()}
    accum = torch.zeros(P0, 1, device=dev)
    accum[:N_CLONE + N_SPLIT] = 1.0
    new, n_cloned, n_split, n_pruned = densify.densify_and_prune(
        params, opt, accum, torch.ones(P0, 1, device=dev), grad_thr=0.5, extent=10.0,
        generator=torch.Generator(device=dev).manual_seed(1))
    assert (n_cloned, n_split, n_pruned) == (N_CLONE, N_SPLIT, N_PRUNE)
    n_kept = P0 - N_SPLIT - N_PRUNE
    total = n_kept + N_CLONE + 2 * N_SPLIT
    tag = new['tag'].detach()[:, 0].long()
    assert tag.numel() == total and torch.equal(tag[:n_kept], torch.sort(tag[:n_kept]).values) and int(tag[n_kept - 1]) == P0 - 1
    for group in opt.param_groups:
        n, p = group['name'], group['params'][0]
        assert p is new[n] and p.shape[0] == total and params[n] not in opt.state
        st = opt.state[p]
        assert float(st['step']) == 1.0
        for k in ('exp_avg', 'exp_avg_sq'):
            assert st[k].shape == p.shape
            assert torch.equal(st[k][:n_kept], old[n][k][tag[:n_kept]]), (n, k)      # the rows follow their Gaussians
            assert old[n][k].abs().min() > 0 and not st[k][n_kept:].any(), (n, k)    # new rows start at zero
    for p in new.values():
        p.grad = torch.from_numpy(rs.randn(*p.shape).astype(np.float32)).to(dev)
    before = new['mean'].detach().clone()
    opt.step()
    for group in opt.param_groups:
        p = group['params'][0]
        assert float(opt.state[p]['step']) == 2.0 and bool(torch.isfinite(p).all())
        assert bool(torch.isfinite(opt.state[p]['exp_avg']).all()) and bool((opt.state[p]['exp_avg_sq'][n_kept:] > 0).all())
    assert not torch.equal(new['mean'].detach(), before)


def test_the_raw_c_abi_from_plain_pointers(dev):
    """What a native host does: no Optimizer object, data pointers and a stream handle."""
    lib = _lib.load()
    rs = np.random.RandomState(4)
    sizes, steps, lrs = (C + 9, 0, 17), (1, 1, 4), (1e-3, 1e-3, 5e-2)
    host = [_values(rs, n) for n in sizes]
    device = [[torch.from_numpy(a).to(dev) for a in h] for h in host]
    segs = (_lib.ExaRasterAdamSegment * 3)()
    for s, d, n, t, lr in zip(segs, device, sizes, steps, lrs):
        s.param, s.grad, s.exp_avg, s.exp_avg_sq = (x.data_ptr() if n else None for x in d)
        s.n = n
        s.step_size, s.bc2_sqrt = ao.scalars(t, lr, 0.9, 0.999)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    rc = lib.exa_raster_adam_step(segs, 3, 0.9, 0.999, 1e-15, ctypes.c_void_p(stream.cuda_stream))
    assert rc == 0, lib.exa_raster_last_error()
    stream.synchronize()
    for h, d, t, lr in zip(host, device, steps, lrs):
        p, m, v = ao.step(*h, t=t, lr=lr, eps=1e-15)
        for got, want in zip((d[0], d[2], d[3]), (p, m, v)):
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(d[1].cpu().numpy(), h[1])


def test_step_under_a_stream_capture_raises_and_leaves_the_capture_usable(dev):
    p = torch.nn.Parameter(torch.ones(C + 5, device=dev))
    opt = exa.Adam([p], lr=1e-2)
    x = torch.arange(8, dtype=torch.float32, device=dev)
    q, g, m, v = (torch.zeros(16, device=dev) for _ in range(4))      # the functional form's tensors, allocated before the capture
    p.grad = torch.ones_like(p)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = x * 2
        with pytest.raises(RuntimeError, match='Adam.step: the step count and the learning rate travel by value'):
            opt.step()
        with pytest.raises(RuntimeError, match='adam_step: the step count and the learning rate travel by value'):
            exa.adam_step([q], [g], [m], [v], [1], lr=1e-3)
        z = y + 1
    assert len(opt.state) == 0 and not q.any() and not m.any()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(z.cpu(), torch.arange(8, dtype=torch.float32) * 2 + 1)
    assert torch.equal(p.detach().cpu(), torch.ones(C + 5))
    opt.step()                                                  # and outside the capture it steps
    assert float(opt.state[p]['step']) == 1.0 and bool((p.detach() < 1).all())

