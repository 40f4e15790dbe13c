"""Host layer of the Gaussian rasterizer's autograd nodes (``rasterizer.py``): the pieces a plain and a composite render
share -- gradient arena, backward job, output planes, capacity policy.  Plain CPU tensors (``data_ptr()`` works there), no
library call."""
import ctypes

import pytest
import torch

from exavatar_release_amd import _lib
from exavatar_release_amd import rasterizer as rz

CPU = torch.device('cpu')
WIDTHS = (3, 3, 3, 1, 3, 4, 6)


def test_grad_arena_all_on_is_one_storage_in_the_documented_order():
    rows = 37
    *views, d_sh = rz._grad_arena(rows, (True,) * 7, False, 0, CPU)
    assert d_sh is None and len(views) == 7
    base = views[0].data_ptr()
    for v, w, off in zip(views, WIDTHS, (0, 3, 6, 9, 10, 13, 17)):
        assert v.shape == (rows, w) and v.dtype == torch.float32 and v.is_contiguous()
        assert v.untyped_storage().data_ptr() == views[0].untyped_storage().data_ptr()
        assert v.storage_offset() == rows * off and v.data_ptr() == base + 4 * rows * off
    assert views[0].untyped_storage().nbytes() == 4 * rows * 23


def test_grad_arena_partial_patterns_close_up_in_order():
    rows = 5
    want = (False, True, False, True, False, True, True)             # means2D, opacity, rotations, cov3D
    *views, d_sh = rz._grad_arena(rows, want, False, 0, CPU)
    assert [v is not None for v in views] == list(want) and d_sh is None
    on = [v for v in views if v is not None]
    assert [tuple(v.shape) for v in on] == [(rows, 3), (rows, 1), (rows, 4), (rows, 6)]
    assert [v.storage_offset() for v in on] == [0, rows * 3, rows * 4, rows * 8]
    assert len({v.untyped_storage().data_ptr() for v in on}) == 1 and on[0].untyped_storage().nbytes() == 4 * rows * 14
    assert rz._grad_arena(rows, (False,) * 7, False, 0, CPU) == [None] * 8          # all off: nothing is allocated


def test_grad_arena_d_sh_is_a_tensor_of_its_own():
    rows, M = 6, 9
    *views, d_sh = rz._grad_arena(rows, (True,) + (False,) * 6, True, M, CPU)
    assert d_sh.shape == (rows, M, 3) and d_sh.dtype == torch.float32 and d_sh.is_contiguous()
    assert d_sh.untyped_storage().data_ptr() != views[0].untyped_storage().data_ptr()
    assert views[0].untyped_storage().nbytes() == 4 * rows * 3
    only_sh = rz._grad_arena(rows, (False,) * 7, True, M, CPU)
    assert only_sh[:7] == [None] * 7 and only_sh[7].shape == (rows, M, 3)


def test_grad_arena_of_zero_rows():
    *views, d_sh = rz._grad_arena(0, (True,) * 7, True, 4, CPU)
    assert [tuple(v.shape) for v in views] == [(0, w) for w in WIDTHS] and d_sh.shape == (0, 4, 3)


INPUT_FIELDS = ('means3D', 'shs', 'colors_precomp', 'opacities', 'scales', 'rotations', 'cov3D_precomp')
GRAD_FIELDS = ('dL_dmeans3D', 'dL_dmeans2D', 'dL_dcolors', 'dL_dopacity', 'dL_dscales', 'dL_drotations', 'dL_dcov3D', 'dL_dsh')


@pytest.mark.parametrize('with_cov', [True, False])
def test_fill_backward_job_names_every_tensor_and_leaves_the_callers_fields_zero(with_cov):
    P, M, H, W = 7, 4, 5, 9
    t = lambda *shape: torch.zeros(shape)           # noqa: E731
    if with_cov:        # colours + a precomputed covariance: no shs / scales / rotations
        inputs7 = (t(P, 3), None, t(P, 3), t(P, 1), None, None, t(P, 6))
        sh_M = 0
    else:               # the reverse
        inputs7 = (t(P, 3), t(P, M, 3), None, t(P, 1), t(P, 3), t(P, 4), None)
        sh_M = M
    want = tuple(x is not None for x in (inputs7[0], True, inputs7[2], inputs7[3], inputs7[4], inputs7[5], inputs7[6]))
    dgrads8 = rz._grad_arena(P, want, inputs7[1] is not None, sh_M, CPU)
    assert [d is not None for d in dgrads8[:7]] == list(want)
    radii, grad_ws = torch.zeros(P, dtype=torch.int32), torch.zeros(64, dtype=torch.uint8)
    image_grads = (t(3, H, W), None, t(1, H, W)) if with_cov else (t(3, H, W), t(1, H, W), None)
    settings = _lib.ExaRasterSettings()
    arr = (_lib.ExaRasterBackwardJob * 1)()
    a = arr[0]
    rz._fill_backward_job(a, settings, P, sh_M, inputs7, radii, (1024, 2048, 4096), 640, image_grads, grad_ws, dgrads8)
    assert ctypes.addressof(a.settings.contents) == ctypes.addressof(settings)
    assert (a.P, a.sh_M, a.capacity) == (P, sh_M, 640)
    assert (a.geom_ws, a.tile_ws, a.bin_ws) == (1024, 2048, 4096)
    for name, x in zip(INPUT_FIELDS + GRAD_FIELDS + ('dL_dcolor', 'dL_ddepth', 'dL_dalpha', 'radii', 'grad_ws'),
                       tuple(inputs7) + tuple(dgrads8) + image_grads + (radii, grad_ws)):
        assert getattr(a, name) == (None if x is None else x.data_ptr()), name          # (a NULL c_void_p reads as None)
    assert a.dL_dcolor_indirect is None
    # what the two callers own stays as the zero-initialised structure had it
    assert (a.grad_first, a.accumulate, a.used_slots, a.compose_P_a, a.compose_capacity_b) == (0, 0, 0, 0, 0)
    assert a.compose_geom_a is None
    assert (a.densify_grad_accum, a.densify_track_cnt, a.densify_radius_max) == (None, None, None)


def test_fill_backward_job_looks_up_the_indirect_colour_gradient_while_a_backward_is_recorded():
    """``dL_dcolor_indirect``: the pointer-table entry a recorded backward reads dL/dcolor through, found by the address of the
    colour gradient in the capture scope's ``grad_ind``; a gradient the table does not name gets none."""
    P, H, W = 3, 4, 6
    inputs7 = (torch.zeros(P, 3), None, torch.zeros(P, 3), torch.zeros(P, 1), torch.zeros(P, 3), torch.zeros(P, 4), None)
    radii, grad_ws = torch.zeros(P, dtype=torch.int32), torch.zeros(64, dtype=torch.uint8)
    known, other = torch.zeros(3, H, W), torch.zeros(3, H, W)
    with rz.capture_scope(grad_ind={known.data_ptr(): 0x7000}):
        for g_color, expect in ((known, 0x7000), (other, None)):
            arr = (_lib.ExaRasterBackwardJob * 1)()
            rz._fill_backward_job(arr[0], _lib.ExaRasterSettings(), P, 0, inputs7, radii, (64, 128, 192), 64, (g_color, None, None),
                                  grad_ws, [None] * 8)
            assert arr[0].dL_dcolor == g_color.data_ptr() and arr[0].dL_dcolor_indirect == expect


# ---- the capture scope ---------------------------------------------------------------------------------------------------
def _nothing_held():
    return [rz.report_for(0), rz.report_for(0, True), rz.used_for(0), rz.used_for(0, True), rz.indirect_for(0x10)]


def test_capture_scope_accessors_return_what_was_put_in_and_none_elsewhere():
    assert rz._capture is None and _nothing_held() == [None] * 5          # no scope is active
    with rz.capture_scope(report=[(9, 1), None], report_c=[None, (11, 3)], used=([4, 5, 6], [7]), grad_ind={0x10: 0x7000}) as scope:
        assert rz._capture is scope and scope.jobs is None
        assert [rz.report_for(k) for k in range(3)] == [(9, 1), None, None]          # an entry, a None entry, past the end
        assert [rz.report_for(k, True) for k in range(3)] == [None, (11, 3), None]
        assert [rz.used_for(k) for k in range(4)] == [4, 5, 6, None]
        assert [rz.used_for(k, True) for k in range(2)] == [7, None]
        assert rz.indirect_for(0x10) == 0x7000 and rz.indirect_for(0x20) is None
        scope.report = [(10, 2)]                                                     # fields may be assigned in the body
        assert rz.report_for(0) == (10, 2) and rz.report_for(1) is None
    assert rz._capture is None and _nothing_held() == [None] * 5
    with rz.capture_scope(jobs=[]) as scope:                                         # every field left out: nothing is held
        assert _nothing_held() == [None] * 5 and scope.jobs == []
    assert rz._capture is None


def test_capture_scope_restores_config_and_removes_itself_on_every_kind_of_exit():
    cfg = rz.config
    entry = (cfg.mode, cfg.fixed_capacity, cfg.on_overflow, dict(vars(cfg)))
    state = lambda: (cfg.mode, cfg.fixed_capacity, cfg.on_overflow, dict(vars(cfg)))          # noqa: E731
    other = 'raise' if cfg.on_overflow == 'retry' else 'retry'
    with rz.capture_scope(mode='exact', fixed_capacity=None, on_overflow=other):                # a normal exit
        assert (cfg.mode, cfg.fixed_capacity, cfg.on_overflow) == ('exact', None, other)
    assert state() == entry and rz._capture is None
    with pytest.raises(KeyError, match='from the body'):                                        # an exception in the body
        with rz.capture_scope(mode='capacity', fixed_capacity=[64, 128]):
            assert (cfg.mode, cfg.fixed_capacity) == ('capacity', [64, 128])
            raise KeyError('from the body')
    assert state() == entry and rz._capture is None
    with rz.capture_scope(mode='exact', on_overflow=other):                                     # the body reassigns, as
        cfg.mode, cfg.fixed_capacity = 'capacity', [192]                                        # GraphedIteration._capture does
        assert (cfg.mode, cfg.fixed_capacity) == ('capacity', [192])
    assert state() == entry and rz._capture is None
    with rz.capture_scope(report=[(9, 1)], mode='exact') as outer:                              # scopes do not nest
        with pytest.raises(RuntimeError, match='already active'):
            with rz.capture_scope(report=[(10, 2)], mode='capacity'):
                raise AssertionError('the inner body ran')
        assert rz._capture is outer and rz.report_for(0) == (9, 1) and cfg.mode == 'exact'      # the first scope is intact
    assert state() == entry and rz._capture is None


def test_capture_scope_is_seen_from_another_thread():
    """``torch.autograd.grad`` inside a capture runs ``_Rasterize.backward`` / ``_Compose.backward`` on autograd's device thread:
    the scope is process-wide, not thread-local."""
    import threading
    seen = []
    with rz.capture_scope(used=([3], []), grad_ind={0x10: 0x7000}) as scope:
        t = threading.Thread(target=lambda: seen.append((rz._capture, rz.used_for(0), rz.indirect_for(0x10))))
        t.start()
        t.join()
    assert len(seen) == 1 and seen[0][0] is scope and seen[0][1:] == (3, 0x7000)


def test_image_grads_fill_in_a_missing_colour_and_keep_missing_planes_none():
    H, W = 5, 9
    g = torch.ones(3, H, W)
    color, depth, alpha = rz._image_grads((g, None, None, None), H, W, CPU)
    assert color is g and depth is None and alpha is None
    color, depth, alpha = rz._image_grads((None, None, torch.ones(1, H, W, dtype=torch.float64), None), H, W, CPU)
    assert color.shape == (3, H, W) and not color.any() and alpha is None
    assert depth.dtype == torch.float32 and depth.shape == (1, H, W) and depth.is_contiguous()


def test_plane_ptrs_and_outputs_of_a_ragged_image():
    H, W = 37, 53
    planes = torch.zeros(5, H, W)
    base = planes.data_ptr()
    assert rz._plane_ptrs(planes, H, W) == (base, base + 12 * H * W, base + 16 * H * W)
    color, depth, alpha = rz._plane_outputs(planes)
    assert (color.shape, depth.shape, alpha.shape) == ((3, H, W), (1, H, W), (1, H, W))
    assert (color.data_ptr(), depth.data_ptr(), alpha.data_ptr()) == rz._plane_ptrs(planes, H, W)


@pytest.fixture
def policy():
    """A temporary capacity policy: ``config`` and the capacity memo are put back afterwards."""
    cfg = rz.config
    saved = (cfg.fixed_capacity, cfg.capacity_growth, cfg.min_capacity)
    key = ('test_raster_host', 1, 2, 3)
    yield cfg, key
    cfg.fixed_capacity, cfg.capacity_growth, cfg.min_capacity = saved
    rz._seen_D.pop(key, None)


def test_capacity_for_states_the_policy_once(policy):
    cfg, key = policy
    cfg.capacity_growth, cfg.min_capacity = 1.5, 1000
    # a fixed capacity wins over what was seen: one number for every job, or one per job -- not rounded here: the Python
    # node rounds up to whole 64-instance batch slots when it carves the workspace, the compiled node rounds in C++
    rz._seen_D[key] = 5000
    cfg.fixed_capacity = 1001
    assert rz._capacity_for(key, 0) == rz._capacity_for(key, 3) == rz._capacity_for(key) == 1001
    cfg.fixed_capacity = [130, 70000.0, 64]
    assert [rz._capacity_for(key, k) for k in range(3)] == [130, 70000, 64] and rz._capacity_for(key) == 130
    assert all(type(rz._capacity_for(key, k)) is int for k in range(3))
    # no fixed capacity: what was seen x growth, at least min_capacity
    cfg.fixed_capacity = None
    rz._seen_D[key] = 600                        # 600 x 1.5 = 900 < min_capacity
    assert rz._capacity_for(key, 0) == 1000
    rz._seen_D[key] = 667                        # 1000.5: truncated, equal to the floor
    assert rz._capacity_for(key, 0) == 1000
    rz._seen_D[key] = 4001                       # 6001.5: truncated, NOT a multiple of 64
    assert rz._capacity_for(key, 1) == 6001
    # a shape nobody measured: 0 = measure it (exact mode)
    del rz._seen_D[key]
    assert rz._capacity_for(key, 0) == 0


# ---- header-report pool: slot arithmetic, waiting and release over plain host memory ---------------------------------
DEV_BASE = 0x7f0000001000
RING, TOTAL = 8, 12                  # ring slots 0..7, reserved slots 8..11


@pytest.fixture
def pool():
    p = object.__new__(rz._HdrPool)
    p.words = (ctypes.c_uint32 * (4 * TOTAL))(*range(100, 100 + 4 * TOTAL))
    p.dev_base, p.N, p.next, p.tag, p.free_reserved = DEV_BASE, RING, 0, 1, [11, 10]
    return p


class _Stream:
    """Stands in for a stream: counts ``synchronize()`` calls; ``lands`` = (pool, slot, tag) the wait makes arrive."""

    def __init__(self, lands=None):
        self.calls, self.lands = 0, lands

    def synchronize(self):
        self.calls += 1
        if self.lands is not None:
            p, slot, tag = self.lands
            p.words[4 * slot + 3] = tag


@pytest.mark.parametrize('slot', [0, 5, 9])          # first slot, a ring slot, a reserved slot
def test_pool_slot_operations_touch_the_right_words_only(pool, slot):
    before = list(pool.words)
    assert pool.addr(slot) == DEV_BASE + 16 * slot
    assert pool.read(slot) == (before[4 * slot], before[4 * slot + 1])
    assert type(pool.read(slot)[0]) is int and type(pool.read(slot)[1]) is int
    assert pool.landed(slot, before[4 * slot + 3]) and not pool.landed(slot, before[4 * slot + 3] + 1)
    assert list(pool.words) == before                # addr / read / landed write nothing
    pool.clear(slot)
    after = list(pool.words)
    assert after[4 * slot + 3] == 0 and not pool.landed(slot, before[4 * slot + 3]) and pool.landed(slot, 0)
    after[4 * slot + 3] = before[4 * slot + 3]
    assert after == before                           # every other word, the neighbouring slots' included, is untouched
    pool.words[4 * slot], pool.words[4 * slot + 1] = 77, 1
    assert pool.read(slot) == (77, 1)


def test_pool_take_and_reserve_hand_out_addr(pool):
    assert pool.take() == (0, 1, DEV_BASE) and pool.take() == (1, 2, DEV_BASE + 16)
    assert pool.reserve() == (10, 3, DEV_BASE + 160) and pool.words[43] == 0 and pool.free_reserved == [11]


def test_pool_wait_returns_a_landed_report_without_the_clock(pool, monkeypatch):
    def clock():
        raise AssertionError('the clock was consulted')
    monkeypatch.setattr(rz.time, 'perf_counter', clock)
    pool.words[4 * 9 + 3] = 41
    s = _Stream()
    assert pool.wait(9, 41, 1e-3, s) is True and s.calls == 0
    assert pool.collect([(9, 41)], 1e-3) == [(136, 137)] and pool.collect([(9, 41)], 1e-3, shared=True) == [(136, 137)]


def test_pool_wait_falls_back_on_the_stream_once(pool):
    import time
    s = _Stream(lands=(pool, 5, 41))
    t0 = time.perf_counter()
    assert pool.wait(5, 41, 1e-3, s) is True
    assert time.perf_counter() - t0 >= 1e-3 and s.calls == 1
    # a stream that does not bring the report: False, after spin_s and not before, one synchronize
    s = _Stream()
    t0 = time.perf_counter()
    assert pool.wait(5, 42, 1e-3, s) is False
    assert time.perf_counter() - t0 >= 1e-3 and s.calls == 1
    # no stream: nothing to synchronise
    t0 = time.perf_counter()
    assert pool.wait(5, 42, 1e-3) is False
    assert time.perf_counter() - t0 >= 1e-3


def test_pool_wait_with_a_deadline_in_the_past_returns_at_once(pool, monkeypatch):
    import time
    t_end = time.perf_counter() - 1.0
    polls = []
    real = time.perf_counter
    monkeypatch.setattr(rz.time, 'perf_counter', lambda: polls.append(1) or real())
    s = _Stream()
    assert pool.wait(5, 42, 10.0, s, t_end=t_end) is False and s.calls == 1
    assert len(polls) == 1                           # one look at the clock: the loop body never ran
    assert pool.wait(5, 42, 10.0, _Stream(lands=(pool, 5, 42)), t_end=t_end) is True


def test_pool_collect_reads_every_report_or_none(pool, monkeypatch):
    import time
    stream = _Stream()
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda device=None: stream)
    reports = [(8, 7), (9, 8), (10, 9)]
    pool.words[4 * 8 + 3] = 7
    # one shared budget, starting at the first report that has not landed (9; 10 never gets a budget of its own); no stream wait
    t0 = time.perf_counter()
    assert pool.collect(reports, 1e-3, shared=True) is None
    assert 1e-3 <= time.perf_counter() - t0 < 0.5 and stream.calls == 0
    # a budget per report, then the device's current stream, then give up at the first that is missing
    t0 = time.perf_counter()
    assert pool.collect(reports, 1e-3, device=torch.device('cpu')) is None
    assert time.perf_counter() - t0 >= 1e-3 and stream.calls == 1
    stream.lands = (pool, 9, 8)                      # the stream wait brings report 9; 10 has landed
    pool.words[4 * 10 + 3] = 9
    assert pool.collect(reports, 1e-3, device=torch.device('cpu')) == [(132, 133), (136, 137), (140, 141)] and stream.calls == 2
    assert pool.collect(reports, 1e-3, shared=True) == [(132, 133), (136, 137), (140, 141)]
    assert pool.collect([], 1e-3) == []


def test_pool_release_reports_skips_none_ring_and_free_slots(pool):
    assert pool.reserve()[0] == 10 and pool.free_reserved == [11]
    pool.release_reports([None, (3, 5), (10, 6), None, (10, 6), (11, 9)])
    assert sorted(pool.free_reserved) == [10, 11]
    pool.release(10)
    pool.release(2)
    assert sorted(pool.free_reserved) == [10, 11]


# ---- the trusted focal tensor of the graphed classes -------------------------------------------------------------
@pytest.fixture
def focal(pool, monkeypatch):
    """A ``_TrustedFocal`` over the fake pool; ``camera_block_device`` is replaced by a recorder that checks on the
    'device' exactly when the real one would for a float32 focal tensor (``expect`` and ``flag`` given)."""
    from exavatar_release_amd import renderer
    calls = []

    def block(cam_param, img_shape, out38, expect=None, flag=None):
        calls.append((expect, flag))
        check = expect is not None and flag is not None
        return (expect if check else (0.5, 0.4, None, 170.0, 170.0)), check
    monkeypatch.setattr(renderer, 'camera_block_device', block)
    monkeypatch.setattr(rz, '_hdr_pool', pool)
    stream = _Stream()
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda device=None: stream)
    return renderer._TrustedFocal(), calls, stream


def test_trusted_focal_protocol(pool, focal):
    tf, calls, stream = focal
    f = torch.tensor([170.0, 170.0])
    out38 = torch.zeros(38)
    # first frame: host path, verified at once, no slot
    assert tf.before({'focal': f}, (8, 8), out38) == ((0.5, 0.4), False)
    assert calls[-1] == (None, None) and pool.next == 0 and tf.src is f and tf.ver == f._version
    # same object and version: trusted, no slot taken, no device check
    assert tf.before({'focal': f}, (8, 8), out38) == ((0.5, 0.4), False)
    assert calls[-1] == (None, None) and pool.next == 0
    # a new object: a ring slot is taken, the check is pending
    g = f.clone()
    pool.words[3] = 0
    assert tf.before({'focal': g}, (8, 8), out38) == ((0.5, 0.4), True)
    assert pool.next == 1 and calls[-1] == (tf.intr, (DEV_BASE, 1)) and tf.src is f
    pool.words[0], pool.words[3] = 1, 1              # the kernel reports "unchanged" with tag 1
    assert tf.after(torch.device('cpu')) is True and tf.src is g and tf.ver == g._version and tf.intr is not None
    assert stream.calls == 0
    # the same object written in place: a new version is checked again; flag word 0 = changed: intrinsics forgotten
    g.add_(1.0)
    assert tf.before({'focal': g}, (8, 8), out38)[1] is True and pool.next == 2
    pool.words[4], pool.words[7] = 0, 2
    assert tf.after(torch.device('cpu')) is False and tf.intr is None
    # ... so the next frame goes the host path again and is verified
    assert tf.before({'focal': g}, (8, 8), out38)[1] is False and calls[-1] == (None, None) and tf.src is g and pool.next == 2
    # a report that never lands (after the spin and one stream wait): forgotten as well
    h = g.clone()
    pool.words[11] = 0
    assert tf.before({'focal': h}, (8, 8), out38)[1] is True and pool.next == 3
    assert tf.after(torch.device('cpu')) is False and tf.intr is None and stream.calls == 1 and tf.src is g


def test_pool_clear_reports_zeroes_the_tags_of_its_reports_only(pool):
    before = list(pool.words)
    pool.clear_reports([(9, 1), None, (0, 2)])
    after = list(pool.words)
    assert after[3] == 0 and after[39] == 0
    after[3], after[39] = before[3], before[39]
    assert after == before
