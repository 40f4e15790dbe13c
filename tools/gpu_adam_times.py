"""The optimizer step on the MI355X over the reference's parameter set at C3 size, every tensor the only member of its own
group as the reference builds them (avatar/common/nets/module.py:141-150, 320-335, 666-671):

  scene   P = 150 000 Gaussians with SH degree 3: mean, feature_dc, feature_rest, opacity, scale, rotation (six groups);
  human   two triplanes (3, 32, 128, 128), the eight nets of tests/human_case.NETS, shape_param [100], joint_offset [55, 3];
  smplx   --frames (1 000) frames x nine tensors, of which ONE frame has gradients.

One ``step()`` of

  hip           exavatar_release_amd.Adam (one launch per 64 tensors with a gradient, across all groups),
  torch         torch.optim.Adam with its default setting,
  torch_fused   torch.optim.Adam(fused=True), when this build accepts it on the device,

each over its own copy of the parameters and gradients:

  *_wall_ms     host clock per eager call: a window of --iters calls that ends in a device synchronise;
  *_queued_ms   the device time of one call by HIP events with no host time in it: a sleep kernel occupies the stream while
                the host enqueues the whole step behind it, the first event sits behind the sleep, the second behind the step
                (a call whose enqueue outlasts the sleep is repeated with a longer one and counted in *_queued_retries);
  *_idle_wall_ms  the same host clock with no gradient anywhere: the walk over the groups alone;
  *_launches    kernel, memcpy and memset records of one call on the device timeline (torch.profiler; the span of the
                Optimizer.step annotation is listed apart in *_other_device_records, and hip_device_records names every
                record of the hip step; --no-launch-counts skips them).

hip_kernel_ms is the launch alone (exa_raster_adam_step on prebuilt segments between two events, queued the same way) and
hip_bytes_per_s the 28 B per element (p, g, m, v read; p, m, v written) over it.  Medians over --reps windows with their
min / max.  Prints one JSON line; --out writes it to a file too.

    python tools/gpu_adam_times.py [--reps 15] [--iters 20] [--frames 1000] [--out adam_times.json]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import exavatar_release_amd as exa                              # noqa: E402
from exavatar_release_amd import _lib, build, optim              # noqa: E402
from tests import human_case                                    # noqa: E402
from tests.adam_oracle import FRAME, SCENE                      # noqa: E402
from _timing import emit                                        # noqa: E402

P = 150000
LR, EPS = 1e-3, 1e-15


def shapes(frames):
    """name -> shape in the reference's group order, and the names that get a gradient."""
    out = {n: (P,) + s for n, s in SCENE.items()}
    out['triplane'], out['triplane_face'] = (3, 32, 128, 128), (3, 32, 128, 128)
    for net in human_case.NETS:
        for key, shape in human_case.net_keys(net):
            out['%s.%s' % (net, key)] = shape
    out['shape_param'], out['joint_offset'] = (100,), (55, 3)
    live = list(out)
    for f in range(frames):
        for n, s in FRAME.items():
            out['smplx_%s_%d' % (n, f)] = s
    return out, live + ['smplx_%s_0' % n for n in FRAME]


def reference_groups(named):
    """The reference's groups: one per scene tensor and per SMPL-X tensor; on the human side the triplanes, each NET (all of
    its tensors in one group), shape_param and joint_offset."""
    groups, nets = [], {}
    for n, p in named.items():
        net = n.split('.')[0]
        if net in human_case.NETS:
            if net not in nets:
                nets[net] = {'params': [], 'name': net, 'lr': LR}
                groups.append(nets[net])
            nets[net]['params'].append(p)
        else:
            groups.append({'params': [p], 'name': n, 'lr': LR})
    return groups


def stats(values):
    v = sorted(values)
    return v[len(v) // 2], [v[0], v[-1]]


def wall_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


class Queued:
    """Device time of ``fn()`` with the host's enqueue time hidden behind a sleep kernel."""

    def __init__(self):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1 << 20)
        torch.cuda.synchronize()
        s.record()
        torch.cuda._sleep(1 << 24)
        e.record()
        e.synchronize()
        self.cycles_per_ms = (1 << 24) / s.elapsed_time(e)
        self.retries = 0

    def ms(self, fn, sleep_ms):
        for attempt in range(4):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            torch.cuda._sleep(int(sleep_ms * self.cycles_per_ms))
            s.record()
            fn()
            e.record()
            hidden = not s.query()          # the sleep still runs: everything of fn() waits behind it
            e.synchronize()
            if hidden:
                return s.elapsed_time(e)
            self.retries += 1
            sleep_ms *= 2
        raise SystemExit('gpu_adam_times.py: the enqueue of one step outlasts a %.0f ms sleep kernel' % sleep_ms)


def launches(fn):
    """``{name: count}`` of the device-side records of one call of ``fn`` (torch.profiler): kernels, memcpys and memsets
    by their names, and whatever else the profiler puts on the device timeline (annotation spans)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = {}
    for e in prof.events():
        if getattr(e, 'device_type', None) == torch.autograd.DeviceType.CUDA:
            names[e.name] = names.get(e.name, 0) + 1
    return names


def is_launch(name):
    """A kernel, memcpy or memset record; not the span of a ``record_function`` annotation (``Optimizer.step#...``)."""
    return not name.startswith('Optimizer.step')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--no-launch-counts', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_adam_times.py needs a ROCm device')
    dev = torch.device('cuda:0')
    shp, live = shapes(args.frames)
    gen = torch.Generator(device=dev).manual_seed(1)
    init = {n: torch.randn(s, device=dev, generator=gen) for n, s in shp.items()}
    grads = {n: torch.randn(shp[n], device=dev, generator=gen) * 1e-2 for n in live}
    elements = sum(grads[n].numel() for n in live)
    res = {'build_digest': build._digest()[:12], 'device': torch.cuda.get_device_name(0), 'torch': torch.__version__,
           'reps': args.reps, 'iters': args.iters, 'frames': args.frames, 'groups': None, 'tensors': len(shp),
           'tensors_with_grad': len(live), 'elements_with_grad': elements, 'bytes_per_step': 28 * elements}

    variants = {'hip': lambda g: exa.Adam(g, lr=0.0, eps=EPS), 'torch': lambda g: torch.optim.Adam(g, lr=0.0, eps=EPS)}
    try:
        torch.optim.Adam([torch.nn.Parameter(torch.zeros(4, device=dev))], fused=True)
        variants['torch_fused'] = lambda g: torch.optim.Adam(g, lr=0.0, eps=EPS, fused=True)
    except Exception as e:      # noqa: BLE001  (whatever this build raises: the column is reported as absent, with the reason)
        res['torch_fused_unavailable'] = '%s: %s' % (type(e).__name__, e)
    opts, named = {}, {}
    for k, make in variants.items():
        named[k] = {n: torch.nn.Parameter(a.clone()) for n, a in init.items()}
        groups = reference_groups(named[k])
        res['groups'] = len(groups)
        opts[k] = make(groups)

    def set_grads(k, on):
        for n, p in named[k].items():
            p.grad = grads[n].clone() if on and n in grads else None

    q = Queued()
    walls = {k: [] for k in opts}
    idle = {k: [] for k in opts}
    queued = {k: [] for k in opts}
    for k in opts:                      # warm-up: state creation, code objects
        set_grads(k, True)
        for _ in range(3):
            opts[k].step()
    torch.cuda.synchronize()
    sleep_ms = {k: 3.0 * wall_ms(opts[k].step, 3) + 1.0 for k in opts}
    for _ in range(args.reps):          # the variants interleaved, window by window
        for k in opts:
            walls[k].append(wall_ms(opts[k].step, args.iters))
        for k in opts:
            queued[k].append(q.ms(opts[k].step, sleep_ms[k]))
    # the launch alone: the segments of the hip optimizer's live tensors, prebuilt
    hip = opts['hip']
    segs = [optim._segment(p, p.grad, hip.state[p]['exp_avg'], hip.state[p]['exp_avg_sq'], 10.0, LR, 0.9, 0.999)
            for p, _ in hip._flat_params() if p.grad is not None]
    arr = (_lib.ExaRasterAdamSegment * len(segs))(*segs)
    lib, stream = _lib.load(), torch.cuda.current_stream(dev).cuda_stream

    def launch_only():
        _lib.check(lib.exa_raster_adam_step(arr, len(segs), 0.9, 0.999, EPS, stream))

    kernel = [q.ms(launch_only, 1.0) for _ in range(3 * args.reps)]
    res['hip_kernel_ms'], res['hip_kernel_min_max_ms'] = stats(kernel)
    res['hip_bytes_per_s'] = 28 * elements / (res['hip_kernel_ms'] * 1e-3)
    res['hip_launches_expected'] = -(-len(segs) // optim.MAX_SEGMENTS)
    if not args.no_launch_counts:
        for k in opts:
            names = launches(opts[k].step)
            res[k + '_launches'] = sum(c for n, c in names.items() if is_launch(n))
            res[k + '_other_device_records'] = {n: c for n, c in names.items() if not is_launch(n)}
            if k == 'hip':
                res['hip_device_records'] = names
    for k in opts:
        set_grads(k, False)
    for _ in range(args.reps):
        for k in opts:
            idle[k].append(wall_ms(opts[k].step, args.iters))
    for k in opts:
        res[k + '_wall_ms'], res[k + '_wall_min_max_ms'] = stats(walls[k])
        res[k + '_queued_ms'], res[k + '_queued_min_max_ms'] = stats(queued[k])
        res[k + '_idle_wall_ms'], res[k + '_idle_wall_min_max_ms'] = stats(idle[k])
    res['queued_retries'] = q.retries
    emit(res, args.out)


if __name__ == '__main__':
    main()
