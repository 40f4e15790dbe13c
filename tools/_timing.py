"""What the tools/gpu_*_times.py scripts share: HIP-event medians after a warm-up and the one JSON line they print."""
import json
import os

import torch


def median_ms(fn, reps, warmup):
    """Median milliseconds of one call, each between two HIP events of its own."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e))
    times.sort()
    return times[len(times) // 2]


def window_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def medians(fns, reps, iters, warmup=10):
    """Median per-call milliseconds of every function, their windows interleaved."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(window_ms(fn, iters))
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}, {k: (min(v), max(v)) for k, v in times.items()}


def emit(res, out=None):
    """Print ``res`` as one JSON line; ``out`` names a file that gets the line too."""
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(line + '\n')
