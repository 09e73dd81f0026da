"""The timing rules the cost tools share (filter_cost.py, temporal_cost.py)."""
import time

import numpy as np
import torch


def timed(fn, steps):
    """Median and best of `steps` calls of fn in ms, device events around each, after two warm-up calls."""
    for _ in range(2):
        fn()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms))


def wall(fn, steps):
    """Median of `steps` synchronised calls fn(i) by the host clock, in ms, after two warm-up calls."""
    ms = []
    for i in range(steps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(i)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms[2:]))
