#!/usr/bin/env python3
"""Cost of the a-trous filter on disney_spheres at 1800 x 800 and 1366 x 768: a 4 spp mis frame and
its four feature frames, filtered with the library's defaults at 1 .. 6 iterations.
  whole calls   device events around filter.atrous (pack + k iterations + unpack), median and best of `steps` calls
                after two warm-up calls; "per added iteration" is the difference of consecutive medians
  per kernel    the pack / iteration / unpack kernels' own durations from torch.profiler's device trace of `steps`
                5-iteration calls (median per launch position), when the profiler records them
  the condition the whole 5-iteration filter at 1800 x 800 against one 16 spp mis increment of the same scene
                (Progressive.render(16), device events, same session): a preview step must not be dominated by its filter
beside the bytes each stage moves per pixel.  Prints a table to stderr and one JSON line.

  tools/filter_cost.py [--steps N] [--no-profiler]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7)
ap.add_argument("--no-profiler", action="store_true")
args = ap.parse_args()

import numpy as np
import torch
import scenes
from vimg_amd import filter as flt, hip
from _timing import timed

# bytes per pixel: pack reads 4 or 5 frames of 12 B and writes 3 planes of 16 B; an iteration reads its own 3 x 16 B
# and up to 24 taps x 3 x 16 B (through L2: neighbouring lanes and rows share them) and writes 16 B; unpack reads 16 B
# + the albedo and writes 12 B
BYTES = {"pack": 5 * 12 + 3 * 16, "iteration": 25 * 3 * 16 + 16, "unpack": 16 + 12 + 12}


def kernel_times(fn, steps, iterations):
    """{stage: median ms} from the device trace: each call is pack, `iterations` iteration kernels, unpack."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
    dt = lambda e: getattr(e, "device_time", None) or getattr(e, "cuda_time", 0)      # (the name changed between torch releases)
    ev = sorted((e for e in prof.events() if "atrous_" in e.name and dt(e) > 0), key=lambda e: e.time_range.start)
    per = 2 + iterations
    if len(ev) != steps * per:
        return None
    out = {}
    for k in range(per):
        name = "pack" if k == 0 else "unpack" if k == per - 1 else f"iteration {k - 1} (step {1 << (k - 1)})"
        out[name] = float(np.median([dt(ev[c * per + k]) for c in range(steps)])) / 1e3
    return out


hip.init(0)
out = {"steps": args.steps, "bytes_per_pixel": BYTES, "sizes": {}}
for res in ((1800, 800), (1366, 768)):
    s = scenes.json_scene("disney_spheres.json", res=res)
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    noisy = dev.render(p, stats=False)
    g = dev.render_features(p, flt.GUIDES)
    w, h = res
    work = torch.empty(flt.atrous_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
    result = torch.empty_like(noisy)
    call = lambda k: flt.atrous(noisy, g["normal"], g["position"], g["depth"], albedo=g["albedo"], iterations=k, out=result,
                                workspace=work)
    row = {"whole_ms": {}, "live_fraction": float((g["depth"][..., 0] > 0).float().mean())}
    for k in range(1, 7):
        row["whole_ms"][k] = timed(lambda: call(k), args.steps)
    if not args.no_profiler:
        try:
            row["kernel_ms"] = kernel_times(lambda: call(5), args.steps, 5)
        except Exception as e:      # (a build of torch without the device tracer)
            row["kernel_ms"] = None
            row["profiler_error"] = repr(e)
    acc = dev.progressive(s.default_params(integrator="mis", samples=1))
    frame = torch.empty_like(noisy)
    row["mis_16spp_increment_ms"] = timed(lambda: acc.render(16, out=frame), args.steps)
    acc.close()
    dev.close()
    out["sizes"][f"{w}x{h}"] = row
    print(f"{w} x {h}  ({row['live_fraction'] * 100:.1f} % live pixels, {w * h * 64 / 2 ** 20:.0f} MiB workspace)", file=sys.stderr)
    prev = None
    for k, (med, best) in row["whole_ms"].items():
        added = "" if prev is None else f"   +{med - prev:.3f} for the added iteration"
        print(f"  {k} iterations: median {med:8.3f} ms  best {best:8.3f} ms{added}", file=sys.stderr)
        prev = med
    for name, ms in (row.get("kernel_ms") or {}).items():
        stage = name.split()[0]
        print(f"  kernel {name:24} {ms:8.3f} ms   {BYTES[stage]} B/pixel -> {BYTES[stage] * w * h / ms / 1e6:8.1f} GB/s", file=sys.stderr)
    med, best = row["mis_16spp_increment_ms"]
    print(f"  one 16 spp mis increment: median {med:8.3f} ms  best {best:8.3f} ms   "
          f"filter (5 iterations) / increment = {row['whole_ms'][5][0] / med:.3f}", file=sys.stderr)
big = out["sizes"]["1800x800"]
out["condition_filter_below_increment"] = bool(big["whole_ms"][5][0] < big["mis_16spp_increment_ms"][0])
print(json.dumps(out))
