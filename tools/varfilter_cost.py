#!/usr/bin/env python3
"""Cost of the variance-guided a-trous filter on disney_spheres at 1800 x 800: a 16 spp mis frame in
four increments with the accumulator's variance (nothing to estimate) and a 4 spp frame without one (every live pixel
estimated), with their four feature frames, at the library's defaults and 1 .. 6 iterations - and, in the same session,
filter.atrous on the same frame and one Progressive.render(16).
  whole calls   device events around varfilter.atrous (pack + estimate + k iterations + unpack) and around
                filter.atrous (pack + k iterations + unpack), alternating, median and best of `steps` calls after two
                warm-up calls
  per kernel    the kernels' own durations from torch.profiler's device trace of `steps` 5-iteration calls of each
                filter (median per launch position), when the profiler records them
  the condition the whole 5-iteration call against one 16 spp mis increment; and the ratio of one variance-guided
                iteration to one a-trous iteration, from the same run
Prints a table to stderr and one JSON line.

  tools/varfilter_cost.py [--steps N] [--no-profiler]"""
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
from vimg_amd import filter as flt, hip, varfilter
from _timing import timed

# bytes per pixel requested: the a-trous figures (tools/filter_cost.py) and what this filter adds - the variance frame in
# pack and unpack, 49 taps x (2 guides x 16 B + 12 B of colour) in the estimate where it runs, and in an iteration the
# prefilter's tile: 66 x 6 cells of 2 dwords per workgroup of 256 pixels, 12 B per pixel
BYTES = {"pack": 5 * 12 + 4 + 3 * 16, "estimate": 49 * (2 * 16 + 12) + 4, "iteration": 25 * 3 * 16 + 12 + 16,
         "unpack": 16 + 12 + 12 + 4}


def kernel_times(fn, steps, names, marker):
    """{stage: median ms} from the device trace: each call is the kernels `names`, in that order."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
    dt = lambda e: getattr(e, "device_time", None) or getattr(e, "cuda_time", 0)      # (the name changed between torch releases)
    ev = sorted((e for e in prof.events() if marker in e.name and dt(e) > 0), key=lambda e: e.time_range.start)
    per = len(names)
    if len(ev) != steps * per:
        return None
    return {name: float(np.median([dt(ev[c * per + k]) for c in range(steps)])) / 1e3 for k, name in enumerate(names)}


def profiled(fn, names, marker):
    if args.no_profiler:
        return None
    try:
        return kernel_times(fn, args.steps, names, marker)
    except Exception as e:      # (a build of torch without the device tracer)
        return {"profiler_error": repr(e)}


hip.init(0)
w, h = 1800, 800
s = scenes.json_scene("disney_spheres.json", res=(w, h))
dev = hip.DeviceScene(s)
p = s.default_params(integrator="mis", samples=4)
g = dev.render_features(p, flt.GUIDES)
acc = dev.progressive(p)
noisy4 = acc.render(4)
for _ in range(3):
    noisy16 = acc.render(4)
var16 = acc.variance()
work = torch.empty(varfilter.workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
result, result_v = torch.empty_like(noisy16), torch.empty_like(var16)
guided = lambda k, c=noisy16, v=var16: varfilter.atrous(c, g["normal"], g["position"], g["depth"], albedo=g["albedo"], variance=v,
                                                        iterations=k, out=result, out_variance=result_v, workspace=work)
fixed = lambda k: flt.atrous(noisy16, g["normal"], g["position"], g["depth"], albedo=g["albedo"], iterations=k, out=result,
                             workspace=work)
out = {"steps": args.steps, "size": f"{w}x{h}", "bytes_per_pixel": BYTES, "live_fraction": float((g["depth"][..., 0] > 0).float().mean()),
       "guided_ms": {}, "guided_estimating_ms": {}, "fixed_ms": {}}
for k in range(1, 7):       # alternating: the two filters see the same machine
    out["guided_ms"][k] = timed(lambda: guided(k), args.steps)
    out["fixed_ms"][k] = timed(lambda: fixed(k), args.steps)
    out["guided_estimating_ms"][k] = timed(lambda: guided(k, noisy4, None), args.steps)
stages = lambda lead: lead + [f"iteration {i} (step {1 << i})" for i in range(5)] + ["unpack"]
out["guided_kernel_ms"] = profiled(lambda: guided(5), stages(["pack", "estimate"]), "varfilter_")
out["guided_estimating_kernel_ms"] = profiled(lambda: guided(5, noisy4, None), stages(["pack", "estimate"]), "varfilter_")
out["fixed_kernel_ms"] = profiled(lambda: fixed(5), stages(["pack"]), "atrous_")
out["variance_ms"] = timed(lambda: acc.variance(), args.steps)
frame = torch.empty_like(noisy16)
out["mis_16spp_increment_ms"] = timed(lambda: acc.render(16, out=frame), args.steps)
acc.close()
dev.close()

print(f"{w} x {h}  ({out['live_fraction'] * 100:.1f} % live pixels, {w * h * 64 / 2 ** 20:.0f} MiB workspace)", file=sys.stderr)
for k in range(1, 7):
    (gm, gb), (fm, fb), (em, eb) = out["guided_ms"][k], out["fixed_ms"][k], out["guided_estimating_ms"][k]
    print(f"  {k} iterations: variance-guided median {gm:7.3f} ms best {gb:7.3f}   estimating {em:7.3f} / {eb:7.3f}   "
          f"a-trous {fm:7.3f} / {fb:7.3f}   ratio {gm / fm:.2f}", file=sys.stderr)
for title, key in (("variance-guided", "guided_kernel_ms"), ("variance-guided, estimating", "guided_estimating_kernel_ms"),
                   ("a-trous", "fixed_kernel_ms")):
    for name, ms in (out[key] or {}).items():
        if isinstance(ms, float):
            b = BYTES.get(name.split()[0])
            print(f"  {title:28} kernel {name:24} {ms:8.3f} ms" + (f"   {b} B/pixel -> {b * w * h / ms / 1e6:8.1f} GB/s" if b else ""),
                  file=sys.stderr)
added = lambda t: (t[6][0] - t[1][0]) / 5
out["iteration_ratio"] = added(out["guided_ms"]) / added(out["fixed_ms"])
med, best = out["mis_16spp_increment_ms"]
out["condition_filter_below_increment"] = bool(out["guided_ms"][5][0] < med)
print(f"  Progressive.variance: median {out['variance_ms'][0]:.3f} ms", file=sys.stderr)
print(f"  one added iteration (whole calls, 6 against 1): variance-guided {added(out['guided_ms']):.3f} ms, a-trous "
      f"{added(out['fixed_ms']):.3f} ms, ratio {out['iteration_ratio']:.2f}", file=sys.stderr)
print(f"  one 16 spp mis increment: median {med:8.3f} ms  best {best:8.3f} ms   variance-guided filter (5 iterations) / increment = "
      f"{out['guided_ms'][5][0] / med:.3f}", file=sys.stderr)
print(json.dumps(out))
