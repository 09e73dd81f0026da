#!/usr/bin/env python3
"""Cost of adaptive sampling on config 2 (disney_spheres 1800x800, mis).  Blocking calls, host
wall clock around them, after a warm-up; one JSON line per measurement.
  1. render_adaptive to `target` (steps of `step`, cap `cap`): wall time, total samples, launches, the histogram
     of the counts - against the uniform progressive render, in the same steps, to the same worst-pixel error
     (the largest error among the pixels the adaptive run left below its cap; pixels at the cap count for
     neither).
  2. One masked step of `step` samples as a function of the active share: random masks over an accumulator
     that stands at 2 * step everywhere, timed one at a time (reset and two plain increments between).
Usage: adaptive_cost.py [target=0.05] [step=16] [cap=512]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import scenes
from vimg_amd import hip

hip.init(0)
target = float(sys.argv[1]) if len(sys.argv) > 1 else 0.05
step = int(sys.argv[2]) if len(sys.argv) > 2 else 16
cap = int(sys.argv[3]) if len(sys.argv) > 3 else 512
s = scenes.json_scene("disney_spheres.json")
w, h = s.resolution
p = s.default_params()
d = hip.DeviceScene(s)
out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
acc = d.progressive(p)
acc.render(step, out=out)                                         # warm-up
acc.render(step, out=out, mask=torch.ones((h, w), dtype=torch.uint8, device="cuda"))

# ---- 1. adaptive against uniform
acc.reset()
steps = []
t0 = time.perf_counter()
acc.render_adaptive(target, step, cap, out=out, progress=lambda n, a: steps.append((n, a, time.perf_counter() - t0)))
t_adaptive = time.perf_counter() - t0
counts, err = acc.counts(), acc.error()
below = counts < cap
worst = float(err[below].max()) if bool(below.any()) else 0.0
hist = {int(k): int(v) for k, v in zip(*torch.unique(counts, return_counts=True))}
print(json.dumps({"run": "adaptive", "target": target, "step": step, "cap": cap, "ms": round(t_adaptive * 1e3, 1),
                  "samples_total": int(counts.sum()), "mean_spp": round(float(counts.float().mean()), 2),
                  "launches": acc.launches, "pixels_at_cap": int((~below).sum()), "worst_error_below_cap": worst,
                  "counts": hist, "steps": [(n, a, round(t * 1e3, 1)) for n, a, t in steps]}), flush=True)
acc.reset()
t0 = time.perf_counter()
n = 0
while n < cap:
    acc.render(step, out=out)
    n += step
    if n >= 2 * step and float(acc.error()[below].max() if bool(below.any()) else 0.0) <= worst:
        break
t_uniform = time.perf_counter() - t0
print(json.dumps({"run": "uniform to the same worst error (over the same pixels)", "spp": n, "ms": round(t_uniform * 1e3, 1),
                  "samples_total": n * w * h, "adaptive_over_uniform_time": round(t_adaptive / t_uniform, 3),
                  "adaptive_over_uniform_samples": round(int(counts.sum()) / (n * w * h), 3)}), flush=True)

# ---- 2. a masked step by active share
g = torch.Generator(device="cuda").manual_seed(1)
rnd = torch.rand((h, w), device="cuda", generator=g)
for share in (1.0, 0.5, 0.25, 0.1, 0.03, 0.01, 0.001, 0.0):
    acc.reset()
    acc.render(step, out=False)
    acc.render(step, out=False)
    mask = (rnd < share).to(torch.uint8)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    acc.render(step, out=out, mask=mask)
    t = time.perf_counter() - t0
    print(json.dumps({"run": "masked step", "share": share, "active": int(mask.sum()), "samples": step,
                      "ms": round(t * 1e3, 2)}), flush=True)
acc.reset()
acc.render(step, out=False)
t0 = time.perf_counter()
acc.render(step, out=out)
print(json.dumps({"run": "plain step (no mask)", "samples": step, "ms": round((time.perf_counter() - t0) * 1e3, 2)}), flush=True)
t0 = time.perf_counter()
_, active = acc.select(target, cap)
print(json.dumps({"run": "select", "active": active, "ms": round((time.perf_counter() - t0) * 1e3, 2)}), flush=True)
