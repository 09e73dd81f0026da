#!/usr/bin/env python3
"""Cost of progressive rendering (DESIGN.md 4.2 "Progressive rendering"): config 2 (disney_spheres 1800x800,
mis) rendered as one 512 spp launch, as 8 x 64 and as 16 x 32 spp increments of one accumulator.  Every
call is blocking, so all three are timed the same way: host wall clock around the calls, after a warm-up,
best of `reps`.  Prints one JSON line per schedule and checks the final images are bit-identical."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import scenes
from vimg_amd import hip

hip.init(0)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
s = scenes.json_scene("disney_spheres.json")
w, h = s.resolution
p = s.default_params(samples=512)
d = hip.DeviceScene(s)
out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
d.render(p, out=out, stats=False)                                 # warm-up
times = []
for _ in range(reps):
    t0 = time.perf_counter()
    d.render(p, out=out, stats=False)
    times.append(time.perf_counter() - t0)
best = min(times)
one = out.clone()
print(json.dumps({"schedule": "1 x 512", "ms": round(best * 1e3, 1)}), flush=True)
for k, n in ((8, 64), (16, 32)):
    acc = d.progressive(p)
    runs = []
    for _ in range(reps + 1):                                     # (the first is the warm-up)
        acc.reset()
        t = []
        for _ in range(k):
            t0 = time.perf_counter()
            acc.render(n, out=out)
            t.append(time.perf_counter() - t0)
        runs.append(t)
    t = min(runs[1:], key=sum)
    same = bool(torch.equal(out.view(torch.int32), one.view(torch.int32)))
    print(json.dumps({"schedule": f"{k} x {n}", "ms": round(sum(t) * 1e3, 1), "over_one_shot": round(sum(t) / best - 1.0, 4),
                      "per_increment_ms": [round(x * 1e3, 1) for x in t], "bit_identical": same}), flush=True)
    assert same
    acc.close()
