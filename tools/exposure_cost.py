#!/usr/bin/env python3
"""Cost of the auto-exposure at 450 x 200 and 1800 x 800, on a disney_spheres frame, mis at 4 spp:
  adapt        exposure.adapt in place on a carried state (meter + resolve + apply), meter-only (meter + resolve), and in
               place on two synthetic frames of the same size: one of a single colour - every lane of a wave adds to the
               SAME LDS word, the worst case of the meter's LDS atomics - and a log-uniform random one, the best
  beside it    temporal.accumulate against a history and despeckle.clamp in place, in the same run: adapt moves 12 B in
               and 12 B out per pixel plus 12 B in for the meter, temporal.accumulate is the yardstick
Device events around each call; medians of `steps` calls after two warm-up calls, `rounds` rounds alternating the forms
(other people's work shares the machine).  A call of a few microseconds of device work is bounded by what the host needs
to enqueue it, so every form is also timed as `batch` calls back to back between one pair of events, per call: that is
the device's own time once the queue is full.  Prints tables to stderr and one JSON line.

  tools/exposure_cost.py [--steps N] [--rounds N] [--batch N]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=15)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=50)
args = ap.parse_args()

import numpy as np
import torch
import scenes
from vimg_amd import despeckle, exposure, hip, temporal
from _timing import timed

hip.init(0)
res_out = {"steps": args.steps, "rounds": args.rounds, "batch": args.batch, "frames": {}}
for res in ((450, 200), (1800, 800)):
    w, h = res
    s = scenes.json_scene("disney_spheres.json", res=res)
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    g = dev.render_features(p, despeckle.GUIDES)
    guides = (g["normal"], g["position"], g["depth"])
    noisy = dev.render(p, stats=False)
    hist = temporal.accumulate(noisy, *guides, world_to_pixel=temporal.world_to_pixel(dev.camera))
    nxt, rgb = torch.empty_like(hist.tensor), torch.empty_like(noisy)
    work = torch.empty(despeckle.workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    flat = torch.full_like(noisy, 0.4)
    spread = torch.exp2(torch.rand((h, w, 1), device="cuda", generator=gen) * 20 - 10).expand(h, w, 3).contiguous()
    bufs = {k: v.clone() for k, v in (("rendered", noisy), ("one colour", flat), ("log-uniform", spread))}
    state = exposure.new_state()
    forms = {"adapt in place": lambda: exposure.adapt(bufs["rendered"], state=state, out=bufs["rendered"], rate_brighten=1, rate_darken=1),
             "adapt out of place, with depth": lambda: exposure.adapt(noisy, g["depth"], state=state, out=rgb),
             "adapt, meter only": lambda: exposure.adapt(noisy, state=state),
             "adapt in place, one colour": lambda: exposure.adapt(bufs["one colour"], state=state, out=bufs["one colour"], rate_brighten=1, rate_darken=1),
             "adapt in place, log-uniform": lambda: exposure.adapt(bufs["log-uniform"], state=state, out=bufs["log-uniform"], rate_brighten=1, rate_darken=1),
             "temporal.accumulate with a history": lambda: temporal.accumulate(noisy, *guides, history=hist, out=rgb, next_history=nxt),
             "despeckle.clamp in place": lambda: despeckle.clamp(rgb, *guides, albedo=g["albedo"], out=rgb, out_code=False, workspace=work)}

    def batched(fn):
        def run():
            for _ in range(args.batch):
                fn()
        return run

    ms = {k: [] for k in forms}
    per = {k: [] for k in forms}
    for _ in range(args.rounds):               # alternating: other people's work shares the machine
        for k, fn in forms.items():
            ms[k].append(timed(fn, args.steps))
            per[k].append(timed(batched(fn), max(3, args.steps // 3))[0] / args.batch)
    torch.cuda.synchronize()
    row = {"calls_ms": {k: {"median_ms": float(np.median([m[0] for m in ms[k]])), "best_ms": float(min(m[1] for m in ms[k])),
                           "back_to_back_ms": float(np.median(per[k]))} for k in forms}}
    yard = row["calls_ms"]["temporal.accumulate with a history"]
    row["adapt_over_accumulate"] = {k: row["calls_ms"]["adapt in place"][k] / yard[k] for k in ("median_ms", "back_to_back_ms")}
    row["state"] = exposure.read(state)
    dev.close()
    res_out["frames"][f"{w}x{h}"] = row
    print(f"{w} x {h}: adapt in place / temporal.accumulate = {row['adapt_over_accumulate']['median_ms']:.2f} per call, "
          f"{row['adapt_over_accumulate']['back_to_back_ms']:.2f} back to back", file=sys.stderr)
    for k, cell in row["calls_ms"].items():
        print(f"  {k:40} median {cell['median_ms']:.4f}  best {cell['best_ms']:.4f}  back to back {cell['back_to_back_ms']:.4f} ms", file=sys.stderr)
print(json.dumps(res_out))
