#!/usr/bin/env python3
"""Cost of the sampling mask on disney_spheres at 450 x 200 and 1800 x 800, mis, 4 samples a frame, on
tools/temporal_cost.py's orbit, by tools/wtemporal_cost.py's protocol:
  call     one demand.mask (stride 2, a history one orbit step old, so the taps are real gathers; with and without the
           lengths and the counts) against one temporal.accumulate on the same guides and history in the same run; device
           events around each call, median and best of `steps` calls after two warm-up calls, `rounds` rounds alternating
           the calls.  Bytes per pixel against temporal's: no colour read (12 fewer), no history written (48 fewer), 1 + 4
           written.
  frame    a whole TemporalPreview.frame() - sparse=2 with the a-trous filter, with and without demand=True - after a
           set_camera and standing still, by the host clock around synchronised calls, `rounds` rounds alternating the
           previews; and the share of the pixels a moved frame samples.
Prints tables to stderr and one JSON line.

  tools/demand_cost.py [--steps N] [--rounds N]"""
import argparse, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=15)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()

import numpy as np
import torch
import scenes
from vimg_amd import demand, hip, infill, temporal
from _timing import timed, wall

NAME = "disney_spheres.json"
EYE0, AT0, VFOV = np.array((0.0, 20.0, 1600.0)), np.array((0.0, -4.0, 0.0)), 25.0


def orbit_camera(i):
    """Step i of tools/temporal_cost.py's orbit of disney_spheres, 1.5 degrees per step."""
    pivot = EYE0 + 1.7 * (AT0 - EYE0)
    a, r = math.radians(1.5 * i), EYE0 - pivot
    eye = pivot + np.array([r[0] * math.cos(a) + r[2] * math.sin(a), r[1], -r[0] * math.sin(a) + r[2] * math.cos(a)])
    return eye, eye + (AT0 - EYE0), (0.0, 1.0, 0.0), VFOV


hip.init(0)
out = {"steps": args.steps, "rounds": args.rounds, "frames": {}}
for res in ((450, 200), (1800, 800)):
    w, h = res
    s = scenes.json_scene(NAME, res=res)
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    dev.set_camera(*orbit_camera(0))
    g0 = dev.render_features(p, infill.GUIDES)
    hist = temporal.accumulate(dev.render(p, stats=False), g0["normal"], g0["position"], g0["depth"],
                               world_to_pixel=temporal.world_to_pixel(dev.camera))
    dev.set_camera(*orbit_camera(1))
    g = dev.render_features(p, infill.GUIDES)
    color = dev.render(p, stats=False)
    nxt, rgb = torch.empty_like(hist.tensor), torch.empty_like(color)
    mask, length = torch.empty((h, w), dtype=torch.uint8, device="cuda"), torch.empty((h, w), device="cuda")
    counts = demand.new_counts()
    calls = {
        "temporal.accumulate": lambda: temporal.accumulate(color, g["normal"], g["position"], g["depth"], history=hist, out=rgb,
                                                           next_history=nxt),
        "demand.mask": lambda: demand.mask(g["normal"], g["position"], g["depth"], history=hist, stride=2, phase=1, out=mask,
                                           out_length=length, counts=counts),
        "demand.mask, no lengths": lambda: demand.mask(g["normal"], g["position"], g["depth"], history=hist, stride=2, phase=1, out=mask,
                                                       out_length=False, counts=counts),
        "demand.mask, mask alone": lambda: demand.mask(g["normal"], g["position"], g["depth"], history=hist, stride=2, phase=1, out=mask,
                                                       out_length=False, counts=False),
    }
    ms = {k: [] for k in calls}
    for _ in range(args.rounds):               # alternating: other people's work shares the machine
        for k, fn in calls.items():
            ms[k].append(timed(fn, args.steps))
    torch.cuda.synchronize()
    row = {"call_ms": {k: {"median": float(np.median([m[0] for m in v])), "best": float(min(m[1] for m in v))} for k, v in ms.items()}}
    calls["demand.mask"]()
    row["counts"] = demand.read(counts)

    previews = {"sparse=2": dev.temporal_preview(p, samples=4, sparse=2), "sparse=2, demand": dev.temporal_preview(p, samples=4, sparse=2, demand=True)}
    moved, still = {k: [] for k in previews}, {k: [] for k in previews}
    for _ in range(args.rounds):
        for k, pv in previews.items():
            def after_set_camera(i, pv=pv):
                dev.set_camera(*orbit_camera(i % 2))
                pv.frame()
            moved[k].append(wall(after_set_camera, args.steps))
            still[k].append(wall(lambda i, pv=pv: pv.frame(), args.steps))
    row["frame_after_set_camera_ms"] = {k: float(np.median(v)) for k, v in moved.items()}
    row["frame_standing_still_ms"] = {k: float(np.median(v)) for k, v in still.items()}
    dev.set_camera(*orbit_camera(0))
    previews["sparse=2, demand"].frame()
    row["share_sampled_moved"] = demand.read(previews["sparse=2, demand"].last_demand[2])["masked"] / (w * h)
    for pv in previews.values():
        pv.close()
    dev.close()
    out["frames"][f"{w}x{h}"] = row
    base = row["call_ms"]["temporal.accumulate"]["median"]
    print(f"{w} x {h}   (counts of the timed call: {row['counts']})", file=sys.stderr)
    for k, v in row["call_ms"].items():
        print(f"  {k:34} median {v['median']:8.4f} ms  best {v['best']:8.4f} ms   ({v['median'] / base:.3f} of temporal.accumulate)",
              file=sys.stderr)
    for what in ("frame_after_set_camera_ms", "frame_standing_still_ms"):
        plain = row[what]["sparse=2"]
        print(f"  {what:34} " + "   ".join(f"{k} {v:8.3f} ms ({v / plain:.3f})" for k, v in row[what].items()), file=sys.stderr)
    print(f"  a moved frame with demand samples {100 * row['share_sampled_moved']:.1f} % of the pixels", file=sys.stderr)
print(json.dumps(out))
