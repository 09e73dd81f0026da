#!/usr/bin/env python3
"""Cost of the history clamp on disney_spheres at 450 x 200 and 1800 x 800, mis at 4 spp:
  clamp       rectify.clamp in place on a slow history of two frames beside a fast one of one, with the picture written
              and no codes, radius 1, 2, 3.  The call is in place, so from the second call on the pixels stand inside their
              bounds and only the picture is written: the usual case, the 16 bytes per clamped pixel are not in it
  beside it   temporal.accumulate - the call the preview makes once more for the fast history - in the same run: every
              figure is set against it
  frame       a whole temporal_preview.frame() with and without ``rectify=True``, the two alternating: of a standing
              camera, and of a camera that moves every frame (an orbit step, so the guides are rendered again)
Device events around each call for the library calls, the host clock around synchronised calls for frame() (a render
call waits for its launch); medians of `steps` calls after two warm-up calls, `rounds` rounds alternating the forms.
Prints tables to stderr and one JSON line.

  tools/rectify_cost.py [--steps N] [--rounds N]"""
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
from vimg_amd import hip, rectify, temporal
from _timing import timed, wall

EYE, AHEAD, PIVOT, VFOV = np.array((0.0, 20.0, 1600.0)), np.array((0.0, -24.0, -1600.0)), np.array((0.0, -20.8, -1120.0)), 25.0


def orbit_camera(i, degrees=1.5):
    a, r = math.radians(degrees * i), EYE - PIVOT
    eye = PIVOT + np.array([r[0] * math.cos(a) + r[2] * math.sin(a), r[1], -r[0] * math.sin(a) + r[2] * math.cos(a)])
    return eye, eye + AHEAD, (0.0, 1.0, 0.0), VFOV


hip.init(0)
res_out = {"steps": args.steps, "rounds": args.rounds, "frames": {}}
for res in ((450, 200), (1800, 800)):
    w, h = res
    s = scenes.json_scene("disney_spheres.json", res=res)
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    g = dev.render_features(p, ("albedo", "normal", "position", "depth"))
    guides = (g["normal"], g["position"], g["depth"])
    m = temporal.world_to_pixel(dev.camera)
    acc = dev.progressive(p)
    first, second = acc.render(4).clone(), acc.render(4).clone()
    acc.close()
    slow = temporal.accumulate(second, *guides, history=temporal.accumulate(first, *guides, world_to_pixel=m), world_to_pixel=m)
    fast = temporal.accumulate(second, *guides, world_to_pixel=m)
    keep = slow.tensor.clone()
    out, nxt = torch.empty_like(first), torch.empty_like(slow.tensor)

    forms = {f"clamp radius {r}": (lambda r=r: rectify.clamp(slow, fast, albedo=g["albedo"], out=out, radius=r, min_taps=4)) for r in (1, 2, 3)}
    forms["clamp at the defaults, with codes"] = lambda: rectify.clamp(slow, fast, albedo=g["albedo"], out=out, code=True)
    forms["temporal.accumulate"] = lambda: temporal.accumulate(second, *guides, history=fast, world_to_pixel=m, next_history=nxt, out=out)
    forms["temporal.accumulate, no picture"] = lambda: temporal.accumulate(second, *guides, history=fast, world_to_pixel=m, next_history=nxt)
    ms = {k: [] for k in forms}
    for _ in range(args.rounds):               # alternating: other people's work shares the machine
        for k, fn in forms.items():
            ms[k].append(timed(fn, args.steps))
    torch.cuda.synchronize()
    row = {"calls_ms": {k: {"median_ms": float(np.median([x[0] for x in v])), "best_ms": float(min(x[1] for x in v))} for k, v in ms.items()}}
    slow.tensor.copy_(keep)
    code = rectify.clamp(slow, fast, albedo=g["albedo"], code=True)[2]
    row["codes"] = [float((code == k).float().mean()) for k in range(4)]
    for kind in ("standing", "moved"):
        previews = {f"frame() {kind}, plain": dev.temporal_preview(p, samples=4), f"frame() {kind}, rectify": dev.temporal_preview(p, samples=4, rectify=True)}

        def frame(i, v):
            if kind == "moved":
                dev.set_camera(*orbit_camera(i % 8))
            v.frame()
        rounds = [{k: wall(lambda i, v=v: frame(i, v), args.steps) for k, v in previews.items()} for _ in range(args.rounds)]
        row.setdefault("frame_ms_median_of_rounds", {}).update({k: float(np.median([r[k] for r in rounds])) for k in previews})
        row.setdefault("frame_ms_rounds", []).append(rounds)
        for v in previews.values():
            v.close()
    dev.close()
    res_out["frames"][f"{w}x{h}"] = row
    base = row["calls_ms"]["temporal.accumulate"]["median_ms"]
    print(f"{w} x {h}: codes 0..3 at the defaults: " + " ".join(f"{100 * x:.2f} %" for x in row["codes"]), file=sys.stderr)
    for k, cell in row["calls_ms"].items():
        print(f"  {k:52} median {cell['median_ms']:.4f}  best {cell['best_ms']:.4f} ms  ({cell['median_ms'] / base:.2f} x temporal.accumulate)", file=sys.stderr)
    for k, v in row["frame_ms_median_of_rounds"].items():
        print(f"  {k:52} {v:8.3f} ms  ({v / base:.1f} x temporal.accumulate)", file=sys.stderr)
print(json.dumps(res_out))
