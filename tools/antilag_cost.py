#!/usr/bin/env python3
"""Cost of the anti-lag pass on disney_spheres at 1800 x 800 and 1366 x 768, mis at 4 spp:
  rescale     antilag.rescale (pair + scale) at the library's defaults and at radius 1 / 2 / 8, on the history of one
              frame against the frame of a camera one orbit step on, device events around each call
  beside it   the same session's temporal.accumulate on those frames and one a-trous iteration
  frame       a whole TemporalPreview.frame() after set_camera, with and without antilag, by the host clock around
              synchronised calls, the two previews alternating between two cameras
Medians of `steps` calls after two warm-up calls.  Prints tables to stderr and one JSON line.

  tools/antilag_cost.py [--steps N]"""
import argparse, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7)
args = ap.parse_args()

import numpy as np
import torch
import scenes
from vimg_amd import antilag, filter as flt, hip, temporal
from _timing import timed, wall

EYE, AT, VFOV, DEGREES = np.array((0.0, 20.0, 1600.0)), np.array((0.0, -4.0, 0.0)), 25.0, 1.5


def orbit_camera(i):
    pivot = EYE + 1.7 * (AT - EYE)
    a, r = math.radians(DEGREES * i), EYE - pivot
    eye = pivot + np.array([r[0] * math.cos(a) + r[2] * math.sin(a), r[1], -r[0] * math.sin(a) + r[2] * math.cos(a)])
    return eye, eye + (AT - EYE), (0.0, 1.0, 0.0), VFOV


hip.init(0)
out = {"steps": args.steps, "frames": {}}
for res in ((1800, 800), (1366, 768)):
    w, h = res
    s = scenes.json_scene("disney_spheres.json", res=res)
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    shots = []
    for i in (0, 1):
        dev.set_camera(*orbit_camera(i))
        shots.append((dev.render(p, stats=False), dev.render_features(p, flt.GUIDES), temporal.world_to_pixel(dev.camera)))
    (c0, g0, m0), (c1, g1, m1) = shots
    first = temporal.accumulate(c0, g0["normal"], g0["position"], g0["depth"], world_to_pixel=m0)
    lengths = first.length.clone()
    scale = torch.empty((h, w), dtype=torch.float32, device="cuda")
    work = torch.empty((antilag.workspace_bytes(w, h),), dtype=torch.uint8, device="cuda")
    nxt = torch.empty_like(first.tensor)
    fwork = torch.empty((flt.atrous_workspace_bytes(w, h),), dtype=torch.uint8, device="cuda")
    fout = torch.empty_like(c1)
    row = {}

    def rescale(**kw):
        first.length.copy_(lengths)          # (outside the events' span only in effect: a 4-byte-per-pixel copy, timed below on its own)
        antilag.rescale(c1, g1["normal"], g1["position"], g1["depth"], first, m1, out_scale=scale, workspace=work, **kw)

    row["restore lengths (in every rescale row)"] = timed(lambda: first.length.copy_(lengths), args.steps)
    row["antilag.rescale, defaults"] = timed(rescale, args.steps)
    row["antilag.rescale, no scale frame"] = timed(lambda: (first.length.copy_(lengths), antilag.rescale(
        c1, g1["normal"], g1["position"], g1["depth"], first, m1, out_scale=False, workspace=work)), args.steps)
    for radius in (1, 2, 4, 8):
        row[f"antilag.rescale, radius {radius}"] = timed(lambda: rescale(radius=radius), args.steps)
    first.length.copy_(lengths)
    row["temporal.accumulate"] = timed(lambda: temporal.accumulate(c1, g1["normal"], g1["position"], g1["depth"], history=first,
                                                                  world_to_pixel=m1, next_history=nxt), args.steps)
    row["filter.atrous, 1 iteration"] = timed(lambda: flt.atrous(c1, g1["normal"], g1["position"], g1["depth"], albedo=g1["albedo"],
                                                                 out=fout, workspace=fwork, iterations=1), args.steps)
    previews = {"frame() after set_camera": dev.temporal_preview(p, samples=4), "frame() after set_camera, antilag": dev.temporal_preview(p, samples=4, antilag=True)}
    for pv in previews.values():
        pv.frame()

    def moved(pv):
        def go(i):
            dev.set_camera(*orbit_camera(i % 2))
            pv.frame()
        return go

    frame_ms = {k: wall(moved(pv), args.steps) for k, pv in previews.items()}
    for pv in previews.values():
        pv.close()
    dev.close()
    out["frames"][f"{w}x{h}"] = {"device_ms_median_best": row, "wall_ms": frame_ms}
    print(f"{w} x {h}", file=sys.stderr)
    for k, (med, best) in row.items():
        print(f"  {k:44} median {med:.4f} best {best:.4f} ms", file=sys.stderr)
    for k, v in frame_ms.items():
        print(f"  {k:44} {v:.3f} ms by the host clock", file=sys.stderr)
print(json.dumps(out))
