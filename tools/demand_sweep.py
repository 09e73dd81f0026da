#!/usr/bin/env python3
"""What sampling on demand buys a sparse preview: the orbit of 4.24 (tools/wtemporal_sweep.py's: the eye
on a circle, 1.5 degrees per step, viewing direction kept; 8 steps, mis at 4 spp) on cornell_box_spheres (64 x 64 and
256 x 256) and disney_spheres (450 x 200), walked by DeviceScene.temporal_preview(sparse=stride, denoise=False,
demand=dict(min_history=m)) for strides 2 to 4 and min_history 0, 0.5, 1, 2, 4.  min_history 0 is the lattice alone, bit for
bit the preview without ``demand`` (tests/test_demand.py).  e = mean((x - ref)^2 / (ref^2 + 0.01)) of the last frame against
mis at 1024 spp from the last camera, and the share of the frame's pixels that were sampled - on the first frame, and the
mean over the eight moved ones - beside the full temporal preview (every pixel sampled every frame).  Also
e over the last frame's live pixels alone (first-hit depth > 0) and over the others (misses, which no history covers and
the fill alone colours): demand samples live pixels only.  The default min_history is moved only for a
value with a lower geometric-mean e at no larger a sampled share.  Prints tables to stderr and one JSON line.

  tools/demand_sweep.py"""
import json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch
import scenes
from vimg_amd import demand, hip

ORBIT_STEPS, DEGREES = 8, 1.5
MIN_HISTORIES = (0.0, 0.5, 1.0, 2.0, 4.0)
STRIDES = (2, 3, 4)
VIEWS = {"cornell_box_spheres.json": ((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0),
         "disney_spheres.json": ((0.0, 20.0, 1600.0), (0.0, -4.0, 0.0), 25.0)}


def orbit_camera(name, i):
    """Step i of tools/temporal_cost.py's orbit."""
    eye0, at0, vfov = (np.array(v) if k < 2 else v for k, v in enumerate(VIEWS[name]))
    pivot = eye0 + 1.7 * (at0 - eye0)
    a, r = math.radians(DEGREES * i), eye0 - pivot
    eye = pivot + np.array([r[0] * math.cos(a) + r[2] * math.sin(a), r[1], -r[0] * math.sin(a) + r[2] * math.cos(a)])
    return eye, eye + (at0 - eye0), (0.0, 1.0, 0.0), vfov


def rse(x, ref, where=None):
    err = ((x - ref) ** 2) / (ref ** 2 + 0.01)
    return float((err if where is None else err[where]).mean())


def walk(dev, name, preview, pixels):
    """The last frame of the orbit, its live pixels, and the share of pixels sampled on each frame (none without demand)."""
    shares = []
    for i in range(ORBIT_STEPS + 1):
        dev.set_camera(*orbit_camera(name, i))
        frame = preview.frame()
        if preview.last_demand is not None:
            shares.append(demand.read(preview.last_demand[2])["masked"] / pixels)
    return frame.cpu().numpy().astype(np.float64), (preview.history.tensor[1, ..., 3] > 0).cpu().numpy(), shares


hip.init(0)
out = {"min_histories": MIN_HISTORIES, "strides": STRIDES, "pictures": {}}
for name, res in (("cornell_box_spheres.json", (64, 64)), ("cornell_box_spheres.json", (256, 256)), ("disney_spheres.json", (450, 200))):
    w, h = res
    s = scenes.json_scene(name, res=res)
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    full = dev.temporal_preview(p, samples=4, denoise=False)
    last_full, live, _ = walk(dev, name, full, w * h)
    full.close()
    ref = dev.render(s.default_params(integrator="mis", samples=1024), stats=False).cpu().numpy().astype(np.float64)
    row = {"e_temporal_full": rse(last_full, ref), "e_temporal_full_live": rse(last_full, ref, live), "live": float(live.mean()), "strides": {}}
    for stride in STRIDES:
        cell = {"e": {}, "e_live": {}, "e_not_live": {}, "share_first": {}, "share_moved": {}}
        for m in MIN_HISTORIES:
            pv = dev.temporal_preview(p, samples=4, sparse=stride, denoise=False, demand=dict(min_history=m))
            last, live, shares = walk(dev, name, pv, w * h)
            pv.close()
            cell["e"][str(m)] = rse(last, ref)
            cell["e_live"][str(m)] = rse(last, ref, live)
            cell["e_not_live"][str(m)] = rse(last, ref, ~live) if not live.all() else 0.0
            cell["share_first"][str(m)] = shares[0]
            cell["share_moved"][str(m)] = float(np.mean(shares[1:]))
        row["strides"][str(stride)] = cell
    dev.close()
    key = f"{name.split('.')[0]} {w}x{h}"
    out["pictures"][key] = row
    print(f"{key}: e full temporal {row['e_temporal_full']:.5f}   over its live pixels ({100 * row['live']:.1f} % of the frame) "
          f"{row['e_temporal_full_live']:.5f}", file=sys.stderr)
    for stride in STRIDES:
        cell = row["strides"][str(stride)]
        print(f"  stride {stride}, by min_history:   e " + "  ".join(f"{m:g}: {cell['e'][str(m)]:.5f}" for m in MIN_HISTORIES), file=sys.stderr)
        print("       e over the live pixels    " + "  ".join(f"{m:g}: {cell['e_live'][str(m)]:.5f}" for m in MIN_HISTORIES)
              + "     over the others " + "  ".join(f"{m:g}: {cell['e_not_live'][str(m)]:.5f}" for m in MIN_HISTORIES), file=sys.stderr)
        print("       share sampled, moved frames " + "  ".join(f"{m:g}: {cell['share_moved'][str(m)]:.4f}" for m in MIN_HISTORIES)
              + "     first frame " + "  ".join(f"{m:g}: {cell['share_first'][str(m)]:.4f}" for m in MIN_HISTORIES), file=sys.stderr)


def geo(values):
    return float(np.exp(np.mean(np.log(values))))


out["geometric_mean_e"] = {str(m): geo([row["strides"][str(st)]["e"][str(m)] for row in out["pictures"].values() for st in STRIDES])
                           for m in MIN_HISTORIES}
out["mean_share_moved"] = {str(m): float(np.mean([row["strides"][str(st)]["share_moved"][str(m)] for row in out["pictures"].values()
                                                  for st in STRIDES])) for m in MIN_HISTORIES}
for st in STRIDES:
    out[f"geometric_mean_e_stride{st}"] = {str(m): geo([row["strides"][str(st)]["e"][str(m)] for row in out["pictures"].values()])
                                           for m in MIN_HISTORIES}
    out[f"mean_share_moved_stride{st}"] = {str(m): float(np.mean([row["strides"][str(st)]["share_moved"][str(m)]
                                                                  for row in out["pictures"].values()])) for m in MIN_HISTORIES}
out["geometric_mean_e_live"] = {str(m): geo([row["strides"][str(st)]["e_live"][str(m)] for row in out["pictures"].values() for st in STRIDES])
                                for m in MIN_HISTORIES}
out["geometric_mean_e_temporal_full"] = geo([row["e_temporal_full"] for row in out["pictures"].values()])
out["library_default"] = float(demand.params().min_history)
print("geometric mean of e over the pictures and strides, by min_history: "
      + "  ".join(f"{float(k):g}: {v:.5f}" for k, v in out["geometric_mean_e"].items())
      + f"     full temporal {out['geometric_mean_e_temporal_full']:.5f}", file=sys.stderr)
print("the same over the live pixels alone:                               "
      + "  ".join(f"{float(k):g}: {v:.5f}" for k, v in out["geometric_mean_e_live"].items()), file=sys.stderr)
print("mean share sampled on the moved frames:                           "
      + "  ".join(f"{float(k):g}: {v:.4f}" for k, v in out["mean_share_moved"].items()), file=sys.stderr)
for st in STRIDES:
    print(f"  stride {st} alone: e " + "  ".join(f"{float(k):g}: {v:.5f}" for k, v in out[f"geometric_mean_e_stride{st}"].items())
          + "   share " + "  ".join(f"{float(k):g}: {v:.4f}" for k, v in out[f"mean_share_moved_stride{st}"].items()), file=sys.stderr)
print(f"vimg_demand_defaults' min_history is {out['library_default']:g}", file=sys.stderr)
print(json.dumps(out))
