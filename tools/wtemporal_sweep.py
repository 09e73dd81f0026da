#!/usr/bin/env python3
"""The weight of a filled pixel: the orbit of 4.19 (tools/temporal_cost.py's: the eye on a circle, 1.5
degrees per step, viewing direction kept; 8 steps, mis at 4 spp) on cornell_box_spheres (64 x 64 and 256 x 256) and
disney_spheres (450 x 200), every frame sampled on one lattice of stride 2 or 3 - the phase cycling as
TemporalPreview(sparse=stride) cycles it - filled by infill.reconstruct at radius = stride and accumulated by
wtemporal.accumulate with sparse_weights at fill_weight 0, 1/16, 1/8, 1/4, 1/2, 1.  The sparse frames are rendered once
per stride and accumulated again under every fill_weight (the pieces TemporalPreview.frame() is made of, bit for bit:
tests/test_wtemporal.py).  e = mean((x - ref)^2 / (ref^2 + 0.01)) of the last frame against mis at 1024 spp from the
last camera; beside it the last sparse frame alone (what DeviceScene.render_sparse gives), the noisy full frame and the
full temporal accumulation (every pixel sampled, temporal.accumulate).  The default is the fill_weight with the lowest
geometric mean of e over the three pictures and both strides.  Prints tables to stderr and one JSON line.

  tools/wtemporal_sweep.py"""
import json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch
import scenes
from vimg_amd import hip, infill, temporal, wtemporal

ORBIT_STEPS, DEGREES = 8, 1.5
FILL_WEIGHTS = (0.0, 1 / 16, 1 / 8, 1 / 4, 1 / 2, 1.0)
STRIDES = (2, 3)
VIEWS = {"cornell_box_spheres.json": ((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0),
         "disney_spheres.json": ((0.0, 20.0, 1600.0), (0.0, -4.0, 0.0), 25.0)}


def orbit_camera(name, i):
    """Step i of tools/temporal_cost.py's orbit."""
    eye0, at0, vfov = (np.array(v) if k < 2 else v for k, v in enumerate(VIEWS[name]))
    pivot = eye0 + 1.7 * (at0 - eye0)
    a, r = math.radians(DEGREES * i), eye0 - pivot
    eye = pivot + np.array([r[0] * math.cos(a) + r[2] * math.sin(a), r[1], -r[0] * math.sin(a) + r[2] * math.cos(a)])
    return eye, eye + (at0 - eye0), (0.0, 1.0, 0.0), vfov


def rse(x, ref):
    return float((((x - ref) ** 2) / (ref ** 2 + 0.01)).mean())


hip.init(0)
out = {"fill_weights": FILL_WEIGHTS, "strides": STRIDES, "pictures": {}}
for name, res in (("cornell_box_spheres.json", (64, 64)), ("cornell_box_spheres.json", (256, 256)), ("disney_spheres.json", (450, 200))):
    w, h = res
    s = scenes.json_scene(name, res=res)
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    acc = dev.progressive(p)
    full, sparse = [], {stride: [] for stride in STRIDES}
    for i in range(ORBIT_STEPS + 1):
        dev.set_camera(*orbit_camera(name, i))
        g = dev.render_features(p, infill.GUIDES)
        m = temporal.world_to_pixel(dev.camera)
        full.append((dev.render(p, stats=False), g, m))
        for stride in STRIDES:
            acc.reset()
            noisy = acc.render(4, mask=infill.lattice_mask(h, w, stride, i % (stride * stride)))
            count = acc.counts()
            filled, code = infill.reconstruct(noisy, g["normal"], g["position"], g["depth"], count, albedo=g["albedo"], radius=stride)
            sparse[stride].append((filled, code, count, g, m))
    ref = dev.render(s.default_params(integrator="mis", samples=1024), stats=False).cpu().numpy().astype(np.float64)
    hist = None
    for c, g, m in full:
        hist = temporal.accumulate(c, g["normal"], g["position"], g["depth"], history=hist, world_to_pixel=m)
    row = {"e_noisy": rse(full[-1][0].cpu().numpy(), ref), "e_temporal_full": rse(hist.color.cpu().numpy(), ref), "strides": {}}
    for stride in STRIDES:
        cell = {"e_sparse_alone": rse(sparse[stride][-1][0].cpu().numpy(), ref), "e": {}, "codes_last": {}}
        for fw in FILL_WEIGHTS:
            hist = None
            for filled, code, count, g, m in sparse[stride]:
                wgt = wtemporal.sparse_weights(count, code, fill_weight=fw)
                hist, what = wtemporal.accumulate(filled, g["normal"], g["position"], g["depth"], wgt, history=hist, world_to_pixel=m)
            cell["e"][str(fw)] = rse(hist.color.cpu().numpy(), ref)
            cell["codes_last"][str(fw)] = [float((what == k).float().mean()) for k in range(5)]
        row["strides"][str(stride)] = cell
    key = f"{name.split('.')[0]} {w}x{h}"
    out["pictures"][key] = row
    print(f"{key}: e noisy 4 spp {row['e_noisy']:.5f}   full temporal {row['e_temporal_full']:.5f}", file=sys.stderr)
    for stride in STRIDES:
        cell = row["strides"][str(stride)]
        print(f"  stride {stride}: sparse frame alone {cell['e_sparse_alone']:.5f}   sparse + history, by fill_weight: "
              + "  ".join(f"{fw:g}: {cell['e'][str(fw)]:.5f}" for fw in FILL_WEIGHTS), file=sys.stderr)
        print(f"            codes 0..4 of the last frame at fill_weight {wtemporal.FILL_WEIGHT:g}: "
              + " ".join(f"{100 * x:.1f} %" for x in cell["codes_last"][str(float(wtemporal.FILL_WEIGHT))]), file=sys.stderr)
    acc.close()
    dev.close()

geo = {}
for fw in FILL_WEIGHTS:
    es = [row["strides"][str(stride)]["e"][str(fw)] for row in out["pictures"].values() for stride in STRIDES]
    geo[str(fw)] = float(np.exp(np.mean(np.log(es))))
out["geometric_mean_e"] = geo
for stride in STRIDES:
    out[f"geometric_mean_e_stride{stride}"] = {
        str(fw): float(np.exp(np.mean(np.log([row["strides"][str(stride)]["e"][str(fw)] for row in out["pictures"].values()]))))
        for fw in FILL_WEIGHTS}
out["best_fill_weight"] = float(min(geo, key=geo.get))
out["library_default"] = wtemporal.FILL_WEIGHT
print("geometric mean of e over the pictures and strides, by fill_weight: " + "  ".join(f"{float(k):g}: {v:.5f}" for k, v in geo.items()),
      file=sys.stderr)
for stride in STRIDES:
    print(f"  stride {stride} alone: " + "  ".join(f"{float(k):g}: {v:.5f}" for k, v in out[f'geometric_mean_e_stride{stride}'].items()),
          file=sys.stderr)
print(f"lowest at fill_weight {out['best_fill_weight']:g}; vimg_amd.wtemporal.FILL_WEIGHT is {wtemporal.FILL_WEIGHT:g}", file=sys.stderr)
print(json.dumps(out))
