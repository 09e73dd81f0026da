#!/usr/bin/env python3
"""The sweep behind the defaults of the variance-guided filter, by 4.18's procedure and metric:
cornell_box_spheres 512 x 512, disney_spheres 900 x 400 and cornell_box_spheres 64 x 64, mis, against mis at 1024 spp,
e = mean((x - ref)^2 / (ref^2 + 0.01)).  Three frames per scene from one accumulator each:
  4 spp       one increment: K = 1, no variance, every pixel's is estimated
  16 spp      four increments of 4: K = 4, the accumulator's variance
  adaptive    render_adaptive(target=0.05, step=4, max_samples=64): pixels at different counts, the accumulator's variance
Each is filtered by filter.atrous at its defaults (the yardstick) and by varfilter.atrous over the grid
iterations x sigma_luminance x variance_floor; the score of a setting is the geometric mean of e_filtered / e_noisy over
the six frames of the two large scenes (the 64 x 64 picture is reported beside it, as in 4.18).  Prints a table to
stderr and one JSON line.

  tools/varfilter_sweep.py [--top N]"""
import argparse, itertools, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--top", type=int, default=12)
args = ap.parse_args()

import numpy as np
import torch
import scenes
from vimg_amd import filter as flt, hip, varfilter

SCENES = (("cornell", "cornell_box_spheres.json", (512, 512)), ("disney", "disney_spheres.json", (900, 400)),
          ("cornell64", "cornell_box_spheres.json", (64, 64)))
SCORED = ("cornell", "disney")
ITERATIONS = (2, 3, 4, 5, 6)
SIGMA_LUMINANCE = (1.0, 2.0, 4.0, 8.0, 16.0)
VARIANCE_FLOOR = (1e-10, 1e-8, 1e-6, 1e-4)

hip.init(0)
frames = {}      # "scene frame" -> (noisy, variance or None, guides, reference)
for tag, name, res in SCENES:
    s = scenes.json_scene(name, res=res)
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    ref = dev.render(s.default_params(integrator="mis", samples=1024), stats=False).double()
    g = dev.render_features(p, flt.GUIDES)
    acc = dev.progressive(p)
    frames[f"{tag} 4spp"] = (acc.render(4).clone(), None, g, ref)
    for _ in range(3):
        img = acc.render(4)
    frames[f"{tag} 16spp"] = (img.clone(), acc.variance(), g, ref)
    acc.reset()
    img = acc.render_adaptive(target=0.05, step=4, max_samples=64)
    counts = acc.counts().double()
    frames[f"{tag} adaptive"] = (img.clone(), acc.variance(), g, ref)
    print(f"{tag}: adaptive frame at {counts.mean():.1f} spp on average, {float((counts >= 64).double().mean()) * 100:.1f} % of the pixels at 64",
          file=sys.stderr)
    acc.close()


def rse(x, ref):
    return float((((x.double() - ref) ** 2) / (ref ** 2 + 0.01)).mean())


out = {"frames": {}, "grid": []}
for key, (noisy, var, g, ref) in frames.items():
    fixed = flt.atrous(noisy, g["normal"], g["position"], g["depth"], albedo=g["albedo"])
    out["frames"][key] = {"noisy": rse(noisy, ref), "fixed": rse(fixed, ref)}
for it, sl, vf in itertools.product(ITERATIONS, SIGMA_LUMINANCE, VARIANCE_FLOOR):
    row = {"iterations": it, "sigma_luminance": sl, "variance_floor": vf, "ratio": {}}
    for key, (noisy, var, g, ref) in frames.items():
        got, _ = varfilter.atrous(noisy, g["normal"], g["position"], g["depth"], albedo=g["albedo"], variance=var, iterations=it,
                                  sigma_luminance=sl, variance_floor=vf)
        row["ratio"][key] = rse(got, ref) / out["frames"][key]["noisy"]
    scored = [v for k, v in row["ratio"].items() if k.split()[0] in SCORED]
    row["score"] = float(np.exp(np.mean(np.log(scored))))
    out["grid"].append(row)

keys = list(frames)
print("frame: e noisy, fixed filter's ratio", file=sys.stderr)
for k in keys:
    f = out["frames"][k]
    print(f"  {k:20} {f['noisy']:.5f}  {f['fixed'] / f['noisy']:.3f}", file=sys.stderr)
fixed_score = float(np.exp(np.mean([np.log(out["frames"][k]["fixed"] / out["frames"][k]["noisy"]) for k in keys if k.split()[0] in SCORED])))
out["fixed_score"] = fixed_score
print(f"fixed filter's score {fixed_score:.4f}", file=sys.stderr)
print("it  s_lum  v_floor   score   " + "  ".join(f"{k:>16}" for k in keys), file=sys.stderr)
for row in sorted(out["grid"], key=lambda r: r["score"])[:args.top]:
    print(f"{row['iterations']:2d} {row['sigma_luminance']:6.1f} {row['variance_floor']:8.0e}  {row['score']:.4f}   "
          + "  ".join(f"{row['ratio'][k]:16.3f}" for k in keys), file=sys.stderr)
print(json.dumps(out))
