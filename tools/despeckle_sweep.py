#!/usr/bin/env python3
"""The sweep behind the defaults of the firefly clamp, on the frames and by the metric of 4.18:
cornell_box_spheres 512 x 512 and disney_spheres 900 x 400, mis at 4 and 16 spp (two increments of half the count, so
the accumulator knows a variance), guides at 4 samples, against mis at 1024 spp, e = mean((x - ref)^2 / (ref^2 + 0.01))
over the whole frame.  Each frame is clamped by despeckle.clamp over the grid radius x rank x gain (min_taps 4, or the
rank where that is larger; the sigmas and the floor at the library's defaults) and then filtered by filter.atrous and by
varfilter.atrous at their defaults.  For each setting: e of the clamped frame, e of the clamped-then-filtered frame
under both filters, the share of the live pixels clamped on the noisy frame and on the 1024-spp frame, and the mean
luminance kept.  The score of a setting is the geometric mean of its eight filtered e; a setting is ELIGIBLE when none of
the eight is above that of the same frame filtered without a clamp and it clamps at most 1 % of the live pixels of each
reference frame.  Prints tables to stderr and one JSON line.

  tools/despeckle_sweep.py [--top N]"""
import argparse, itertools, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--top", type=int, default=12)
args = ap.parse_args()

import numpy as np
import torch
import scenes
from vimg_amd import despeckle, filter as flt, hip, varfilter

SCENES = (("cornell", "cornell_box_spheres.json", (512, 512)), ("disney", "disney_spheres.json", (900, 400)))
SPPS = (4, 16)
RADIUS, RANK, GAIN = (1, 2, 3), (1, 2, 3, 4), (1.0, 1.5, 2.0, 3.0, 4.0)
LUM = torch.tensor([0.212671, 0.715160, 0.072169], dtype=torch.float64, device="cuda")


def rse(x, ref):
    return float((((x.double() - ref) ** 2) / (ref ** 2 + 0.01)).mean())


def filtered(color, g, variance):
    kw = dict(albedo=g["albedo"])
    return (flt.atrous(color, g["normal"], g["position"], g["depth"], **kw),
            varfilter.atrous(color, g["normal"], g["position"], g["depth"], variance=variance, **kw)[0])


def clamp(color, g, **kw):
    return despeckle.clamp(color, g["normal"], g["position"], g["depth"], albedo=g["albedo"], **kw)


hip.init(0)
frames, refs = {}, {}      # "scene spp" -> (noisy frame, variance, guides, reference); scene -> (reference, guides)
out = {"frames": {}, "grid": []}
for tag, name, res in SCENES:
    s = scenes.json_scene(name, res=res)
    dev = hip.DeviceScene(s)
    ref = dev.render(s.default_params(integrator="mis", samples=1024), stats=False)
    g = dev.render_features(s.default_params(integrator="mis", samples=4), despeckle.GUIDES)
    refs[tag] = (ref, g)
    for spp in SPPS:
        acc = dev.progressive(s.default_params(integrator="mis", samples=spp))
        acc.render(spp // 2, out=False)
        noisy = acc.render(spp // 2).clone()
        variance = acc.variance().clone()
        acc.close()
        key = f"{tag} {spp}spp"
        frames[key] = (noisy, variance, g, ref.double())
        fixed, guided = filtered(noisy, g, variance)
        out["frames"][key] = {"noisy": rse(noisy, ref.double()), "filtered": rse(fixed, ref.double()),
                              "variance_guided": rse(guided, ref.double())}
    dev.close()

keys = list(frames)
for r, k, gain in itertools.product(RADIUS, RANK, GAIN):
    p = dict(radius=r, rank=k, gain=gain, min_taps=max(4, k))
    row = dict(p, e_clamped={}, e_filtered={}, e_variance_guided={}, clamped_share={}, luminance_kept={}, reference_share={})
    for key, (noisy, variance, g, ref) in frames.items():
        c, code = clamp(noisy, g, **p)
        fixed, guided = filtered(c, g, variance)
        row["e_clamped"][key], row["e_filtered"][key], row["e_variance_guided"][key] = rse(c, ref), rse(fixed, ref), rse(guided, ref)
        row["clamped_share"][key] = float((code == 1).sum() / (code != 3).sum())
        row["luminance_kept"][key] = float((c.double() @ LUM).mean() / (noisy.double() @ LUM).mean())
    for tag, (ref, g) in refs.items():
        code = clamp(ref, g, **p)[1]
        row["reference_share"][tag] = float((code == 1).sum() / (code != 3).sum())
    eight = [row[f][key] for f in ("e_filtered", "e_variance_guided") for key in keys]
    row["score"] = float(np.exp(np.mean(np.log(eight))))
    row["not_worse"] = all(row["e_filtered"][key] <= out["frames"][key]["filtered"] and
                           row["e_variance_guided"][key] <= out["frames"][key]["variance_guided"] for key in keys)
    row["eligible"] = bool(row["not_worse"] and max(row["reference_share"].values()) <= 0.01)
    out["grid"].append(row)

none = [out["frames"][key][f] for f in ("filtered", "variance_guided") for key in keys]
out["score_without_clamp"] = float(np.exp(np.mean(np.log(none))))
d = despeckle.params()
out["defaults"] = {"radius": d.radius, "rank": d.rank, "gain": d.gain, "min_taps": d.min_taps}
shipped = next(row for row in out["grid"] if (row["radius"], row["rank"], row["gain"]) == (d.radius, d.rank, d.gain))
eligible = sorted((row for row in out["grid"] if row["eligible"]), key=lambda row: row["score"])
out["best_eligible"] = {k: eligible[0][k] for k in ("radius", "rank", "gain", "score")} if eligible else None
out["shipped"] = {k: shipped[k] for k in ("score", "not_worse", "eligible")}


def line(row):
    return (f"{row['radius']:2d} {row['rank']:4d} {row['gain']:5.1f}  {row['score']:.5f}  {'yes' if row['eligible'] else ' no'}  "
            + "  ".join(f"{row['e_clamped'][k]:.5f} {row['e_filtered'][k]:.5f} {row['e_variance_guided'][k]:.5f} "
                        f"{100 * row['clamped_share'][k]:5.2f}% {row['luminance_kept'][k]:.4f}" for k in keys)
            + "  | " + "  ".join(f"{100 * v:.3f}%" for v in row["reference_share"].values()))


print("frame: e noisy, e filtered, e variance-guided, without a clamp", file=sys.stderr)
for k, f in out["frames"].items():
    print(f"  {k:14} {f['noisy']:.5f}  {f['filtered']:.5f}  {f['variance_guided']:.5f}", file=sys.stderr)
print(f"score without a clamp: {out['score_without_clamp']:.5f}", file=sys.stderr)
print(" r rank  gain    score  elig  per frame (" + ", ".join(keys) + "): e clamped, e filtered, e variance-guided, share clamped, "
      "luminance kept  | share of the reference clamped (" + ", ".join(refs) + ")", file=sys.stderr)
for row in sorted(out["grid"], key=lambda row: row["score"])[:args.top]:
    print(line(row), file=sys.stderr)
print("the shipped defaults:", file=sys.stderr)
print(line(shipped), file=sys.stderr)
print("the best eligible setting:", file=sys.stderr)
print(line(eligible[0]) if eligible else "  none", file=sys.stderr)
for gain in GAIN:
    print(f"gain {gain}: score by radius (rows) x rank (columns); * = eligible", file=sys.stderr)
    for r in RADIUS:
        print("  " + "  ".join(f"{row['score']:.5f}{'*' if row['eligible'] else ' '}" for row in out["grid"]
                                if row["radius"] == r and row["gain"] == gain), file=sys.stderr)
print(json.dumps(out))
