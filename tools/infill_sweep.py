#!/usr/bin/env python3
"""The sweep behind the defaults of the reconstruction of sparsely sampled frames, on the frames and
by the metric of 4.18: cornell_box_spheres 512 x 512 and disney_spheres 900 x 400, mis at 4 and 16 spp on the stride-2
lattice of phase 0 (one pixel in four has the samples), against mis at 1024 spp, e = mean((x - ref)^2 / (ref^2 + 0.01))
over the whole frame.  Each frame is filled by infill.reconstruct over the grid radius x sigma_normal x sigma_plane; the
score of a setting is the geometric mean of e over the four frames.  Beside it: e of the tent-weighted mean without
guides (radius 2), e of the same samples on every pixel (the plain render at that count), and the shares of the codes.
Small pictures (cornell 64 x 64, disney 90 x 40, and the two of tests/test_infill.py, glass_in_box and
sphere_light_medium_mis at 64 x 64; 16 spp) are reported beside it, as in 4.18, and do not count in the score.
Prints tables to stderr and one JSON line.

  tools/infill_sweep.py [--top N]"""
import argparse, itertools, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--top", type=int, default=12)
args = ap.parse_args()

import numpy as np
import torch
import scenes
from vimg_amd import hip, infill

SCENES = (("cornell", "cornell_box_spheres.json", (512, 512), (4, 16)), ("disney", "disney_spheres.json", (900, 400), (4, 16)),
          ("cornell64", "cornell_box_spheres.json", (64, 64), (16,)), ("disney90", "disney_spheres.json", (90, 40), (16,)),
          ("glass64", "glass_in_box.json", (64, 64), (16,)), ("light64", "MIS_light_tests/sphere_light_medium_mis.json", (64, 64), (16,)))
SCORED = ("cornell", "disney")
RADIUS = (1, 2, 3, 4)
SIGMA_NORMAL = (0.25, 0.5, 1.0, 2.0, 4.0)
SIGMA_PLANE = (0.0002, 0.0005, 0.001, 0.002, 0.005, 0.02)


def rse(x, ref):
    return float((((x.double() - ref) ** 2) / (ref ** 2 + 0.01)).mean())


def tent_fill(color, sampled, radius):
    """The tent-weighted mean of the sampled pixels within `radius`, without guides (tests/infill_ref.py's tent_fill)."""
    h, w = sampled.shape
    pad = torch.nn.functional.pad
    c = pad((color.double() * sampled[..., None]).permute(2, 0, 1), (radius,) * 4)
    m = pad(sampled.double(), (radius,) * 4)
    sw, sc = torch.zeros_like(m[:h, :w]), torch.zeros_like(c[:, :h, :w])
    for dy, dx in itertools.product(range(2 * radius + 1), repeat=2):
        k = float((radius + 1 - abs(dx - radius)) * (radius + 1 - abs(dy - radius)))
        sw += k * m[dy:dy + h, dx:dx + w]
        sc += k * c[:, dy:dy + h, dx:dx + w]
    mean = (sc / torch.where(sw > 0, sw, torch.ones_like(sw))).permute(1, 2, 0)
    return torch.where(sampled[..., None], color.double(), mean)


hip.init(0)
frames = {}      # "scene spp" -> (sparse frame, counts, guides, reference)
out = {"frames": {}, "grid": []}
for tag, name, res, spps in SCENES:
    s = scenes.json_scene(name, res=res)
    dev = hip.DeviceScene(s)
    w, h = res
    ref = dev.render(s.default_params(integrator="mis", samples=1024), stats=False).double()
    g = dev.render_features(s.default_params(integrator="mis", samples=4), infill.GUIDES)
    mask = infill.lattice_mask(h, w, 2, 0)
    for spp in spps:
        p = s.default_params(integrator="mis", samples=spp)
        acc = dev.progressive(p)
        noisy = acc.render(spp, mask=mask).clone()
        count = acc.counts().to(torch.int32)
        acc.close()
        key = f"{tag} {spp}spp"
        frames[key] = (noisy, count, g, ref)
        got, code = infill.reconstruct(noisy, g["normal"], g["position"], g["depth"], count, albedo=g["albedo"])
        unsampled = count == 0
        out["frames"][key] = {"tent_only_radius2": rse(tent_fill(noisy, count > 0, 2), ref), "defaults": rse(got, ref),
                              "every_pixel_sampled": rse(dev.render(p, stats=False), ref),
                              "code_share_of_unsampled": [float(((code == k) & unsampled).sum() / unsampled.sum()) for k in (1, 2, 3)]}
    dev.close()

scored = [k for k in frames if k.split()[0] in SCORED]
for r, sn, sp in itertools.product(RADIUS, SIGMA_NORMAL, SIGMA_PLANE):
    row = {"radius": r, "sigma_normal": sn, "sigma_plane": sp, "e": {}, "code2_share_of_unsampled": {}}
    for key, (noisy, count, g, ref) in frames.items():
        got, code = infill.reconstruct(noisy, g["normal"], g["position"], g["depth"], count, albedo=g["albedo"], radius=r, sigma_normal=sn,
                                       sigma_plane=sp)
        row["e"][key] = rse(got, ref)
        row["code2_share_of_unsampled"][key] = float((code == 2).sum() / (count == 0).sum())
    row["score"] = float(np.exp(np.mean(np.log([row["e"][k] for k in scored]))))
    out["grid"].append(row)

d = infill.params()
out["defaults"] = {"radius": d.radius, "sigma_normal": d.sigma_normal, "sigma_plane": d.sigma_plane}
print("frame: e tent only (radius 2), e at the defaults, e with every pixel sampled; codes 1 / 2 / 3 as shares of the unsampled pixels", file=sys.stderr)
for k, f in out["frames"].items():
    print(f"  {k:18} {f['tent_only_radius2']:.5f}  {f['defaults']:.5f}  {f['every_pixel_sampled']:.5f}   "
          + " / ".join(f"{100 * x:.2f} %" for x in f["code_share_of_unsampled"]), file=sys.stderr)
for name, pick in (("tent only", "tent_only_radius2"), ("defaults", "defaults")):
    out[f"score {name}"] = float(np.exp(np.mean([np.log(out["frames"][k][pick]) for k in scored])))
    print(f"score of {name}: {out[f'score {name}']:.5f}", file=sys.stderr)
others = [k for k in frames if k not in scored]
print(" r  s_normal  s_plane    score   " + "  ".join(f"{k:>14}" for k in scored) + "   | e and code 2 share: " + "  ".join(others), file=sys.stderr)
for row in sorted(out["grid"], key=lambda r: r["score"])[:args.top]:
    print(f"{row['radius']:2d} {row['sigma_normal']:9.3f} {row['sigma_plane']:8.4f}  {row['score']:.5f}   "
          + "  ".join(f"{row['e'][k]:14.5f}" for k in scored) + "   | "
          + "  ".join(f"{row['e'][k]:.5f} {100 * row['code2_share_of_unsampled'][k]:5.2f} %" for k in others), file=sys.stderr)
for r in RADIUS:
    print(f"radius {r}: score by sigma_normal (rows) x sigma_plane (columns)", file=sys.stderr)
    for sn in SIGMA_NORMAL:
        print(f"  {sn:5.2f}  " + "  ".join(f"{row['score']:.5f}" for row in out["grid"] if row["radius"] == r and row["sigma_normal"] == sn), file=sys.stderr)
print(json.dumps(out))
