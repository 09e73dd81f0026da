#!/usr/bin/env python3
"""The flicker the auto-exposure exists to remove: on a standing camera, cornell_box_spheres 64 x 64 (as
it is, and looking down into the box with the ceiling light out of view) and disney_spheres 450 x 200, mis, 16 frames of
4 spp each, the frame-to-frame relative change |x_k / x_(k-1) - 1| of
  E*               the exposure a frame is metered to on its own (exposure.adapt on a fresh state) at the library's defaults
  1 / max L        the scale vimg_hip_post_rgb8's Reinhard operator takes from the frame's largest luminance
for two kinds of sequence, each with and without ``despeckle``:
  increments       the 16 independent 4-spp frames themselves (k mean_k - (k - 1) mean_(k-1) of a Progressive), unfiltered:
                   the noisiest thing a viewer could be shown
  preview          what DeviceScene.temporal_preview(...).frame() returns: accumulated and filtered
With --permilles it also reports E*'s flicker on the increments for other windows, the evidence for or against the defaults.
Prints tables to stderr and one JSON line.

  tools/exposure_sweep.py [--frames N] [--permilles]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--permilles", action="store_true")
args = ap.parse_args()

import numpy as np
import torch
import scenes
from vimg_amd import despeckle, exposure, hip

# (tag, scene, resolution, camera or None: the scene's own).  Both scenes' own cameras SEE a light source, whose radiance is
# then the frame's largest luminance on every frame; the third sequence looks down into the box, the ceiling light out of view
SCENES = (("cornell", "cornell_box_spheres.json", (64, 64), None), ("disney", "disney_spheres.json", (450, 200), None),
          ("cornell, light out of view", "cornell_box_spheres.json", (64, 64), ((278.0, 278.0, -800.0), (278.0, 0.0, 279.0), (0.0, 1.0, 0.0), 40.0)))
WINDOWS = ((0, 1000), (100, 900), (250, 750), (500, 950), (500, 990), (500, 1000), (800, 990))
LUM = torch.tensor([0.212671, 0.715160, 0.072169], dtype=torch.float32, device="cuda")


def target(frame, **kw):
    """E* of the frame on its own: a fresh state's first exposure."""
    return exposure.read(exposure.adapt(frame, **kw)[1])["exposure"]


def inverse_max(frame):
    L = (frame * LUM).sum(-1)
    return 1.0 / float(L[torch.isfinite(L)].max())


def flicker(xs):
    r = np.abs(np.array(xs[1:]) / np.array(xs[:-1]) - 1)
    return {"max": float(r.max()), "mean": float(r.mean()), "spread": float(max(xs) / min(xs))}


hip.init(0)
out = {"frames": args.frames, "sequences": {}}
for tag, name, res, camera in SCENES:
    s = scenes.json_scene(name, res=res)
    dev = hip.DeviceScene(s)
    if camera is not None:
        dev.set_camera(*camera)
    p = s.default_params(integrator="mis", samples=4)
    g = dev.render_features(p, despeckle.GUIDES)
    acc, last, increments = dev.progressive(p), None, []
    for k in range(1, args.frames + 1):
        mean = acc.render(4).double()
        increments.append((mean if last is None else k * mean - (k - 1) * last).float().contiguous())
        last = mean
    acc.close()
    sequences = {"increments": increments,
                 "increments, despeckle": [despeckle.clamp(c, g["normal"], g["position"], g["depth"], albedo=g["albedo"], out_code=False)[0]
                                           for c in increments]}
    for label, kw in (("preview", {}), ("preview, despeckle", dict(despeckle=True))):
        pv = dev.temporal_preview(p, samples=4, **kw)
        sequences[label] = [pv.frame().clone() for _ in range(args.frames)]
        pv.close()
    for label, frames in sequences.items():
        row = {"E*": flicker([target(f) for f in frames]), "1/max": flicker([inverse_max(f) for f in frames])}
        if args.permilles and label.startswith("increments"):
            row["windows"] = {f"{lo}-{hi}": flicker([target(f, low_permille=lo, high_permille=hi) for f in frames]) for lo, hi in WINDOWS}
        out["sequences"][f"{tag} {label}"] = row
        print(f"{tag:26} {label:22} E*: max {100 * row['E*']['max']:7.3f} %  mean {100 * row['E*']['mean']:7.3f} %   "
              f"1 / max L: max {100 * row['1/max']['max']:8.2f} %  mean {100 * row['1/max']['mean']:8.2f} %  (largest / smallest "
              f"{row['1/max']['spread']:.2f})", file=sys.stderr)
        for win, f in row.get("windows", {}).items():
            print(f"{'':12} E* over the permilles {win:9} max {100 * f['max']:7.3f} %  mean {100 * f['mean']:7.3f} %", file=sys.stderr)
    dev.close()
print(json.dumps(out))
