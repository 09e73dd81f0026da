#!/usr/bin/env python3
"""Cost of the firefly clamp on disney_spheres at 450 x 200 and 1800 x 800, mis at 4 spp:
  clamp       despeckle.clamp in place with a caller's workspace and no codes (pack + clamp), radius 1, 2, 3, rank 1 and 4
  beside it   infill.reconstruct at radius 2 on the stride-2 lattice, and one iteration of filter.atrous, in the same run
  frame       a whole temporal_preview.frame() of a standing camera with and without ``despeckle=True``, the two
              alternating
Device events around each call for the library calls, the host clock around synchronised calls for frame() (a render
call waits for its launch); medians of `steps` calls after two warm-up calls, `rounds` rounds alternating the forms.
Prints tables to stderr and one JSON line.

  tools/despeckle_cost.py [--steps N] [--rounds N]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=15)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()

import numpy as np
import torch
import scenes
from vimg_amd import despeckle, filter as flt, hip, infill
from _timing import timed, wall

hip.init(0)
res_out = {"steps": args.steps, "rounds": args.rounds, "frames": {}}
for res in ((450, 200), (1800, 800)):
    w, h = res
    s = scenes.json_scene("disney_spheres.json", res=res)
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    g = dev.render_features(p, despeckle.GUIDES)
    guides = (g["normal"], g["position"], g["depth"])
    noisy = dev.render(p, stats=False)
    acc = dev.progressive(p)
    sparse = acc.render(4, mask=infill.lattice_mask(h, w, 2, 0))
    count = acc.counts().to(torch.int32)
    acc.close()
    buf, out = noisy.clone(), torch.empty_like(noisy)
    work = torch.empty(max(despeckle.workspace_bytes(w, h), infill.workspace_bytes(w, h), flt.atrous_workspace_bytes(w, h)),
                       dtype=torch.uint8, device="cuda")
    forms = {f"clamp radius {r} rank {k}": (lambda r=r, k=k: despeckle.clamp(buf, *guides, albedo=g["albedo"], out=buf, out_code=False,
                                                                             workspace=work, radius=r, rank=k))
             for r in (1, 2, 3) for k in (1, 4)}
    forms["clamp at the defaults, out of place, with codes"] = lambda: despeckle.clamp(noisy, *guides, albedo=g["albedo"], out=out, workspace=work)
    forms["infill.reconstruct radius 2"] = lambda: infill.reconstruct(sparse, *guides, count, albedo=g["albedo"], radius=2, out=out,
                                                                      workspace=work)
    forms["filter.atrous, 1 iteration"] = lambda: flt.atrous(noisy, *guides, albedo=g["albedo"], iterations=1, out=out, workspace=work)
    forms["filter.atrous, 3 iterations"] = lambda: flt.atrous(noisy, *guides, albedo=g["albedo"], iterations=3, out=out, workspace=work)
    ms = {k: [] for k in forms}
    for _ in range(args.rounds):               # alternating: other people's work shares the machine
        for k, fn in forms.items():
            ms[k].append(timed(fn, args.steps))
    torch.cuda.synchronize()
    row = {"calls_ms": {k: {"median_ms": float(np.median([m[0] for m in v])), "best_ms": float(min(m[1] for m in v))} for k, v in ms.items()}}
    code = despeckle.clamp(noisy, *guides, albedo=g["albedo"])[1]
    row["codes"] = [float((code == k).float().mean()) for k in range(4)]
    previews = {"frame() plain": dev.temporal_preview(p, samples=4), "frame() with despeckle": dev.temporal_preview(p, samples=4, despeckle=True)}
    rounds = [{k: wall(lambda i, v=v: v.frame(), args.steps) for k, v in previews.items()} for _ in range(args.rounds)]
    row["frame_ms_median_of_rounds"] = {k: float(np.median([r[k] for r in rounds])) for k in previews}
    row["frame_ms_rounds"] = rounds
    for v in previews.values():
        v.close()
    dev.close()
    res_out["frames"][f"{w}x{h}"] = row
    print(f"{w} x {h}: codes 0..3 at the defaults: " + " ".join(f"{100 * x:.2f} %" for x in row["codes"]), file=sys.stderr)
    for k, cell in row["calls_ms"].items():
        print(f"  {k:52} median {cell['median_ms']:.4f}  best {cell['best_ms']:.4f} ms", file=sys.stderr)
    for k, v in row["frame_ms_median_of_rounds"].items():
        print(f"  {k:52} {v:8.3f} ms", file=sys.stderr)
print(json.dumps(res_out))
