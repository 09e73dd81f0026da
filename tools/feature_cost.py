#!/usr/bin/env python3
"""Cost of the first-hit feature integrators: the time of one launch of each of albedo, normal,
depth, position, uv and coverage, beside an s_normal launch of the same frame - the same camera rays through
the product's scheduler - on
  config2    disney_spheres at 1800 x 800, 16 spp
  config5    the config 5 stand-in (519 200 triangles, mip-mapped image textures, normal maps), 1366 x 768, 16 spp
Times are device events right around the kernel (vimg_hip_time_renders), median and best of `steps` launches after
two warm-up launches.  With --parent-lib PATH (a libvimg_hip.so built from the parent commit) a child process
first times s_normal on that library (VIMG_HIP_LIB), so the row the features are compared with is the parent's.
Prints a table to stderr and one JSON line.

  tools/feature_cost.py [--steps N] [--spp N] [--parent-lib PATH] [--only s_normal]"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7)
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--parent-lib")
ap.add_argument("--only")
args = ap.parse_args()

parent = None
if args.parent_lib:     # before this process opens the GPU
    env = dict(os.environ, VIMG_HIP_LIB=os.path.abspath(args.parent_lib))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--spp", str(args.spp),
                        "--only", "s_normal"], env=env, capture_output=True, text=True, check=True)
    parent = json.loads(r.stdout.strip().splitlines()[-1])

import numpy as np
import torch
import scenes
from vimg_amd import abi, hip

hip.init(0)
names = [args.only] if args.only else ["s_normal"] + [n for n in ("albedo", "normal", "depth", "position", "uv", "coverage")
                                                     if n in abi.INTEGRATORS]
out = {"spp": args.spp, "steps": args.steps, "lib": os.environ.get("VIMG_HIP_LIB", "this tree"), "scenes": {}}
for label, make in (("config2", lambda: scenes.json_scene("disney_spheres.json", res=(1800, 800))),
                    ("config5", lambda: scenes.config5_scene())):
    s = make()
    dev = hip.DeviceScene(s)
    w, h = s.resolution
    frame = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    rows = {}
    for name in names:
        p = s.default_params(integrator=name, samples=args.spp)
        dev.time_renders(p, frame, 2)
        ms = np.sort(dev.time_renders(p, frame, args.steps))
        rows[name] = {"kernel": dev.kernel_for(p), "median_ms": float(np.median(ms)), "best_ms": float(ms[0])}
    out["scenes"][label] = rows
    dev.close()
if parent:
    out["parent"] = parent
print(f"{'scene':8} {'integrator':10} {'kernel':32} {'median ms':>10} {'best ms':>10}", file=sys.stderr)
for src, tag in ((parent, " (parent)"), (out, "")):
    for label, rows in (src["scenes"].items() if src else ()):
        for name, r in rows.items():
            print(f"{label:8} {name:10} {r['kernel'] + tag:32} {r['median_ms']:10.3f} {r['best_ms']:10.3f}", file=sys.stderr)
print(json.dumps(out))
