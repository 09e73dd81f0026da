#!/usr/bin/env python3
"""Cost of reprojecting through displacement at 450 x 200 and 1800 x 800, on cornell_box_spheres and on
the config 5 stand-in (tests/scenes.py: about half a million triangles), mis at 4 spp, after an update_geometry that
moves every vertex and every sphere by (0.25, 0, -0.125) - so every hit pixel gathers and adds:
  parts       DeviceScene.camera_rays on motion.centre_samples, DeviceScene.trace_rays (hits only),
              motion.previous_position and the copy of the position frame into plane G1, device events around each call
  beside it   the same session's temporal.accumulate on the same frames
  frame       a whole TemporalPreview.frame() after update_geometry, with and without ``motion``, by the host clock
              around synchronised calls, the scene alternating between its two positions
All in one process, interleaved; median and best of `steps` calls after two warm-up calls.  Prints tables to stderr and
one JSON line.

  tools/motion_cost.py [--steps N] [--no-config5]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7)
ap.add_argument("--no-config5", action="store_true")
args = ap.parse_args()

import numpy as np
import torch
import scenes
from vimg_amd import hip, motion, temporal
from _timing import timed, wall

SHIFT = np.array([0.25, 0.0, -0.125], np.float32)
CAMERAS = {"cornell_box_spheres": ((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), (0, 1, 0), 40.0),
           "config5": ((0.0, 7.0, 13.0), (0.0, 0.5, 0.0), (0, 1, 0), 38.0)}

hip.init(0)
built = {"cornell_box_spheres": scenes.json_scene("cornell_box_spheres.json")}
if not args.no_config5:
    built["config5"] = scenes.config5_scene()
out = {"steps": args.steps, "scenes": {}}
for name, s in built.items():
    for res in ((450, 200), (1800, 800)):
        w, h = res
        s.set_camera(*CAMERAS[name], res)
        dev = hip.DeviceScene(s)
        p = s.default_params(integrator="mis", samples=4)
        verts, _, spheres = s.geometry()
        there = (verts + SHIFT, spheres + np.concatenate([SHIFT, [0]]).astype(np.float32))
        here = (verts, spheres)
        tables = motion.SceneTables.from_host(s)
        dev.update_geometry(vertices=there[0], spheres=there[1] if len(spheres) else None)
        now = motion.Positions(dev.vertices_given, dev.spheres_given if len(spheres) else None)
        old = motion.Positions(tables.positions.vertices, tables.positions.spheres if len(spheres) else None)
        color = dev.render(p, stats=False)
        g = dev.render_features(p, ("normal", "position", "depth"))
        m = temporal.world_to_pixel(dev.camera)
        first = temporal.accumulate(color, g["normal"], g["position"], g["depth"], world_to_pixel=m)
        nxt = torch.empty_like(first.tensor)
        samples = torch.from_numpy(motion.centre_samples(h, w)).cuda()
        rays = torch.empty((h * w, 8), dtype=torch.float32, device="cuda")
        hits = torch.empty((h * w, 4), dtype=torch.float32, device="cuda")
        q, code = torch.empty_like(color), torch.empty((h, w), dtype=torch.uint8, device="cuda")
        row = {}
        calls = {"camera_rays": lambda: dev.camera_rays(samples, out=rays),
                 "trace_rays (hits only)": lambda: dev.trace_rays(rays, out=hits),
                 "motion.previous_position": lambda: motion.previous_position(g["position"], hits, rays, tables, old, now, out=q, out_code=code),
                 "G1 copy": lambda: nxt[2, :, :, :3].copy_(g["position"]),
                 "temporal.accumulate": lambda: temporal.accumulate(color, g["normal"], q, g["depth"], history=first, world_to_pixel=m,
                                                                    next_history=nxt)}
        for _ in range(2):          # interleaved: every call in turn, twice over
            for k, fn in calls.items():
                med, best = timed(fn, args.steps)
                row[k] = (med, best) if k not in row else (min(med, row[k][0]), min(best, row[k][1]))
        moved = float((code != 0).float().mean())
        dev.update_geometry(vertices=here[0], spheres=here[1] if len(spheres) else None)       # the host scene's positions: what motion=s reads
        previews = {"frame() after update_geometry": dev.temporal_preview(p, samples=4),
                    "frame() after update_geometry, motion": dev.temporal_preview(p, samples=4, motion=s)}
        for pv in previews.values():
            pv.frame()

        def stepped(pv):
            def go(i):
                v, sp = there if i % 2 == 0 else here
                dev.update_geometry(vertices=v, spheres=sp if len(spheres) else None)
                pv.frame()
            return go

        def update_only(i):
            v, sp = there if i % 2 == 0 else here
            dev.update_geometry(vertices=v, spheres=sp if len(spheres) else None)

        frame_ms = {"update_geometry alone": wall(update_only, args.steps)}
        for _ in range(2):
            for k, pv in previews.items():
                ms = wall(stepped(pv), args.steps)
                frame_ms[k] = ms if k not in frame_ms else min(ms, frame_ms[k])
        for pv in previews.values():
            pv.close()
        dev.close()
        out["scenes"][f"{name} {w}x{h}"] = {"device_ms_median_best": row, "wall_ms": frame_ms, "moved_share": moved,
                                           "triangles": int(s.view.contents.num_tris)}
        print(f"{name} {w} x {h}: {100 * moved:.1f} % of the pixels moved", file=sys.stderr)
        for k, (med, best) in row.items():
            print(f"  {k:44} median {med:.4f} best {best:.4f} ms", file=sys.stderr)
        for k, v in frame_ms.items():
            print(f"  {k:44} {v:.3f} ms by the host clock", file=sys.stderr)
print(json.dumps(out))
