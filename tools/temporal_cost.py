#!/usr/bin/env python3
"""Cost and defaults of temporal accumulation.
  cost    disney_spheres at 1800 x 800 and 1366 x 768: one temporal.accumulate call (a history one orbit step old, so
          the taps are real gathers), beside one 4 spp mis increment (Progressive.render(4)) and one 3-iteration a-trous
          call in the same session; device events around each call, median and best of `steps` calls after two warm-up
          calls.  Bytes per pixel: 60 read, up to 4 taps x 44 gathered (16 of plane A, 12 of each guide
          plane, whose fourth component is not read), 48 + 12 written.
          Also a whole TemporalPreview.frame() - after a set_camera (reset, four feature frames, 4 spp, accumulate,
          a-trous) and standing still (4 spp, accumulate, a-trous) - by the host clock around synchronised calls.
  sweep   the orbit of tests/test_temporal.py (the eye on a circle, 1.5 degrees per step, viewing direction kept; 8 steps,
          mis at 4 spp; the pivot is 1.7 times as far as the look-at point, z = 560 on cornell_box_spheres, 4 units
          behind the test's) on cornell_box_spheres (64 x 64 and 256 x 256) and disney_spheres (450 x 200): the frames are
          rendered once and accumulated again under every setting of max_history x sigma_normal x sigma_plane;
          e = mean((x - ref)^2 / (ref^2 + 0.01)) of the last frame against mis at 1024 spp from the last camera, over
          the noisy frame's; with the library's defaults also the a-trous filter alone and behind the accumulation, the
          latter for sigma_color 2 .. 0.2 at 3, 2 and 1 iterations (what TemporalPreview's sigma_color / sqrt(n) rests on).
Prints tables to stderr and one JSON line.

  tools/temporal_cost.py [--steps N] [--no-sweep] [--no-cost]"""
import argparse, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7)
ap.add_argument("--no-sweep", action="store_true")
ap.add_argument("--no-cost", action="store_true")
args = ap.parse_args()

import numpy as np
import torch
import scenes
from vimg_amd import filter as flt, hip, temporal
from _timing import timed, wall

ORBIT_STEPS, DEGREES = 8, 1.5
MAX_HISTORY, SIGMA_NORMAL, SIGMA_PLANE = (2, 4, 8, 16, 32), (0.02, 0.1, 0.5), (0.00001, 0.00002, 0.00005, 0.0001, 0.0002, 0.0005, 0.002, 0.01)
SIGMA_COLOR, ITERATIONS = (2, 1.4, 1, 0.67, 0.5, 0.33, 0.2), (3, 2, 1)
VIEWS = {"cornell_box_spheres.json": ((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0),
         "disney_spheres.json": ((0.0, 20.0, 1600.0), (0.0, -4.0, 0.0), 25.0)}


def orbit_camera(name, i):
    """Step i: the eye revolves about the vertical axis through a pivot 1.7 times as far as the look-at point (on
    cornell_box_spheres the back wall's centre) and keeps its viewing direction."""
    eye0, at0, vfov = (np.array(v) if k < 2 else v for k, v in enumerate(VIEWS[name]))
    pivot = eye0 + 1.7 * (at0 - eye0)
    a, r = math.radians(DEGREES * i), eye0 - pivot
    eye = pivot + np.array([r[0] * math.cos(a) + r[2] * math.sin(a), r[1], -r[0] * math.sin(a) + r[2] * math.cos(a)])
    return eye, eye + (at0 - eye0), (0.0, 1.0, 0.0), vfov


def rse(x, ref):
    return float((((x - ref) ** 2) / (ref ** 2 + 0.01)).mean())


hip.init(0)
out = {"steps": args.steps, "bytes_per_pixel": {"read": 60, "gathered_at_most": 176, "written": 60}}

if not args.no_cost:
    out["cost"] = {}
    name = "disney_spheres.json"
    for res in ((1800, 800), (1366, 768)):
        w, h = res
        s = scenes.json_scene(name, res=res)
        dev = hip.DeviceScene(s)
        p = s.default_params(integrator="mis", samples=4)
        dev.set_camera(*orbit_camera(name, 0))
        g0 = dev.render_features(p, flt.GUIDES)
        hist = temporal.accumulate(dev.render(p, stats=False), g0["normal"], g0["position"], g0["depth"],
                                   world_to_pixel=temporal.world_to_pixel(dev.camera))
        dev.set_camera(*orbit_camera(name, 1))
        noisy = dev.render(p, stats=False)
        g = dev.render_features(p, flt.GUIDES)
        nxt, rgb = torch.empty_like(hist.tensor), torch.empty_like(noisy)
        work = torch.empty(flt.atrous_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
        row = {"live_fraction": float((g["depth"][..., 0] > 0).float().mean())}
        row["accumulate_ms"] = timed(lambda: temporal.accumulate(noisy, g["normal"], g["position"], g["depth"], history=hist, out=rgb,
                                                                 next_history=nxt), args.steps)
        row["with_history_fraction"] = float((nxt[0, ..., 3] > 1).float().mean())
        row["accumulate_no_history_ms"] = timed(lambda: temporal.accumulate(noisy, g["normal"], g["position"], g["depth"], out=rgb,
                                                                            next_history=nxt), args.steps)
        row["atrous_3_ms"] = timed(lambda: flt.atrous(noisy, g["normal"], g["position"], g["depth"], albedo=g["albedo"], iterations=3,
                                                      out=rgb, workspace=work), args.steps)
        acc = dev.progressive(p)
        row["mis_4spp_increment_ms"] = timed(lambda: acc.render(4, out=rgb), args.steps)
        acc.close()

        pv = dev.temporal_preview(p, samples=4)

        def moved(i):
            dev.set_camera(*orbit_camera(name, i % 2))
            pv.frame()

        row["frame_after_set_camera_ms"] = wall(moved, args.steps)
        row["frame_standing_still_ms"] = wall(lambda i: pv.frame(), args.steps)
        pv.close()
        dev.close()
        out["cost"][f"{w}x{h}"] = row
        print(f"{w} x {h}  ({row['live_fraction'] * 100:.1f} % live pixels, {row['with_history_fraction'] * 100:.1f} % find history)", file=sys.stderr)
        print(f"  whole frame(): after set_camera {row['frame_after_set_camera_ms']:.3f} ms, standing still "
              f"{row['frame_standing_still_ms']:.3f} ms (host clock, synchronised)", file=sys.stderr)
        for k in ("accumulate_ms", "accumulate_no_history_ms", "atrous_3_ms", "mis_4spp_increment_ms"):
            med, best = row[k]
            extra = f"   {236 * w * h / med / 1e6:8.1f} GB/s at 236 B/pixel" if k == "accumulate_ms" else ""
            print(f"  {k:28} median {med:8.3f} ms  best {best:8.3f} ms{extra}", file=sys.stderr)

if not args.no_sweep:
    out["sweep"] = {}
    lib_defaults = temporal.temporal_params()
    defaults = (lib_defaults.max_history, round(lib_defaults.sigma_normal, 6), round(lib_defaults.sigma_plane, 6))
    grid = [(mh, sn, sp) for mh in MAX_HISTORY for sn in SIGMA_NORMAL for sp in SIGMA_PLANE]
    for name, res in (("cornell_box_spheres.json", (64, 64)), ("cornell_box_spheres.json", (256, 256)), ("disney_spheres.json", (450, 200))):
        s = scenes.json_scene(name, res=res)
        dev = hip.DeviceScene(s)
        p = s.default_params(integrator="mis", samples=4)
        frames = []
        for i in range(ORBIT_STEPS + 1):
            dev.set_camera(*orbit_camera(name, i))
            frames.append((dev.render(p, stats=False), dev.render_features(p, flt.GUIDES), temporal.world_to_pixel(dev.camera)))
        ref = dev.render(s.default_params(integrator="mis", samples=1024), stats=False).cpu().numpy().astype(np.float64)
        noisy, g, _ = frames[-1]
        e_noisy = rse(noisy.cpu().numpy(), ref)
        e_atrous = rse(flt.atrous(noisy, g["normal"], g["position"], g["depth"], albedo=g["albedo"]).cpu().numpy(), ref)

        def walk(**kw):
            hist = None
            for c, gg, m in frames:
                hist = temporal.accumulate(c, gg["normal"], gg["position"], gg["depth"], history=hist, world_to_pixel=m, **kw)
            return hist

        rows = {}
        for mh, sn, sp in grid:
            hist = walk(max_history=mh, sigma_normal=sn, sigma_plane=sp)
            rows[f"{mh}/{sn}/{sp}"] = rse(hist.color.cpu().numpy(), ref) / e_noisy
        hist = walk()
        accumulated = hist.color.contiguous()
        both = flt.atrous(accumulated, g["normal"], g["position"], g["depth"], albedo=g["albedo"])
        by_sigma_color = {it: {sc: rse(flt.atrous(accumulated, g["normal"], g["position"], g["depth"], albedo=g["albedo"], iterations=it,
                                                  sigma_color=sc).cpu().numpy(), ref) for sc in SIGMA_COLOR} for it in ITERATIONS}
        key = f"{name.split('.')[0]} {res[0]}x{res[1]}"
        out["sweep"][key] = dict(e_noisy=e_noisy, e_atrous=e_atrous, e_temporal=rse(hist.color.cpu().numpy(), ref),
                                 e_temporal_atrous=rse(both.cpu().numpy(), ref), median_length=float(hist.length.median()),
                                 with_history=float((hist.length > 1).float().mean()), ratio=rows,
                                 e_temporal_atrous_by_iterations_and_sigma_color=by_sigma_color)
        r = out["sweep"][key]
        print(f"{key}: e noisy {e_noisy:.5f}  a-trous {e_atrous:.5f}  temporal {r['e_temporal']:.5f}  temporal + a-trous "
              f"{r['e_temporal_atrous']:.5f}   median length {r['median_length']:.1f}, {100 * r['with_history']:.1f} % with history",
              file=sys.stderr)
        for it in ITERATIONS:
            print(f"  e(temporal + a-trous), {it} iterations: " + "  ".join(f"sigma_color {sc}: {by_sigma_color[it][sc]:.5f}" for sc in SIGMA_COLOR),
                  file=sys.stderr)
        print("  e_temporal / e_noisy by max_history (rows) and sigma_normal / sigma_plane (columns)", file=sys.stderr)
        cols = [(sn, sp) for sn in SIGMA_NORMAL for sp in SIGMA_PLANE]
        print("        " + " ".join(f"{sn:>4}/{sp:<6}" for sn, sp in cols), file=sys.stderr)
        for mh in MAX_HISTORY:
            print(f"  {mh:4}  " + " ".join(f"{rows[f'{mh}/{sn}/{sp}']:11.3f}" for sn, sp in cols), file=sys.stderr)
        dev.close()
    out["defaults"] = defaults
print(json.dumps(out))
