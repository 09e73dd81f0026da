#!/usr/bin/env python3
"""Cost and defaults of temporal accumulation with luminance moments.
  cost    disney_spheres at 450 x 200 and 1800 x 800: one moments.accumulate call (a history one orbit step old, so the
          taps are real gathers; a variance frame; both outputs) beside one temporal.accumulate call on the same frames
          in the same process, the two alternating in `rounds` rounds; device events around each call, median and best
          of `steps` calls after two warm-up calls, and the ratio of the medians per round.  Bytes per pixel with one
          tap: temporal 48 read + 48 gathered + 60 written = 156, moments 52 + 64 + 80 = 196, so about 1.25 x.
  orbit   the orbit of tools/temporal_cost.py (8 steps of 1.5 degrees, mis at 4 spp) on cornell_box_spheres (64 x 64 and
          256 x 256) and disney_spheres (450 x 200): the frames are rendered once and accumulated by hand as a preview
          accumulates them (every frame follows a camera move: current_weight 1, no variance frame).
          e = mean((x - ref)^2 / (ref^2 + 0.01)) against mis at 1024 spp from the last camera of: the noisy frame;
          temporal + the fixed a-trous filter at sigma_color / sqrt(9) (today's preview); temporal + the variance-guided
          filter with the variance the moments give; the variance-guided filter on the noisy frame alone.  Also
          mean(V) / mean((Y(A) - Y(ref))^2) over the live pixels with known V (and the ratio of the medians, which a few
          large errors do not carry), and the sweep of min_history 2, 3, 4, 6, 8
          with the geometric mean of e over the three frames.
Prints tables to stderr and one JSON line.

  tools/moments_cost.py [--steps N] [--rounds N] [--no-orbit] [--no-cost]"""
import argparse, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=15)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-orbit", action="store_true")
ap.add_argument("--no-cost", action="store_true")
args = ap.parse_args()

import numpy as np
import torch
import scenes
from vimg_amd import filter as flt, hip, moments, temporal, varfilter
from _timing import timed

ORBIT_STEPS, DEGREES = 8, 1.5
MIN_HISTORY = (2, 3, 4, 6, 8)
VIEWS = {"cornell_box_spheres.json": ((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0),
         "disney_spheres.json": ((0.0, 20.0, 1600.0), (0.0, -4.0, 0.0), 25.0)}
Y = (0.212671, 0.715160, 0.072169)


def orbit_camera(name, i):
    """Step i of the orbit of tools/temporal_cost.py: the eye revolves about the vertical axis through a pivot 1.7 times
    as far as the look-at point and keeps its viewing direction."""
    eye0, at0, vfov = (np.array(v) if k < 2 else v for k, v in enumerate(VIEWS[name]))
    pivot = eye0 + 1.7 * (at0 - eye0)
    a, r = math.radians(DEGREES * i), eye0 - pivot
    eye = pivot + np.array([r[0] * math.cos(a) + r[2] * math.sin(a), r[1], -r[0] * math.sin(a) + r[2] * math.cos(a)])
    return eye, eye + (at0 - eye0), (0.0, 1.0, 0.0), vfov


def rse(x, ref):
    return float((((x.cpu().numpy().astype(np.float64) - ref) ** 2) / (ref ** 2 + 0.01)).mean())


hip.init(0)
out = {"steps": args.steps, "rounds": args.rounds, "bytes_per_pixel_one_tap": {"temporal": 156, "moments": 196}}

if not args.no_cost:
    out["cost"] = {}
    name = "disney_spheres.json"
    for res in ((450, 200), (1800, 800)):
        w, h = res
        s = scenes.json_scene(name, res=res)
        dev = hip.DeviceScene(s)
        p = s.default_params(integrator="mis", samples=4)
        dev.set_camera(*orbit_camera(name, 0))
        g0 = dev.render_features(p, flt.GUIDES)
        first = dev.render(p, stats=False)
        hist_m = moments.accumulate(first, g0["normal"], g0["position"], g0["depth"], world_to_pixel=moments.world_to_pixel(dev.camera))
        hist_t = temporal.History(hist_m.tensor[:3].clone(), hist_m.world_to_pixel)
        dev.set_camera(*orbit_camera(name, 1))
        acc = dev.progressive(p)
        acc.render(2, out=False)
        noisy = acc.render(2)                      # 4 spp in two increments: the accumulator knows a variance
        var = acc.variance()
        acc.close()
        g = dev.render_features(p, flt.GUIDES)
        nxt_m, nxt_t, rgb, out_var = torch.empty_like(hist_m.tensor), torch.empty_like(hist_t.tensor), torch.empty_like(noisy), torch.empty_like(var)
        frames = (noisy, g["normal"], g["position"], g["depth"])
        run_t = lambda: temporal.accumulate(*frames, history=hist_t, out=rgb, next_history=nxt_t)
        run_m = lambda: moments.accumulate(*frames, variance=var, history=hist_m, out=rgb, out_variance=out_var, next_history=nxt_m)
        rounds = []
        for _ in range(args.rounds):               # alternating: other people's work shares the machine
            t, m = timed(run_t, args.steps), timed(run_m, args.steps)
            rounds.append({"temporal_ms": t, "moments_ms": m, "ratio_of_medians": m[0] / t[0]})
        same = bool(torch.equal(nxt_m[:3].view(torch.int32), nxt_t.view(torch.int32)))
        row = {"live_fraction": float((g["depth"][..., 0] > 0).float().mean()), "with_history_fraction": float((nxt_m[0, ..., 3] > 1).float().mean()),
               "known_variance_out_fraction": float(((out_var >= 0) & (out_var < math.inf)).float().mean()),
               "planes_0_to_2_equal_temporal": same, "rounds": rounds,
               "ratio_median_of_rounds": float(np.median([r["ratio_of_medians"] for r in rounds]))}
        dev.close()
        out["cost"][f"{w}x{h}"] = row
        print(f"{w} x {h}  ({row['live_fraction'] * 100:.1f} % live pixels, {row['with_history_fraction'] * 100:.1f} % find history, "
              f"planes 0..2 equal temporal's: {same})", file=sys.stderr)
        for r in rounds:
            (tm, tb), (mm, mb) = r["temporal_ms"], r["moments_ms"]
            print(f"  temporal median {tm:7.4f} ms best {tb:7.4f} ms ({156 * w * h / tm / 1e6:7.1f} GB/s at 156 B/pixel)   "
                  f"moments median {mm:7.4f} ms best {mb:7.4f} ms ({196 * w * h / mm / 1e6:7.1f} GB/s at 196 B/pixel)   "
                  f"ratio {r['ratio_of_medians']:.3f}", file=sys.stderr)

if not args.no_orbit:
    out["orbit"] = {}
    sigma_color = flt.atrous_params().sigma_color
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
        guides = (g["normal"], g["position"], g["depth"])

        def walk(mod, **kw):
            hist = None
            for c, gg, m in frames:
                hist = mod.accumulate(c, gg["normal"], gg["position"], gg["depth"], history=hist, world_to_pixel=m, **kw)
            return hist

        ht = walk(temporal)
        n = min(float(len(frames)), temporal.temporal_params().max_history)
        fixed = flt.atrous(ht.color.contiguous(), *guides, albedo=g["albedo"], sigma_color=sigma_color / math.sqrt(n))
        row = dict(e_noisy=rse(noisy, ref), e_temporal=rse(ht.color, ref), e_temporal_fixed=rse(fixed, ref),
                   e_guided_alone=rse(varfilter.atrous(noisy, *guides, albedo=g["albedo"])[0], ref), by_min_history={})
        lum = lambda a: a[..., 0] * Y[0] + a[..., 1] * Y[1] + a[..., 2] * Y[2]
        for mh in MIN_HISTORY:
            hm = walk(moments, min_history=mh)
            assert torch.equal(hm.tensor[:3].view(torch.int32), ht.tensor.view(torch.int32))
            V = hm.variance.contiguous()
            guided = varfilter.atrous(hm.color.contiguous(), *guides, albedo=g["albedo"], variance=V)[0]
            Vn, A, live = V.cpu().numpy().astype(np.float64), hm.color.cpu().numpy().astype(np.float64), (hm.tensor[1, ..., 3] > 0).cpu().numpy()
            sel = live & (Vn >= 0) & (Vn < np.inf)
            err2 = (lum(A) - lum(ref)) ** 2
            row["by_min_history"][mh] = dict(e_temporal_guided=rse(guided, ref), known_fraction_of_live=float(sel.sum() / max(1, live.sum())),
                                             v_ratio=float(Vn[sel].mean() / err2[sel].mean()) if sel.any() else None,
                                             v_ratio_of_medians=float(np.median(Vn[sel]) / np.median(err2[sel])) if sel.any() else None)
        key = f"{name.split('.')[0]} {res[0]}x{res[1]}"
        out["orbit"][key] = row
        print(f"{key}: e noisy {row['e_noisy']:.5f}  temporal {row['e_temporal']:.5f}  temporal + fixed {row['e_temporal_fixed']:.5f}  "
              f"guided alone {row['e_guided_alone']:.5f}", file=sys.stderr)
        for mh, r in row["by_min_history"].items():
            print(f"  min_history {mh}: temporal + guided {r['e_temporal_guided']:.5f}   known V on {100 * r['known_fraction_of_live']:.1f} % of live   "
                  f"mean(V) / mean(err^2) {r['v_ratio']:.4f}   median(V) / median(err^2) {r['v_ratio_of_medians']:.4f}", file=sys.stderr)
        dev.close()
    geo = {mh: float(np.exp(np.mean([math.log(r["by_min_history"][mh]["e_temporal_guided"]) for r in out["orbit"].values()]))) for mh in MIN_HISTORY}
    out["geometric_mean_e_by_min_history"] = geo
    out["geometric_mean_e_temporal_fixed"] = float(np.exp(np.mean([math.log(r["e_temporal_fixed"]) for r in out["orbit"].values()])))
    print("geometric mean of e(temporal + guided) by min_history: " + "  ".join(f"{mh}: {v:.5f}" for mh, v in geo.items())
          + f"   temporal + fixed: {out['geometric_mean_e_temporal_fixed']:.5f}", file=sys.stderr)
    out["default_min_history"] = float(moments.params().min_history)
print(json.dumps(out))
