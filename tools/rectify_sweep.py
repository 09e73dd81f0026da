#!/usr/bin/env python3
"""The defaults of ``rectify`` (libvimg_rectify.so and the preview's fast_history): fast_history 2 / 4 / 8 x
radius 1..3 x k 1 / 1.5 / 2 / 3 / 4 x cut 0 / 0.5 / 1, 135 settings, mis at 4 spp, e = mean((x - ref)^2 / (ref^2 + 0.01))
against mis at 1024 spp of the scene as it then stands, no ``antilag`` unless said:
  (i)   NO EDIT: the three orbits of 4.19 (8 steps of 1.5 degrees; cornell_box_spheres 64 x 64 and 256 x 256, disney_spheres
        450 x 200), unfiltered: e of the last frame, and the share of pixels clamped on it
  (ii)  EDIT, light: cornell_box_spheres 64 x 64, after the orbit's nine frames the light's emission times 0.25, and times
        4; frames 1 - 8 after the edit with the camera standing; the same two with ``antilag=True``
  (iii) EDIT, motion: 4.28's rows where ``motion`` loses today, at 96 x 96 with ``motion=``: the moved panel under the
        variance-guided filter, the fast white sphere unfiltered and under the variance-guided filter (sigma_plane 0.01);
        e of the last of four moved frames over the object's pixels, beside the same preview without ``motion`` and
        without ``rectify`` - the run 4.28 compares with
Every run is a TemporalPreview, so what is measured is what ships; the previews of one leg stand side by side on one
resident scene and render the same increments.  A leg's figure is the geometric mean of its e's; a setting is ELIGIBLE when
the geometric mean of its three (i) is within 2 % of the plain preview's in the same run, and the default is the eligible
setting with the lowest geometric mean over the seven legs of (ii) and (iii).  cornell's orbit is tests/test_temporal.py's,
so the 64 x 64 row of (i) is what tests/test_rectify.py bounds.  Prints tables to stderr and one JSON line.

  tools/rectify_sweep.py [--quick]      (--quick: 12 settings, for a look at the tool itself)"""
import argparse, itertools, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true")
args = ap.parse_args()

import numpy as np
import torch
import scenes
import test_motion as T
from vimg_amd import hip, motion, preview as pv, rectify

ORBIT_STEPS, DEGREES, AFTER = 8, 1.5, 8
FAST, RADII, KS, CUTS = (2, 4, 8), (1, 2, 3), (1.0, 1.5, 2.0, 3.0, 4.0), (0.0, 0.5, 1.0)
if args.quick:
    FAST, RADII, KS, CUTS = (2, 4), (1, 2), (1.0, 2.0, 4.0), (0.5,)
SETTINGS = [dict(fast_history=f, radius=r, k=k, cut=c) for f, r, k, c in itertools.product(FAST, RADII, KS, CUTS)]
# eye, viewing direction, pivot, vfov: 4.19's orbits
VIEWS = {"cornell_box_spheres.json": ((278.0, 278.0, -800.0), (0.0, 0.0, 800.0), (278.0, 278.0, 556.0), 40.0),
         "disney_spheres.json": ((0.0, 20.0, 1600.0), (0.0, -24.0, -1600.0), (0.0, -20.8, -1120.0), 25.0)}
PICTURES = (("cornell_box_spheres.json", (64, 64)), ("cornell_box_spheres.json", (256, 256)), ("disney_spheres.json", (450, 200)))
SPHERE, SPHERE_STEP = 2, np.array([24, 0, -16, 0], np.float32)


def orbit_camera(name, i):
    eye0, ahead, pivot = (np.array(v) for v in VIEWS[name][:3])
    a, r = math.radians(DEGREES * i), eye0 - pivot
    eye = pivot + np.array([r[0] * math.cos(a) + r[2] * math.sin(a), r[1], -r[0] * math.sin(a) + r[2] * math.cos(a)])
    return eye, eye + ahead, (0.0, 1.0, 0.0), VIEWS[name][3]


def rse(x, ref, where=None):
    x = x.cpu().numpy().astype(np.float64)
    if where is not None:
        x, ref = x[where], ref[where]
    return float((((x - ref) ** 2) / (ref ** 2 + 0.01)).mean())


def key(setting):
    return "plain" if setting is None else f"h{setting['fast_history']} r{setting['radius']} k{setting['k']:g} c{setting['cut']:g}"


def previews(dev, p, **kw):
    """key -> a preview of ``dev`` per setting, the plain one first."""
    return {key(x): dev.temporal_preview(p, samples=4, rectify=x, **kw) for x in [None] + SETTINGS}


def step(runs):
    return {k: v.frame() for k, v in runs.items()}


def close(runs):
    for v in runs.values():
        v.close()


geo = lambda xs: float(np.exp(np.mean(np.log(xs))))
hip.init(0)
out = {"settings": [key(x) for x in SETTINGS], "no_edit": {}, "edit": {}, "without_motion": {}}
many = dict(integrator="mis", samples=1024)

# (i) and (ii)
for name, res in PICTURES:
    w, h = res
    pic = f"{name.split('.')[0]} {w}x{h}"
    s = scenes.json_scene(name, res=res)
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    runs = previews(dev, p, denoise=False)
    for i in range(ORBIT_STEPS + 1):
        dev.set_camera(*orbit_camera(name, i))
        frames = step(runs)
    ref = dev.render(s.default_params(**many), stats=False).cpu().numpy().astype(np.float64)
    out["no_edit"][pic] = {k: {"e": rse(frames[k], ref),
                               "clamped": 0.0 if k == "plain" else float((runs[k].last_rectify_code == 1).float().mean())} for k in runs}
    print(f"(i) {pic}: plain e {out['no_edit'][pic]['plain']['e']:.5f}", file=sys.stderr)
    close(runs)
    dev.close()
    if res != (64, 64):
        continue
    for what, factor in (("light x 0.25", 0.25), ("light x 4", 4.0)):
        for lag in (False, True):
            dev = hip.DeviceScene(s)
            runs = previews(dev, p, denoise=False, antilag=lag)
            for i in range(ORBIT_STEPS + 1):
                dev.set_camera(*orbit_camera(name, i))
                step(runs)
            mats = s.materials()
            for mat in mats:
                if max(mat.emit[0], mat.emit[1], mat.emit[2]) > 0:
                    mat.emit[0], mat.emit[1], mat.emit[2] = mat.emit[0] * factor, mat.emit[1] * factor, mat.emit[2] * factor
            dev.update_materials(materials=mats)
            ref = dev.render(s.default_params(**many), stats=False).cpu().numpy().astype(np.float64)
            cell = {k: [] for k in runs}
            for _ in range(AFTER):
                for k, x in step(runs).items():
                    cell[k].append(rse(x, ref))
            leg = f"{what}{', antilag' if lag else ''}"
            out["edit"][leg] = cell
            print(f"(ii) {leg}: plain e of frames 1..{AFTER} " + " ".join(f"{e:.5f}" for e in cell["plain"]), file=sys.stderr)
            close(runs)
            dev.close()


# (iii)
def panel_case():
    s = T.panel_scene()
    return s, T.panel_prims(s), (lambda dev, k: dev.update_geometry(vertices=T.moved_vertices(s, k))), {}


def sphere_case():
    s = scenes.json_scene("cornell_box_spheres.json", res=(T.RES, T.RES))
    prims = motion.prim_records(s)
    which = np.array([i for i, (kind, index) in enumerate(prims) if kind == 1 and index == SPHERE])

    def move(dev, k):
        sp = s.geometry()[2]
        sp[SPHERE] += np.float32(k) * SPHERE_STEP
        dev.update_geometry(spheres=sp)
    return s, which, move, dict(sigma_plane=0.01)


for leg, make, pkw in (("panel, motion, variance-guided", panel_case, dict(variance_guided=True)),
                       ("sphere, motion, unfiltered", sphere_case, dict(denoise=False)),
                       ("sphere, motion, variance-guided", sphere_case, dict(variance_guided=True))):
    s, object_prims, move, kw = make()
    p = s.default_params(integrator="mis", samples=4)
    dev = hip.DeviceScene(s)
    runs = previews(dev, p, motion=s, **pkw, **kw)
    runs["without motion"] = dev.temporal_preview(p, samples=4, **pkw, **kw)
    for k in range(T.MOVES + 1):
        if k:
            move(dev, k)
        frames = step(runs)
    rays = dev.camera_rays(torch.from_numpy(motion.centre_samples(T.RES, T.RES)).cuda())
    inner = T.erode(np.isin(dev.trace_rays(rays).prim.cpu().numpy().reshape(T.RES, T.RES), object_prims))
    ref = dev.render(s.default_params(**many), stats=False).cpu().numpy().astype(np.float64)
    cell = {k: [rse(frames[k], ref, inner)] for k in runs}
    out["without_motion"][leg] = cell.pop("without motion")[0]
    out["edit"][leg] = cell
    print(f"(iii) {leg}: object e with motion {cell['plain'][0]:.5f}, without {out['without_motion'][leg]:.5f} ({int(inner.sum())} px)", file=sys.stderr)
    close(runs)
    dev.close()

legs = list(out["edit"])
summary = {}
for k in ["plain"] + out["settings"]:
    summary[k] = {"no_edit": geo([row[k]["e"] for row in out["no_edit"].values()]),
                  "no_edit_each": [row[k]["e"] for row in out["no_edit"].values()],
                  "clamped": [row[k]["clamped"] for row in out["no_edit"].values()],
                  "legs": [geo(out["edit"][leg][k]) for leg in legs]}
    summary[k]["edit"] = geo(summary[k]["legs"])
base, base_edit = summary["plain"]["no_edit"], summary["plain"]["edit"]
print("legs: " + " | ".join(legs), file=sys.stderr)
print(f"| setting | (i) geo e | / plain | (i) e each | clamped on (i) | (ii, iii) geo e | / plain | " + " | ".join(legs) + " |", file=sys.stderr)
print("|---" * (8 + len(legs)) + "|", file=sys.stderr)
for k, v in summary.items():
    print(f"| {k} | {v['no_edit']:.5f} | {v['no_edit'] / base:.4f} | " + " ".join(f"{e:.5f}" for e in v["no_edit_each"]) + " | "
          + " ".join(f"{100 * t:.1f}" for t in v["clamped"]) + f" % | {v['edit']:.5f} | {v['edit'] / base_edit:.4f} | "
          + " | ".join(f"{e:.5f}" for e in v["legs"]) + " |", file=sys.stderr)
eligible = [k for k in out["settings"] if summary[k]["no_edit"] <= 1.02 * base]
nearest = min(out["settings"], key=lambda k: summary[k]["no_edit"])
best = min(eligible, key=lambda k: summary[k]["edit"]) if eligible else nearest
out.update(summary=summary, legs=legs, eligible=eligible, best=best, best_beats_plain=bool(summary[best]["edit"] < base_edit))
d = rectify.params()
out["shipped_default"] = key(dict(fast_history=int(pv.FAST_HISTORY), radius=d.radius, k=d.k, cut=d.cut))
ship = summary.get(out["shipped_default"])
print(f"{len(eligible)} of {len(SETTINGS)} settings keep (i) within 2 % of the plain preview; "
      + (f"lowest (ii, iii) among them: {best} ({summary[best]['edit'] / base_edit:.4f} of the plain preview's)" if eligible
         else f"none does - the nearest is {nearest} ({summary[nearest]['no_edit'] / base:.4f})")
      + f"; the shipped defaults are {out['shipped_default']}"
      + (f": (i) ratio {ship['no_edit'] / base:.4f}, each " + " ".join(f"{e / b:.4f}" for e, b in zip(ship["no_edit_each"], summary["plain"]["no_edit_each"]))
         + f", (ii, iii) ratio {ship['edit'] / base_edit:.4f}" if ship else ""), file=sys.stderr)
for leg in out["without_motion"]:
    i = legs.index(leg)
    print(f"motion + rectify on '{leg}': without motion {out['without_motion'][leg]:.5f}, motion alone {summary['plain']['legs'][i]:.5f}, "
          f"motion + {best} {summary[best]['legs'][i]:.5f}" + (f", motion + shipped {ship['legs'][i]:.5f}" if ship else ""), file=sys.stderr)
print(json.dumps(out))
