#!/usr/bin/env python3
"""What reprojecting through displacement buys: three sequences at 96 x 96, mis at 4 spp, frame 0 standing
and four frames each after an update_geometry,
  panel    tests/test_motion.py's: cornell_box_spheres plus a 150 x 150 panel moved by (36, 0, -24) per frame
  sphere   cornell_box_spheres' white sphere (radius 90) moved by (24, 0, -16) per frame - a sixth of the box in four
           frames, under a light 250 units above it - and "sphere, slow" by a quarter of that, with sigma_plane = 0.01: at
           the default 0.00005 x depth the plane test rejects the NEIGHBOURING taps of a surface this curved at this
           resolution whether or not it moves (a pixel is 8 units wide, the sphere's sagitta over it 0.36 units, the
           tolerance 0.05), so without the wider plane test neither run keeps a sphere's history
walked by the plain, the sparse (stride 2) and the variance-guided preview, each with and without ``motion``.  Per run:
e = mean((x - ref)^2 / (ref^2 + 0.01)) of the last frame against mis at 1024 spp of the final scene, over the moved
object's pixels (centre hit on it, eroded by 2 px) and over the whole picture, and the object's median history length.
Prints a table to stderr and one JSON line.

  tools/motion_sweep.py"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch
import scenes
import test_motion as T
from test_temporal import rse
from vimg_amd import hip, motion

RES, MOVES = T.RES, T.MOVES
PREVIEWS = {"plain": dict(denoise=False), "sparse 2": dict(denoise=False, sparse=2), "variance-guided": dict(variance_guided=True)}
SPHERE, SPHERE_STEP = 2, np.array([24, 0, -16, 0], np.float32)


def panel_case():
    s = T.panel_scene()
    return s, T.panel_prims(s), (lambda dev, k: dev.update_geometry(vertices=T.moved_vertices(s, k))), {}


def sphere_case(speed=1.0):
    s = scenes.json_scene("cornell_box_spheres.json", res=(RES, RES))
    prims = motion.prim_records(s)
    which = np.array([i for i, (kind, index) in enumerate(prims) if kind == 1 and index == SPHERE])

    def move(dev, k):
        sp = s.geometry()[2]
        sp[SPHERE] += np.float32(k * speed) * SPHERE_STEP
        dev.update_geometry(spheres=sp)
    return s, which, move, dict(sigma_plane=0.01)


hip.init(0)
out = {}
for case, make in (("panel", panel_case), ("sphere", sphere_case), ("sphere, slow", lambda: sphere_case(0.25))):
    s, object_prims, move, kw = make()
    p = s.default_params(integrator="mis", samples=4)
    for name, pkw in PREVIEWS.items():
        dev = hip.DeviceScene(s)
        runs = {"motion": dev.temporal_preview(p, samples=4, motion=s, **pkw, **kw), "without": dev.temporal_preview(p, samples=4, **pkw, **kw)}
        for k in range(MOVES + 1):
            if k:
                move(dev, k)
            frames = {r: pv.frame().cpu().numpy() for r, pv in runs.items()}
        rays = dev.camera_rays(torch.from_numpy(motion.centre_samples(RES, RES)).cuda())
        on = np.isin(dev.trace_rays(rays).prim.cpu().numpy().reshape(RES, RES), object_prims)
        inner = T.erode(on)
        ref = dev.render(s.default_params(integrator="mis", samples=1024), stats=False).cpu().numpy()
        row = {}
        for r, pv in runs.items():
            row[r] = dict(object=rse(frames[r][inner], ref[inner]), picture=rse(frames[r], ref),
                          length=float(np.median(pv.history.length.cpu().numpy()[inner])))
            pv.close()
        dev.close()
        out[f"{case}, {name}"] = dict(pixels=int(inner.sum()), **row)
        a, b = row["motion"], row["without"]
        print(f"{case:12} {name:16} {inner.sum():4d} px  object e {a['object']:.5f} / {b['object']:.5f} (x{b['object'] / a['object']:.2f})  "
              f"picture e {a['picture']:.5f} / {b['picture']:.5f}  median length {a['length']:.3f} / {b['length']:.3f}   (motion / without)",
              file=sys.stderr)
print(json.dumps(out))
