#!/usr/bin/env python3
"""Cost of a new tree for a resident scene: config 5 at its default size (~1 M triangles, 1024^2
textures), every vertex moved by a large deformation (a twist of two turns about the vertical axis through the
centroid plus a seeded jitter).  Reports, best of `reps` after a warm-up:
  rebuild_ms / rebuild_device_ms   host wall clock around DeviceScene.rebuild_bvh (blocking), and the same span by
                                   device events recorded on the stream before and after the call
  host_route_ms                    what the library offered before for the same result: HostScene.set_vertices +
                                   build_bvh_with(hip.ploc_builder()) + a new DeviceScene (its three parts too)
  cost_*                           bvh_cost as uploaded (host sweep tree), after the refit, after the rebuild
  mrays_refit / mrays_rebuilt      a 16 spp render on the refit tree and on the rebuilt one
and checks that the rebuilt scene and the host route's scene render the same bits and event counts.  One JSON
line.  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats` (kernels scene_rebuild_*, ploc_*, emit_*)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import scenes
from vimg_amd import hip

hip.init(0)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
s = scenes.config5_scene()
view = s.view.contents
v0, n0, _ = s.geometry()
p64 = v0.astype(np.float64)
c, y0, y1 = p64.mean(0), p64[:, 1].min(), p64[:, 1].max()
ang = 2.0 * np.pi * 2.0 * (p64[:, 1] - y0) / (y1 - y0)
x, z = p64[:, 0] - c[0], p64[:, 2] - c[2]
v1 = p64.copy()
v1[:, 0], v1[:, 2] = c[0] + np.cos(ang) * x - np.sin(ang) * z, c[2] + np.sin(ang) * x + np.cos(ang) * z
v1 = (v1 + np.random.default_rng(0x5EED).normal(0.0, 0.01, v1.shape)).astype(np.float32)
dv1 = torch.from_numpy(v1).cuda()
stream = torch.cuda.current_stream()
p = s.default_params(samples=16, depth=4)


def mrays(d):
    _, st = d.render(p)
    best = 1e30
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        d.render(p, stats=False)
        b.record(stream)
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return st.rays / best / 1e3


d = hip.DeviceScene(s)
cost_uploaded = d.bvh_cost()
d.update_geometry(vertices=dv1)
cost_refit = d.bvh_cost()
mrays_refit = mrays(d)
wall, dev = [], []
for k in range(reps + 1):               # every rebuild starts from the same positions and gives the same tree
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(stream)
    t0 = time.perf_counter()
    d.rebuild_bvh()
    wall.append(time.perf_counter() - t0)
    b.record(stream)
    b.synchronize()
    dev.append(a.elapsed_time(b))
cost_rebuilt = d.bvh_cost()
mrays_rebuilt = mrays(d)

route, parts = [], []
for k in range(reps + 1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.set_vertices(v1)
    t1 = time.perf_counter()
    s.build_bvh_with(hip.ploc_builder())
    t2 = time.perf_counter()
    fresh = hip.DeviceScene(s)
    t3 = time.perf_counter()
    route.append(t3 - t0)
    parts.append((t1 - t0, t2 - t1, t3 - t2))
    if k < reps:
        fresh.close()
q = s.default_params(samples=1, depth=4)
img, st = d.render_to_host(q)
ref, rst = fresh.render_to_host(q)
same = bool(np.array_equal(img.view(np.uint32), ref.view(np.uint32))) and st.as_dict() == rst.as_dict()
best = int(np.argmin(route[1:])) + 1
print(json.dumps({"scene": "config5", "triangles": int(view.num_tris), "vertices": int(view.num_vertices),
                  "nodes_rebuilt": int(s.view.contents.bvh.num_nodes),
                  "rebuild_ms": round(min(wall[1:]) * 1e3, 3), "rebuild_ms_median": round(float(np.median(wall[1:])) * 1e3, 3),
                  "rebuild_device_ms": round(min(dev[1:]), 3),
                  "host_route_ms": round(route[best] * 1e3, 2), "host_route_ms_median": round(float(np.median(route[1:])) * 1e3, 2),
                  "host_route_set_vertices_ms": round(parts[best][0] * 1e3, 2), "host_route_build_ms": round(parts[best][1] * 1e3, 2),
                  "host_route_upload_ms": round(parts[best][2] * 1e3, 2),
                  "cost_uploaded": round(cost_uploaded, 4), "cost_refit": round(cost_refit, 4), "cost_rebuilt": round(cost_rebuilt, 4),
                  "mrays_refit": round(mrays_refit, 1), "mrays_rebuilt": round(mrays_rebuilt, 1),
                  "bit_identical_to_host_route": same, "scene_bytes_equal": d.bytes == fresh.bytes}), flush=True)
assert same and d.bytes == fresh.bytes
