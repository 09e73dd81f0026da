#!/usr/bin/env python3
"""Cost of changing a resident scene: config 5 at its default size (~1 M triangles, 1024^2
textures), all vertex positions and normals replaced by a seeded displacement.  Reports, best of `reps`
after a warm-up:
  update_ms        host wall clock around DeviceScene.update_geometry (device tensors in, blocking call)
  update_device_ms the re-bake and refit kernels (and the 24-byte root read-back) on the stream, by device
                   events recorded before and after the call
  set_camera_ms    host wall clock around DeviceScene.set_camera
  upload_ms        a full vimg_hip_scene_upload of the same host scene (the host bake + copies)
and checks that one sample per pixel of the updated scene is bit for bit the fresh upload of the host scene
with the same positions and a refit tree.  One JSON line.  Per-kernel times: run it under
`rocprofv3 --kernel-trace --stats` (kernels scene_update_* and scene_refit_*)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import scenes
from vimg_amd import hip

hip.init(0)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
t0 = time.perf_counter()
s = scenes.config5_scene()
build_s = time.perf_counter() - t0
v0, n0, _ = s.geometry()
view = s.view.contents
rng = np.random.default_rng(0x5EED)
v1 = (v0 + rng.normal(0.0, 0.01, v0.shape)).astype(np.float32)
n1 = n0 + rng.normal(0.0, 0.1, n0.shape)
n1 = (n1 / np.maximum(np.linalg.norm(n1, axis=1, keepdims=True), 1e-6)).astype(np.float32)
dv = [torch.from_numpy(v).cuda() for v in (v0, v1)]
dn = [torch.from_numpy(n).cuda() for n in (n0, n1)]

upload = []
for _ in range(reps + 1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d = hip.DeviceScene(s)
    upload.append(time.perf_counter() - t0)
    d.close()
d = hip.DeviceScene(s)
stream = torch.cuda.current_stream()
wall, dev = [], []
for k in range(2 * reps + 2):          # alternately the original and the displaced positions (the last: displaced); the first two warm up
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(stream)
    t0 = time.perf_counter()
    d.update_geometry(vertices=dv[k % 2], normals=dn[k % 2])
    wall.append(time.perf_counter() - t0)
    b.record(stream)
    b.synchronize()
    dev.append(a.elapsed_time(b))
cam = []
for k in range(reps + 1):
    t0 = time.perf_counter()
    d.set_camera((0.0, 7.0 + 0.1 * k, 13.0), (0.0, 0.5, 0.0), (0, 1, 0), 38.0)
    cam.append(time.perf_counter() - t0)
d.set_camera((0.0, 7.0, 13.0), (0.0, 0.5, 0.0), (0, 1, 0), 38.0)
# the last update left v1 / n1 in place: the fresh upload of the same host scene must render the same bits
s.set_vertices(v1, n1)
s.refit_bvh()
p = s.default_params(samples=1, depth=4)
img, st = d.render_to_host(p)
ref, rst = hip.DeviceScene(s).render_to_host(p)
same = bool(np.array_equal(img.view(np.uint32), ref.view(np.uint32))) and st.as_dict() == rst.as_dict()
print(json.dumps({"scene": "config5", "triangles": int(view.num_tris), "vertices": int(view.num_vertices),
                  "nodes": int(view.bvh.num_nodes), "host_build_s": round(build_s, 1),
                  "update_ms": round(min(wall[2:]) * 1e3, 3), "update_ms_median": round(float(np.median(wall[2:])) * 1e3, 3),
                  "update_device_ms": round(min(dev[2:]), 3), "update_device_ms_median": round(float(np.median(dev[2:])), 3),
                  "set_camera_ms": round(min(cam[1:]) * 1e3, 4), "upload_ms": round(min(upload[1:]) * 1e3, 1),
                  "upload_ms_median": round(float(np.median(upload[1:])) * 1e3, 1), "bit_identical_to_fresh": same}),
      flush=True)
assert same
