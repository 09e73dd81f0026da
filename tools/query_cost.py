#!/usr/bin/env python3
"""Rate of the ray queries: Mrays/s of closest hit, closest hit + record, and occlusion, on
  config2        disney_spheres at 1800 x 800 (its tree sits in the queries' LDS)
  config5        the config 5 stand-in (519 200 triangles; the tree is read from global memory below its top)
  caterpillar    a caller-built tree 43 levels deep (test_ray_query.py: big_mesh_scene(n=4), 43 primitives), stacks
                 of 45 entries and no node in LDS
(the JSON line reports each scene's nodes, depth and primitives)
with two ray sets:
  coherent       camera rays of the frame, one jittered sample per pixel, cycled over the pixels up to N
  incoherent     an AO batch: from the coherent rays' hit points, cosine-distributed directions about the geometric
                 normal, t_max = the scene's diagonal
at N = 2^20 and 2^24.  Each row runs under both launch shapes, interleaved: the persistent grid
(VIMG_HIP_QUERY_BLOCKS=1) and one workgroup per 256 rays (=0), each read at upload by a DeviceScene of its own; the
library's policy picks one of them per scene (ray_query.hip:launch_query).  Times are device events
around back-to-back calls of the C ABI (max(2, 2^25 / N) of them) on a non-default stream, per call, best of `reps`
after a warm-up.  Prints a table to stderr and one JSON line.
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats` (kernels ray_query_kernel<0|1|2>)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes as C
import numpy as np
import torch
import scenes
from vimg_amd import hip

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
sizes = [int(a) for a in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1 << 20, 1 << 24]
hip.init(0)
lib = hip._lib()


def caterpillar():
    from test_ray_query import caterpillar_builder
    s = scenes.big_mesh_scene(res=(1280, 800), n=4)
    cb = caterpillar_builder()
    s.build_bvh_with(C.cast(cb, C.c_void_p))
    return s


def diagonal(s):
    v, _, sp = s.geometry()
    pts = [v] if len(v) else []
    if len(sp):
        pts += [sp[:, :3] - sp[:, 3:4], sp[:, :3] + sp[:, 3:4]]
    p = np.concatenate(pts)
    return float(np.linalg.norm(p.max(0) - p.min(0)))


def coherent(dev, s, n, gen):
    w, h = s.resolution
    idx = torch.arange(n, device="cuda") % (w * h)
    smp = torch.stack([(idx % w).float() + torch.rand(n, device="cuda", generator=gen),
                       (idx // w).float() + torch.rand(n, device="cuda", generator=gen),
                       torch.rand(n, device="cuda", generator=gen), torch.rand(n, device="cuda", generator=gen)], 1)
    return dev.camera_rays(smp.contiguous())


def ambient_occlusion(dev, rays, diag, gen):
    r = dev.trace_rays(rays, info=True)
    hit = r.prim >= 0
    p, ng, d = r.p[hit], r.ng[hit], rays[hit][:, 4:7]
    n = torch.where(((ng * d).sum(1, keepdim=True) > 0), -ng, ng)
    a = torch.where(n[:, 0:1].abs() > 0.9, torch.tensor([0.0, 1.0, 0.0], device="cuda"),
                    torch.tensor([1.0, 0.0, 0.0], device="cuda"))
    t = torch.nn.functional.normalize(torch.cross(a.expand_as(n), n, dim=1), dim=1)
    b = torch.cross(n, t, dim=1)
    m = p.shape[0]
    u1, u2 = torch.rand(m, device="cuda", generator=gen), torch.rand(m, device="cuda", generator=gen)
    phi, rad = 2 * np.pi * u1, torch.sqrt(u2)
    dirs = t * (rad * torch.cos(phi))[:, None] + b * (rad * torch.sin(phi))[:, None] + n * torch.sqrt(1 - u2)[:, None]
    out = torch.empty((m, 8), device="cuda")
    out[:, 0:3] = p + n * (1e-4 * diag)
    out[:, 3] = 1e-4
    out[:, 4:7] = dirs
    out[:, 7] = diag
    reps_needed = (rays.shape[0] + m - 1) // max(m, 1)
    return out.repeat(reps_needed, 1)[:rays.shape[0]].contiguous()


def timed(fn, st, k):
    """ms per call of k back-to-back calls between two events (the host's cost of a call overlaps the kernels)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(k):
        fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b) / k


SCENES = {"config2": lambda: scenes.json_scene("disney_spheres.json"), "config5": scenes.config5_scene,
          "caterpillar": caterpillar}
rows = []
st = torch.cuda.Stream()
for name, make in SCENES.items():
    s = make()
    diag = diagonal(s)
    os.environ["VIMG_HIP_QUERY_BLOCKS"] = "1"
    persistent = hip.DeviceScene(s)
    os.environ["VIMG_HIP_QUERY_BLOCKS"] = "0"
    blocks = hip.DeviceScene(s)
    del os.environ["VIMG_HIP_QUERY_BLOCKS"]
    view = s.view.contents
    with torch.cuda.stream(st):
        for n in sizes:
            gen = torch.Generator(device="cuda")
            gen.manual_seed(n)
            sets = {"coherent": coherent(persistent, s, n, gen)}
            sets["incoherent"] = ambient_occlusion(persistent, sets["coherent"], diag, gen)
            hits = torch.empty((n, 4), device="cuda")
            info = torch.empty((n, 12), device="cuda")
            flags = torch.empty(n, dtype=torch.uint8, device="cuda")
            for set_name, rays in sets.items():
                for q in ("closest", "closest_info", "occluded"):
                    # the C ABI itself (what a host program calls), not the Python layer's checks and views
                    calls = {}
                    sp, rp = C.c_void_p(st.cuda_stream), C.c_void_p(rays.data_ptr())
                    hp, ip, fp = C.c_void_p(hits.data_ptr()), C.c_void_p(info.data_ptr()), C.c_void_p(flags.data_ptr())
                    for launch, dev in (("persistent", persistent), ("blocks", blocks)):
                        if q == "closest":
                            calls[launch] = lambda h=dev._h: lib.vimg_hip_trace_rays(h, rp, n, hp, None, sp)
                        elif q == "closest_info":
                            calls[launch] = lambda h=dev._h: lib.vimg_hip_trace_rays(h, rp, n, hp, ip, sp)
                        else:
                            calls[launch] = lambda h=dev._h: lib.vimg_hip_occluded(h, rp, n, fp, sp)
                        assert calls[launch]() == 0, hip._lib().vimg_hip_last_error()
                    k = max(2, (1 << 25) // n)
                    ms = {k_: [] for k_ in calls}
                    for r in range(reps + 1):
                        for launch, fn in calls.items():
                            t = timed(fn, st, k)
                            if r:
                                ms[launch].append(t)
                    row = {"scene": name, "rays": set_name, "n": n, "query": q,
                           "hit_fraction": round(float((persistent.trace_rays(rays[:65536]).prim >= 0).float().mean()), 3)}
                    for launch in calls:
                        best = min(ms[launch])
                        row[f"{launch}_ms"] = round(best, 3)
                        row[f"{launch}_mrays_s"] = round(n / best / 1e3, 1)
                    row["speedup"] = round(row["blocks_ms"] / row["persistent_ms"], 3)
                    rows.append(row)
                    print(f"{name:12s} {set_name:10s} {n:9d} {q:13s} persistent {row['persistent_mrays_s']:8.1f}  "
                          f"blocks {row['blocks_mrays_s']:8.1f} Mrays/s  x{row['speedup']:.3f}", file=sys.stderr, flush=True)
    info_row = {"nodes": int(view.bvh.num_nodes), "max_depth": int(view.bvh.max_depth), "prims": int(view.num_prims)}
    for r in rows:
        if r["scene"] == name:
            r.update(info_row)
    persistent.close()
    blocks.close()
print(json.dumps({"tool": "query_cost", "reps": reps, "rows": rows}), flush=True)
