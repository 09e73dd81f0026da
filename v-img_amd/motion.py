"""Previous-world positions of moved geometry, over frames and tables in device memory: ctypes mirror of
include/vimg_motion.h (libvimg_motion.so, gfx950).

A frame library beside temporal.py's: the accumulate calls look a pixel up in the history where the
last camera saw the pixel's current world position, which is right only while the world stands still.
``previous_position`` writes, per pixel, where the surface point the pixel shows was before
DeviceScene.update_geometry moved it - the position frame plus the displacement of the pixel-centre hit - and
temporal.accumulate, moments.accumulate and wtemporal.accumulate run on that frame as they are.  The binding shares the
render binding's tensor check and stream rule (hip.FrameCall: hip._device_tensor, hip._Launch).  There is no CPU
fallback.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _abi as abi
from .hip import FrameCall, _checker
from .host import HostScene

_lib = abi.motion_lib
_check = _checker(_lib, "vimg_motion_last_error")

# the two position tables of a scene at one moment: ``vertices`` [num_vertices, 3], ``spheres`` [num_spheres, 4] (centre,
# radius), float32 CUDA tensors or numpy arrays; None = not given.  What previous_position takes as ``old`` and ``new``.
Positions = namedtuple("Positions", ("vertices", "spheres"), defaults=(None, None))


def tri_vertex_rows(host_scene):
    """[num_tris, 3] uint32: the GLOBAL vertex rows of every triangle of ``host_scene``,
    meshes[tri_mesh[t]].first_vertex + tri_indices[3 t + k] (include/vimg_motion.h's tri_vertices)."""
    v = host_scene.view.contents
    nt = int(v.num_tris)
    if nt == 0:
        return np.zeros((0, 3), np.uint32)
    first = np.array([v.meshes[m].first_vertex for m in range(v.num_meshes)], dtype=np.uint32)
    local = np.ctypeslib.as_array(v.tri_indices, (nt, 3))
    mesh = np.ctypeslib.as_array(v.tri_mesh, (nt,))
    return (local + first[mesh][:, None]).astype(np.uint32)


def prim_records(host_scene):
    """[num_prims, 2] uint32: the VimgPrim records {type, index} of ``host_scene``."""
    v = host_scene.view.contents
    n = int(v.num_prims)
    if n == 0:
        return np.zeros((0, 2), np.uint32)
    return np.ctypeslib.as_array(C.cast(v.prims, C.POINTER(abi.u32)), (n, 2)).copy()


class SceneTables:
    """What previous_position reads of a scene beside the positions: ``prims`` [num_prims, 2] and ``tri_vertices``
    [num_tris, 3] (int32 CUDA tensors that hold the uint32 bits), the four counts, and ``positions``, the Positions the
    scene had when the tables were read (CUDA tensors)."""

    def __init__(self, prims, tri_vertices, num_vertices, num_spheres, positions=Positions()):
        self.prims, self.tri_vertices = prims, tri_vertices
        self.num_prims, self.num_tris = int(prims.shape[0]), int(tri_vertices.shape[0])
        self.num_vertices, self.num_spheres = int(num_vertices), int(num_spheres)
        self.positions = positions

    @classmethod
    def from_host(cls, host_scene):
        """Device copies of the tables of ``host_scene`` (a HostScene), read once: later edits of it are not seen."""
        import torch
        if not isinstance(host_scene, HostScene):
            raise ValueError(f"motion: expected a HostScene, not {type(host_scene).__name__}")
        verts, _, spheres = host_scene.geometry()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
        return cls(up(prim_records(host_scene).view(np.int32)), up(tri_vertex_rows(host_scene).view(np.int32)), verts.shape[0],
                   spheres.shape[0], Positions(up(verts), up(spheres)))


def centre_samples(height, width):
    """The [H * W, 4] float32 samples {x, y, lens_u, lens_v} of the pixel centres for DeviceScene.camera_rays, in FRAME
    ARRAY order: array row r is the renderer's sample row y = H - 1 - r + 0.5 (vimg_hip_render stores sample row y at
    array row H - 1 - y), column c is x = c + 0.5.  The lens sample is (0, 0), which sample_disk maps to the lens
    centre: a thin lens is treated as its pinhole, as temporal.world_to_pixel treats it."""
    h, w = int(height), int(width)
    s = np.zeros((h, w, 4), np.float32)
    s[..., 0] = np.arange(w, dtype=np.float32)[None, :] + np.float32(0.5)
    s[..., 1] = (np.float32(h - 1) - np.arange(h, dtype=np.float32))[:, None] + np.float32(0.5)
    return s.reshape(h * w, 4)


def previous_position(position, hits, rays, tables, old, new, out=None, out_code=None, stream=None):
    """Where the surface point each pixel shows was under the ``old`` positions (vimg_motion_previous_position).
    ``position``: the current [H, W, 3] float32 position frame; ``hits``: [H * W, 4] float32, the VimgRayHit records
    DeviceScene.trace_rays writes for ``rays``, [H * W, 8] float32, the pixel-centre rays
    (camera_rays(centre_samples(H, W))) - ``rays`` may be None for a scene without spheres; ``tables``: the scene's
    SceneTables; ``old``, ``new``: Positions (or (vertices, spheres) pairs) - a table that is None in either did not
    move, and a table given in one must be given in the other.  Returns (previous, code): previous [H, W, 3] float32,
    the position frame's bits wherever the displacement is exactly zero, and code [H, W] uint8 - 0 a miss or no
    displacement, 1 a moved triangle, 2 a moved sphere, 3 an index out of range (the pixel keeps its position).  CUDA
    tensors are read where they are; numpy arrays are copied up, and with a numpy ``position`` both results are numpy
    arrays.  ``out``: the [H, W, 3] float32 CUDA tensor to write; ``out_code``: the [H, W] uint8 CUDA tensor to write, or
    False for none (None is then returned for it).  The call only enqueues, on ``stream`` or torch's current stream."""
    c = FrameCall("motion", position)
    h, w = c.h, c.w
    pos = c.take(position, "motion position", ("float32",), (h, w, 3))
    hit = c.take(hits, "motion hits", ("float32",), (h * w, 4), aligned=True)
    ray = None if rays is None else c.take(rays, "motion rays", ("float32",), (h * w, 8), aligned=True)
    if not isinstance(tables, SceneTables):
        raise ValueError("motion: tables must be a motion.SceneTables")
    if ray is None and tables.num_spheres:
        raise ValueError(f"motion: rays may be None only for a scene without spheres, this one has {tables.num_spheres}")
    old, new = Positions(*old), Positions(*new)
    given = {}
    for name, rows, cols, aligned in (("vertices", tables.num_vertices, 3, False), ("spheres", tables.num_spheres, 4, True)):
        o, n = getattr(old, name), getattr(new, name)
        if (o is None) != (n is None):
            raise ValueError(f"motion: {name} must be given in both old and new, or in neither")
        if o is not None and rows:
            given[name] = (c.take(o, f"motion old {name}", ("float32",), (rows, cols), aligned),
                           c.take(n, f"motion new {name}", ("float32",), (rows, cols), aligned))
    c.use(tables.prims)
    c.use(tables.tri_vertices)
    out = c.output(out, "motion", "float32", (h, w, 3))
    if out_code is not False:
        out_code = c.output(out_code, "motion out_code", "uint8", (h, w))
    frames = abi.MotionFrames(width=w, height=h, position=pos.data_ptr(), hits=hit.data_ptr(), rays=None if ray is None else ray.data_ptr())
    pair = lambda name, k: given[name][k].data_ptr() if name in given else None
    table = lambda t: t.data_ptr() if t.numel() else None
    geometry = abi.MotionGeometry(num_prims=tables.num_prims, num_tris=tables.num_tris, num_vertices=tables.num_vertices,
                                  num_spheres=tables.num_spheres, prims=table(tables.prims), tri_vertices=table(tables.tri_vertices),
                                  old_vertices=pair("vertices", 0), new_vertices=pair("vertices", 1),
                                  old_spheres=pair("spheres", 0), new_spheres=pair("spheres", 1))
    with c.launch(stream) as sp:
        _check(_lib().vimg_motion_previous_position(C.byref(frames), C.byref(geometry), C.c_void_p(out.data_ptr()),
                                                    None if out_code is False else C.c_void_p(out_code.data_ptr()), sp))
    return c.result(out), (None if out_code is False else c.result(out_code))


__all__ = ["previous_position", "centre_samples", "SceneTables", "Positions", "tri_vertex_rows", "prim_records"]
