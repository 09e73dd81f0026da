"""Temporal accumulation over frames in device memory: ctypes mirror of include/vimg_temporal.h
(libvimg_temporal.so, gfx950).

The third scene-free library: the last preview is reprojected into a moved camera by the `position`
frame and blended with the current frame where normal and position say it is the same surface.  The binding shares the
render binding's tensor check and stream rule (hip.FrameCall: hip._device_tensor, hip._Launch).  There is no CPU
fallback.
"""
import ctypes as C
import math

import numpy as np

from . import _abi as abi
from .hip import FrameCall, FrameHistory, _checker, library_params

FRAMES = ("color", "normal", "position", "depth")
PARAMS = ("max_history", "current_weight", "sigma_normal", "sigma_plane")


_lib = abi.temporal_lib
_check = _checker(_lib, "vimg_temporal_last_error")


def temporal_params(max_history=None, current_weight=None, sigma_normal=None, sigma_plane=None):
    """An abi.TemporalParams: the library's defaults (vimg_temporal_defaults; include/vimg_temporal.h names them) with
    the given values in place of them."""
    return _params(zip(PARAMS, (max_history, current_weight, sigma_normal, sigma_plane)))


def _params(given):
    return library_params("temporal", abi.TemporalParams, _lib().vimg_temporal_defaults, PARAMS, given)


def history_bytes(width, height):
    return int(_lib().vimg_temporal_history_bytes(width, height))


def world_to_pixel(camera):
    """The 12 float32 of vimg_temporal_accumulate's matrix (row-major 3 x 4) for an abi.Camera: a world-space point
    goes to (hx, hy, hw) with column hx / hw and row hy / hw in FRAME ARRAY coordinates - column = the renderer's
    sample x, row = res_y - sample y, because vimg_hip_render stores sample row y at array row H - 1 - y.  The pinhole
    through the lens centre (with aperture_radius > 0 this is the mapping of the lens centre), the inverse of the
    rigid cam_to_world, the image plane of the reference's TLCam (height 2 tan(vfov / 2), width ratio times that, rays
    along -z).  Computed in float64 and rounded once."""
    c2w = np.array(list(camera.cam_to_world), dtype=np.float64).reshape(4, 4).T      # glm column-major
    rot, org = c2w[:3, :3], c2w[:3, 3]
    w2c = np.concatenate([rot.T, -(rot.T @ org)[:, None]], axis=1)                    # camera-space point = w2c [P; 1]
    w, h = float(camera.res_x), float(camera.res_y)
    ph = 2.0 * math.tan(math.radians(float(camera.vfov_deg)) / 2.0)
    pw = (w / h) * ph
    m = np.stack([(w / pw) * w2c[0] - (w / 2.0) * w2c[2],        # sample x = w (x_dir / pw + 1/2),  x_dir = Pc.x / -Pc.z
                  -(h / ph) * w2c[1] - (h / 2.0) * w2c[2],       # row = h - sample y = h (1/2 - y_dir / ph)
                  -w2c[2]])
    return m.astype(np.float32).reshape(12)


class History(FrameHistory):
    """One history of vimg_temporal_accumulate: ``tensor`` [3, H, W, 4] float32 (planes A = {rgb, length},
    G0 = {normal, depth}, G1 = {position, 0}; a CUDA tensor, or a numpy array after a call with numpy frames) and
    ``world_to_pixel``, the matrix of the camera its frame was rendered under (None: unknown, the history cannot be
    reprojected).  ``color`` [H, W, 3] and ``length`` [H, W] are views."""
    PLANES = 3


def accumulate(color, normal, position, depth, history=None, world_to_pixel=None, out=None, next_history=None, stream=None,
               **params):
    """One step of temporal accumulation (vimg_temporal_accumulate): the current ``color`` frame with its first-hit
    frames ``normal``, ``position``, ``depth`` - all [H, W, 3] float32, as DeviceScene.render and render_features
    return them - blended with ``history``, the History of the frame before (None: no history), which is looked up
    where ``history.world_to_pixel`` sends each pixel's position.  Returns the next History; ``world_to_pixel`` is the
    matrix of the CURRENT camera (temporal.world_to_pixel(camera)), which the result remembers for the next step.
    CUDA tensors are read where they are; numpy arrays are copied up, and with a numpy ``color`` the History holds a
    numpy array.  ``out``: a [H, W, 3] float32 CUDA tensor that gets the accumulated colour as packed triples, which
    may be ``color`` itself; ``next_history``: the [3, H, W, 4] float32 CUDA tensor to write (not the one ``history``
    holds), allocated when None.  ``params``: max_history, current_weight, sigma_normal, sigma_plane, default the
    library's (include/vimg_temporal.h).  The call only enqueues, on ``stream`` or torch's current stream."""
    c = FrameCall("temporal", color)
    h, w = c.h, c.w
    p = _params(params.items())
    t = c.frames(FRAMES, (color, normal, position, depth))
    prev, matrix = c.history(history, History)
    next_history = c.output(next_history, "temporal next_history", "float32", (3, h, w, 4), aligned=True)
    if out is not None:
        c.output(out, "temporal", "float32", (h, w, 3))
    frames = abi.TemporalFrames(width=w, height=h, **{k: v.data_ptr() for k, v in t.items()})
    with c.launch(stream) as sp:
        _check(_lib().vimg_temporal_accumulate(C.byref(frames), None if prev is None else C.c_void_p(prev.data_ptr()), matrix,
                                               C.byref(p), C.c_void_p(next_history.data_ptr()),
                                               None if out is None else C.c_void_p(out.data_ptr()), sp))
    return History(c.result(next_history), world_to_pixel)


def __getattr__(name):
    """TemporalPreview is composed in vimg_amd.preview, which imports this module; it still resolves here."""
    if name == "TemporalPreview":
        from .preview import TemporalPreview
        return TemporalPreview
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["accumulate", "temporal_params", "history_bytes", "world_to_pixel", "History", "TemporalPreview", "FRAMES"]
