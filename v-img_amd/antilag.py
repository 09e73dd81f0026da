"""Shortening a reprojected history where the picture has changed, over frames in device memory: ctypes mirror of
include/vimg_antilag.h (libvimg_antilag.so, gfx950).

A frame library beside temporal.py's: the accumulate calls blend a history with the current frame
wherever the surface is the same, whatever has happened to the light on it.  ``rescale`` compares the two, window by
window, by a paired t-test of their luminances and multiplies the history's lengths - nothing else - by a scale in
[0, 1]; temporal.accumulate, moments.accumulate and wtemporal.accumulate then run on that history as they are.  The
binding shares the render binding's tensor check and stream rule (hip.FrameCall: hip._device_tensor, hip._Launch).
There is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _abi as abi
from .hip import FrameCall, FrameHistory, _checker, library_params
from .temporal import FRAMES

FLOATS = ("t_low", "t_high", "min_matches", "sigma_normal", "sigma_plane")

_lib = abi.antilag_lib
_check = _checker(_lib, "vimg_antilag_last_error")


def antilag_params(radius=None, t_low=None, t_high=None, min_matches=None, sigma_normal=None, sigma_plane=None):
    """An abi.AntilagParams: the library's defaults (vimg_antilag_defaults; include/vimg_antilag.h names them) with the
    given values in place of them."""
    return _params(radius, zip(FLOATS, (t_low, t_high, min_matches, sigma_normal, sigma_plane)))


def _params(radius, given):
    return library_params("antilag", abi.AntilagParams, _lib().vimg_antilag_defaults, FLOATS, given,
                          ("radius", radius, f"1..{abi.ANTILAG_MAX_RADIUS}"))


def workspace_bytes(width, height):
    return int(_lib().vimg_antilag_workspace_bytes(width, height))


def rescale(color, normal, position, depth, history, world_to_pixel, out_scale=None, workspace=None, stream=None, **params):
    """Rescales the lengths of ``history`` in place by how well it agrees with the current picture
    (vimg_antilag_rescale).  ``color`` and the first-hit frames ``normal``, ``position``, ``depth`` are the CURRENT
    [H, W, 3] float32 frames and ``world_to_pixel`` the 12 floats of the CURRENT camera's matrix
    (temporal.world_to_pixel(camera)); ``history`` is any hip.FrameHistory - a temporal.History or a moments.History,
    whose plane M is left as it is.  Every history pixel is projected into the current picture; where it lands on the
    same surface the luminances of the two make a pair, and over the (2 radius + 1)^2 window around the history pixel
    the mean of the pairs' differences is measured in its standard errors: below t_low the length stays, from t_high
    on it becomes 0, between them it is scaled linearly in t^2.  Returns (history, scale): ``history`` itself when its
    tensor is a CUDA tensor - only plane A's fourth component has been written - and scale [H, W] float32, 1 for a
    pixel without history.  CUDA tensors are read where they are; numpy arrays are copied up, a history that holds a
    numpy array comes back as a new one of its class, and with a numpy ``color`` the scale is a numpy array.
    ``out_scale``: the [H, W] float32 CUDA tensor to write, or False for none (None is then returned for it);
    ``workspace``: a contiguous, 16-byte aligned CUDA tensor of at least workspace_bytes(W, H) bytes (8 per pixel),
    allocated here when None.  ``params``: radius, t_low, t_high, min_matches, sigma_normal, sigma_plane, default the
    library's (include/vimg_antilag.h).  The call only enqueues, on ``stream`` or torch's current stream."""
    c = FrameCall("antilag", color)
    h, w = c.h, c.w
    p = _params(params.pop("radius", None), params.items())
    t = c.frames(FRAMES, (color, normal, position, depth))
    if not isinstance(history, FrameHistory):
        raise ValueError("antilag: history must be a temporal.History or a moments.History")
    matrix = np.ascontiguousarray(world_to_pixel, dtype=np.float32)
    if matrix.size != 12:
        raise ValueError(f"antilag: world_to_pixel must have 12 entries, not {matrix.size}")
    if isinstance(history.tensor, np.ndarray) and not c.to_host:
        raise ValueError("antilag: a history that holds a numpy array goes with numpy frames; with CUDA frames it is rescaled "
                         "in place and must hold a CUDA tensor")
    hist = c.take(history.tensor, "antilag history", ("float32",), (type(history).PLANES, h, w, 4), aligned=True)
    if out_scale is not False:
        out_scale = c.output(out_scale, "antilag out_scale", "float32", (h, w))
    workspace = c.workspace(workspace, workspace_bytes(w, h))
    frames = abi.AntilagFrames(width=w, height=h, **{k: v.data_ptr() for k, v in t.items()})
    with c.launch(stream) as sp:
        _check(_lib().vimg_antilag_rescale(C.byref(frames), (abi.f32 * 12)(*matrix.reshape(12).tolist()), C.c_void_p(hist.data_ptr()),
                                           C.byref(p), C.c_void_p(workspace.data_ptr()),
                                           workspace.numel() * workspace.element_size(),
                                           None if out_scale is False else C.c_void_p(out_scale.data_ptr()), sp))
    return c.rewritten(history, hist), (None if out_scale is False else c.result(out_scale))


__all__ = ["rescale", "antilag_params", "workspace_bytes", "FLOATS", "FRAMES"]
