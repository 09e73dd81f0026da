"""Filters over frames in device memory: ctypes mirror of include/vimg_filter.h (libvimg_filter.so, gfx950).

A library of its own beside the render library: a filter reads frames, never a scene.  The
binding shares the render binding's tensor check and stream rule (hip.FrameCall: hip._device_tensor, hip._Launch),
so a filter call is ordered against torch exactly as a render is.  There is no CPU fallback.
"""
import ctypes as C

from . import _abi as abi
from .hip import FrameCall, _checker, library_params

FRAMES = ("color", "normal", "position", "depth", "albedo")
GUIDES = ("albedo", "normal", "position", "depth")     # the feature frames the filter reads beside the colour
FLOATS = ("sigma_color", "sigma_normal", "sigma_plane", "albedo_floor")


_lib = abi.filter_lib
_check = _checker(_lib, "vimg_filter_last_error")


def atrous_params(iterations=None, sigma_color=None, sigma_normal=None, sigma_plane=None, albedo_floor=None):
    """An abi.AtrousParams: the library's defaults (vimg_filter_atrous_defaults; include/vimg_filter.h names them) with
    the given values in place of them."""
    return library_params("atrous", abi.AtrousParams, _lib().vimg_filter_atrous_defaults, FLOATS,
                          zip(FLOATS, (sigma_color, sigma_normal, sigma_plane, albedo_floor)), ("iterations", iterations, "1..12"))


def atrous_workspace_bytes(width, height):
    return int(_lib().vimg_filter_atrous_workspace(width, height))


def atrous(color, normal, position, depth, albedo=None, iterations=None, sigma_color=None, sigma_normal=None,
           sigma_plane=None, albedo_floor=None, out=None, workspace=None, stream=None):
    """The edge-avoiding a-trous filter (vimg_filter_atrous) of a noisy ``color`` frame guided by the first-hit
    feature frames ``normal``, ``position``, ``depth`` and, for demodulation, ``albedo`` - all [H, W, 3] float32,
    as DeviceScene.render and render_features return them.  CUDA tensors are read where they are and the result is
    a CUDA tensor; numpy arrays are copied up, and with a numpy ``color`` a numpy array comes back.  The parameters
    default to the library's (include/vimg_filter.h).  ``out``: the [H, W, 3] float32 CUDA tensor to write, which
    may be ``color`` itself; ``workspace``: a contiguous, 16-byte aligned CUDA tensor of at least
    atrous_workspace_bytes(W, H) bytes (64 per pixel), allocated here when None.  The call only enqueues, on
    ``stream`` or torch's current stream."""
    c = FrameCall("atrous", color)
    h, w = c.h, c.w
    params = atrous_params(iterations, sigma_color, sigma_normal, sigma_plane, albedo_floor)
    t = c.frames(FRAMES, (color, normal, position, depth, albedo), optional=("albedo",))
    out = c.output(out, "atrous", "float32", (h, w, 3))
    workspace = c.workspace(workspace, atrous_workspace_bytes(w, h))
    frames = abi.FilterFrames(width=w, height=h, **{k: v.data_ptr() for k, v in t.items()})
    with c.launch(stream) as sp:
        _check(_lib().vimg_filter_atrous(C.byref(frames), C.byref(params), C.c_void_p(out.data_ptr()),
                                         C.c_void_p(workspace.data_ptr()), workspace.numel() * workspace.element_size(), sp))
    return c.result(out)


__all__ = ["atrous", "atrous_params", "atrous_workspace_bytes", "GUIDES"]
