"""The clamp of fireflies in a frame in device memory, before it is filtered: ctypes mirror of include/vimg_despeckle.h
(libvimg_despeckle.so, gfx950).

A frame library beside filter.py's: a frame of 1 - 16 samples per pixel carries single pixels many times
brighter than their surface, which the a-trous filters spread into blotches and the temporal accumulation then carries;
``clamp`` scales such a pixel down to a bound taken from the pixels of its own surface around it, by the first-hit
feature frames.  The binding shares the render binding's tensor check and stream rule (hip.FrameCall:
hip._device_tensor, hip._Launch).  There is no CPU fallback.
"""
import ctypes as C

from . import _abi as abi
from .filter import FRAMES, GUIDES
from .hip import FrameCall, _checker, library_params

_lib = abi.despeckle_lib
_check = _checker(_lib, "vimg_despeckle_last_error")

FLOATS = ("gain", "sigma_normal", "sigma_plane", "albedo_floor")
COUNTS = ("radius", "rank", "min_taps")


def params(radius=None, rank=None, min_taps=None, **floats):
    """An abi.DespeckleParams: the library's defaults (vimg_despeckle_defaults; include/vimg_despeckle.h names them) with
    the given values in place of them: ``radius``, ``rank``, ``min_taps``, ``gain``, ``sigma_normal``, ``sigma_plane``,
    ``albedo_floor``.  The library checks the ranges; here an integer field only has to fit its uint32."""
    return library_params("despeckle", abi.DespeckleParams, _lib().vimg_despeckle_defaults, FLOATS, list(floats.items()),
                          ("radius", radius, f"1..{abi.DESPECKLE_MAX_RADIUS}"), ("rank", rank, f"1..{abi.DESPECKLE_MAX_RANK}"),
                          ("min_taps", min_taps, "rank..(2 radius + 1)^2 - 1"))


def workspace_bytes(width, height):
    return int(_lib().vimg_despeckle_workspace(width, height))


def clamp(color, normal, position, depth, albedo=None, out=None, out_code=None, workspace=None, stream=None, **params_kw):
    """Scales the fireflies of ``color`` down (vimg_despeckle_clamp).  ``color`` and the first-hit feature frames
    ``normal``, ``position``, ``depth`` and, for demodulation, ``albedo`` are [H, W, 3] float32.  A live pixel whose
    (demodulated) luminance is above ``gain`` times the larger of the mean and the ``rank``-th largest luminance of the
    pixels of its own surface within ``radius`` is scaled to that bound; every other pixel is copied, bit for bit.
    Returns (image [H, W, 3] float32, code [H, W] uint8: 0 kept, 1 clamped, 2 fewer than ``min_taps`` pixels of its
    surface around it, 3 not live); ``out_code=False``: no codes are written and None is returned for them.  CUDA
    tensors are read where they are and the results are CUDA tensors; numpy arrays are copied up, and with a numpy
    ``color`` numpy arrays come back.  ``params_kw``: the parameters of ``params``, which default to the library's
    (include/vimg_despeckle.h).  ``out`` may be ``color`` itself; ``workspace``: a contiguous, 16-byte aligned CUDA
    tensor of at least workspace_bytes(W, H) bytes (32 per pixel), allocated here when None.  The call only enqueues, on
    ``stream`` or torch's current stream."""
    c = FrameCall("despeckle", color)
    h, w = c.h, c.w
    p = params(**params_kw)
    t = c.frames(FRAMES, (color, normal, position, depth, albedo), optional=("albedo",))
    out = c.output(out, "despeckle", "float32", (h, w, 3))
    out_code = None if out_code is False else c.output(out_code, "despeckle out_code", "uint8", (h, w))
    workspace = c.workspace(workspace, workspace_bytes(w, h))
    frames = abi.DespeckleFrames(width=w, height=h, **{k: v.data_ptr() for k, v in t.items()})
    with c.launch(stream) as sp:
        _check(_lib().vimg_despeckle_clamp(C.byref(frames), C.byref(p), C.c_void_p(out.data_ptr()),
                                           None if out_code is None else C.c_void_p(out_code.data_ptr()),
                                           C.c_void_p(workspace.data_ptr()), workspace.numel() * workspace.element_size(), sp))
    return c.result(out), None if out_code is None else c.result(out_code)


__all__ = ["clamp", "params", "workspace_bytes", "GUIDES"]
