"""The clamp of a long history of radiance to a short history beside it, over histories in device memory: ctypes mirror of
include/vimg_rectify.h (libvimg_rectify.so, gfx950).

A frame library beside temporal.py's and antilag.py's: the accumulate calls keep up to max_history
frames of radiance, which goes stale when the light on a surface changes; antilag.rescale cuts the history's length where
a test sees the change, and nothing bounds its colour.  ``clamp`` does: a second history of a few frames - the same
accumulate call with a small max_history, on buffers of its own - is noisy but nearly current, and the long history is
clamped, per pixel and in place, to the mean +- k standard deviations of the short one over a window of the same surface.
The binding shares the render binding's tensor check and stream rule (hip.FrameCall: hip._device_tensor, hip._Launch).
There is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _abi as abi
from .hip import FrameCall, FrameHistory, _checker, library_params

_lib = abi.rectify_lib
_check = _checker(_lib, "vimg_rectify_last_error")

FLOATS = ("k", "cut", "sigma_normal", "sigma_plane", "albedo_floor")
COUNTS = ("radius", "min_taps")


def params(radius=None, min_taps=None, **floats):
    """An abi.RectifyParams: the library's defaults (vimg_rectify_defaults; include/vimg_rectify.h names them) with the
    given values in place of them: ``radius``, ``min_taps``, ``k``, ``cut``, ``sigma_normal``, ``sigma_plane``,
    ``albedo_floor``.  The library checks the ranges; here an integer field only has to fit its uint32."""
    return library_params("rectify", abi.RectifyParams, _lib().vimg_rectify_defaults, FLOATS, list(floats.items()),
                          ("radius", radius, f"1..{abi.RECTIFY_MAX_RADIUS}"), ("min_taps", min_taps, "1..(2 radius + 1)^2"))


def workspace_bytes(width, height):
    return int(_lib().vimg_rectify_workspace(width, height))


workspace = workspace_bytes


def clamp(slow, fast, albedo=None, out=None, code=False, workspace=None, stream=None, **params_kw):
    """Clamps the colour of the history ``slow`` IN PLACE to the statistics of the history ``fast`` of the same picture
    (vimg_rectify_clamp).  Both are hip.FrameHistory - a temporal.History, or a moments.History, whose first three
    planes are read and whose plane M is left as it is; ``albedo`` is the [H, W, 3] float32 albedo frame for
    demodulation, or None.  For every pixel with a slow history, the fast colours of the pixels of its own surface
    within ``radius`` (by slow's guides; the pixel itself included) give a mean and a standard deviation per channel;
    a colour outside mean +- ``k`` deviations is moved to the bound, and the pixel's length then moves by ``cut`` of
    the way to its fast length.  Returns (history, image, code): ``history`` is ``slow`` itself when its tensor is a
    CUDA tensor - only plane A has been written; image [H, W, 3] float32 is the resulting colour of every pixel; code
    [H, W] uint8 is 0 kept, 1 clamped, 2 fewer than ``min_taps`` accepted taps, 3 a miss or no slow history.  ``out``:
    the CUDA tensor to write the image to, allocated when None, False for none (None is then returned for it);
    ``code``: False for none, True for a new tensor, or the CUDA tensor to write.  CUDA tensors are read where they
    are; histories that hold numpy arrays are copied up, the clamped one comes back as a new one of its class, and the
    image and the codes are then numpy arrays.  ``workspace``: not needed (workspace_bytes is 0); a caller's is passed
    on as it is.  ``params_kw``: the parameters of ``params``, which default to the library's
    (include/vimg_rectify.h).  The call only enqueues, on ``stream`` or torch's current stream."""
    for name, hist in (("slow", slow), ("fast", fast)):
        if not isinstance(hist, FrameHistory):
            raise ValueError(f"rectify: {name} must be a temporal.History or a moments.History")
    c = FrameCall("rectify", slow.color)
    h, w = c.h, c.w
    p = params(**params_kw)
    if isinstance(fast.tensor, np.ndarray) != c.to_host:
        raise ValueError("rectify: the two histories must both hold CUDA tensors or both hold numpy arrays")
    s = c.take(slow.tensor, "rectify slow", ("float32",), (type(slow).PLANES, h, w, 4), aligned=True)
    f = c.take(fast.tensor, "rectify fast", ("float32",), (type(fast).PLANES, h, w, 4), aligned=True)
    t = c.frames(("albedo",), (albedo,), optional=("albedo",))
    if out is not False:
        out = c.output(out, "rectify", "float32", (h, w, 3))
    if code is not False:
        code = c.output(None if code is True else code, "rectify code", "uint8", (h, w))
    work = None if workspace is None else c.workspace(workspace, 0)
    frames = abi.RectifyFrames(width=w, height=h, slow=s.data_ptr(), fast=f.data_ptr(), **{k: v.data_ptr() for k, v in t.items()})
    with c.launch(stream) as sp:
        _check(_lib().vimg_rectify_clamp(C.byref(frames), C.byref(p), None if out is False else C.c_void_p(out.data_ptr()),
                                         None if code is False else C.c_void_p(code.data_ptr()),
                                         None if work is None else C.c_void_p(work.data_ptr()),
                                         0 if work is None else work.numel() * work.element_size(), sp))
    return c.rewritten(slow, s), (None if out is False else c.result(out)), (None if code is False else c.result(code))


__all__ = ["clamp", "params", "workspace", "workspace_bytes", "FLOATS", "COUNTS"]
