"""Temporal accumulation with luminance moments over frames in device memory: ctypes mirror of
include/vimg_moments.h (libvimg_moments.so, gfx950).

A frame library beside temporal.py's: the same reprojection and blend, bit for bit, and beside the
colour the first two moments of luminance, from which each pixel gets the variance of its accumulated mean - what
vimg_amd.varfilter.atrous takes as ``variance`` - while the camera moves.  The binding shares the render binding's
tensor check and stream rule (hip.FrameCall: hip._device_tensor, hip._Launch).  There is no CPU fallback.
"""
import ctypes as C

from . import _abi as abi
from . import temporal
from .hip import FrameCall, FrameHistory, _checker, library_params
from .temporal import FRAMES, world_to_pixel

PARAMS = ("max_history", "current_weight", "sigma_normal", "sigma_plane", "min_history")

_lib = abi.moments_lib
_check = _checker(_lib, "vimg_moments_last_error")


def params(max_history=None, current_weight=None, sigma_normal=None, sigma_plane=None, min_history=None):
    """An abi.MomentsParams: the library's defaults (vimg_moments_defaults; include/vimg_moments.h names them) with
    the given values in place of them."""
    return _params(zip(PARAMS, (max_history, current_weight, sigma_normal, sigma_plane, min_history)))


def _params(given):
    return library_params("moments", abi.MomentsParams, _lib().vimg_moments_defaults, PARAMS, given)


def history_bytes(width, height):
    return int(_lib().vimg_moments_history_bytes(width, height))


class History(FrameHistory):
    """One history of vimg_moments_accumulate: ``tensor`` [4, H, W, 4] float32 (planes A = {rgb, length},
    G0 = {normal, depth}, G1 = {position, 0}, M = {m1, m2, V, 0}; a CUDA tensor, or a numpy array after a call with
    numpy frames) and ``world_to_pixel``, the matrix of the camera its frame was rendered under (None: unknown, the
    history cannot be reprojected).  ``color`` [H, W, 3], ``length`` [H, W], ``moments`` [H, W, 2] and ``variance``
    [H, W] (NaN: unknown) are views; ``temporal`` is a temporal.History over planes 0..2, a view too, with the same
    matrix."""
    PLANES = 4

    @property
    def moments(self):
        return self.tensor[3, :, :, :2]

    @property
    def variance(self):
        return self.tensor[3, :, :, 2]

    @property
    def temporal(self):
        return temporal.History(self.tensor[:3], self.world_to_pixel)


def accumulate(color, normal, position, depth, variance=None, history=None, world_to_pixel=None, out=None, out_variance=None,
               next_history=None, stream=None, **params_kw):
    """One step of temporal accumulation with moments (vimg_moments_accumulate): temporal.accumulate's arguments and
    result - the same colour and history length, bit for bit - and beside them ``variance``, the [H, W] float32
    variance of the mean luminance of ``color`` (Progressive.variance; NaN = unknown; None: no pixel's is known), and
    ``out_variance``, a [H, W] float32 CUDA tensor that gets the variance of the ACCUMULATED colour's luminance (NaN
    where the history is shorter than min_history, which varfilter.atrous then estimates) and may be ``variance``
    itself.  Returns the next moments.History; ``next_history``: the [4, H, W, 4] float32 CUDA tensor to write (not the
    one ``history`` holds), allocated when None.  CUDA tensors are read where they are; numpy arrays are copied up, and
    with a numpy ``color`` the History holds a numpy array.  ``params_kw``: max_history, current_weight, sigma_normal,
    sigma_plane, min_history, default the library's (include/vimg_moments.h).  The call only enqueues, on ``stream`` or
    torch's current stream."""
    c = FrameCall("moments", color)
    h, w = c.h, c.w
    p = _params(params_kw.items())
    t = c.frames(FRAMES, (color, normal, position, depth))
    if variance is not None:
        t["variance"] = c.take(variance, "moments variance", ("float32",), (h, w))
    prev, matrix = c.history(history, History)
    next_history = c.output(next_history, "moments next_history", "float32", (4, h, w, 4), aligned=True)
    if out is not None:
        c.output(out, "moments", "float32", (h, w, 3))
    if out_variance is not None:
        c.output(out_variance, "moments out_variance", "float32", (h, w))
    frames = abi.MomentsFrames(width=w, height=h, **{k: v.data_ptr() for k, v in t.items()})
    with c.launch(stream) as sp:
        _check(_lib().vimg_moments_accumulate(C.byref(frames), None if prev is None else C.c_void_p(prev.data_ptr()), matrix,
                                              C.byref(p), C.c_void_p(next_history.data_ptr()),
                                              None if out is None else C.c_void_p(out.data_ptr()),
                                              None if out_variance is None else C.c_void_p(out_variance.data_ptr()), sp))
    return History(c.result(next_history), world_to_pixel)


__all__ = ["accumulate", "params", "history_bytes", "world_to_pixel", "History", "PARAMS", "FRAMES"]
