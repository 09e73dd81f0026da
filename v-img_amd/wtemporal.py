"""Temporal accumulation with a weight per pixel, over frames in device memory: ctypes mirror of
include/vimg_wtemporal.h (libvimg_wtemporal.so, gfx950).

A frame library beside temporal.py's: vimg_temporal_accumulate has one current_weight for the whole
picture, here each pixel says how much its current colour is worth - a pixel sampled this frame blends as it does
there, a pixel that infill.reconstruct filled takes its reprojected history when it has one, and the fill is used only
where the history has nothing.  The history is temporal.History: either library continues what the other wrote.  The
binding shares the render binding's tensor check and stream rule (hip.FrameCall: hip._device_tensor, hip._Launch).
There is no CPU fallback.
"""
import ctypes as C

from . import _abi as abi
from .hip import FrameCall, _checker, library_params
from .temporal import FRAMES, History, history_bytes, world_to_pixel

PARAMS = ("max_history", "sigma_normal", "sigma_plane")
# What a pixel filled by infill.reconstruct (its code 1, the guided fill) is worth, in samples: the value with the
# lowest geometric-mean error of tools/wtemporal_sweep.py's orbits (1/16 .. 1/4 lie within 3 %).
FILL_WEIGHT = 0.0625

_lib = abi.wtemporal_lib
_check = _checker(_lib, "vimg_wtemporal_last_error")


def wtemporal_params(max_history=None, sigma_normal=None, sigma_plane=None):
    """An abi.WTemporalParams: the library's defaults (vimg_wtemporal_defaults; include/vimg_wtemporal.h names them)
    with the given values in place of them."""
    return _params(zip(PARAMS, (max_history, sigma_normal, sigma_plane)))


def _params(given):
    return library_params("wtemporal", abi.WTemporalParams, _lib().vimg_wtemporal_defaults, PARAMS, given)


def sparse_weights(count, code, batches=None, fill_weight=FILL_WEIGHT):
    """The [H, W] float32 weight frame of a sparsely sampled picture that infill.reconstruct filled: ``batches`` (1
    when None) where ``count`` > 0 - a pixel with samples weighs the increments it took part in, as
    TemporalPreview's current_weight does for a whole frame - ``fill_weight`` where the infill ``code`` is 1 (filled
    from its own surface), and 0 where it is 2 or 3 (the unguided fallback, a hole: shown when nothing better is there,
    never carried).  ``count``, ``code`` and ``batches`` are [H, W] torch tensors on one device (Progressive.counts(),
    reconstruct's codes, Progressive.state()["batches"]); torch operations on the current stream, no kernel of the
    library."""
    import torch
    fill_weight = float(fill_weight)
    if not fill_weight >= 0.0:
        raise ValueError(f"wtemporal: fill_weight must be >= 0, not {fill_weight}")
    if tuple(count.shape) != tuple(code.shape) or (batches is not None and tuple(batches.shape) != tuple(count.shape)):
        raise ValueError("wtemporal: count, code and batches must have one shape")
    filled = (code == abi.INFILL_GUIDED).to(torch.float32) * fill_weight
    own = torch.ones_like(filled) if batches is None else batches.to(torch.float32)
    return torch.where(count > 0, own, filled)


def accumulate(color, normal, position, depth, weight, history=None, world_to_pixel=None, out=None, out_code=None,
               next_history=None, stream=None, **params):
    """One step of temporal accumulation with per-pixel weights (vimg_wtemporal_accumulate): temporal.accumulate with
    ``weight``, an [H, W] float32 frame, in place of current_weight.  Per pixel: weight > 0 blends the colour with the
    reprojected history at weight / (length + weight), or starts a history of length min(weight, 1) where there is
    none; weight 0 (or negative, or NaN) carries the history alone, or - where there is none - shows the colour with
    length 0, which no later frame takes up.  Returns (the next temporal.History, code [H, W] uint8: 0 not live,
    1 started, 2 blended, 3 carried, 4 shown).  CUDA tensors are read where they are; numpy arrays are copied up, and
    with a numpy ``color`` the History holds a numpy array and the codes are one.  ``out``: a [H, W, 3] float32 CUDA
    tensor that gets the accumulated colour, which may be ``color`` itself; ``out_code``: the [H, W] uint8 CUDA tensor
    to write, or False for none (None is then returned for it); ``next_history``: the [3, H, W, 4] float32 CUDA tensor
    to write (not the one ``history`` holds), allocated when None.  ``params``: max_history, sigma_normal, sigma_plane,
    default the library's (include/vimg_wtemporal.h).  The call only enqueues, on ``stream`` or torch's current
    stream."""
    c = FrameCall("wtemporal", color)
    h, w = c.h, c.w
    p = _params(params.items())
    t = c.frames(FRAMES, (color, normal, position, depth))
    t["weight"] = c.take(weight, "wtemporal weight", ("float32",), (h, w))
    prev, matrix = c.history(history, History)
    next_history = c.output(next_history, "wtemporal next_history", "float32", (3, h, w, 4), aligned=True)
    if out is not None:
        c.output(out, "wtemporal", "float32", (h, w, 3))
    if out_code is not False:
        out_code = c.output(out_code, "wtemporal out_code", "uint8", (h, w))
    frames = abi.WTemporalFrames(width=w, height=h, **{k: v.data_ptr() for k, v in t.items()})
    with c.launch(stream) as sp:
        _check(_lib().vimg_wtemporal_accumulate(C.byref(frames), None if prev is None else C.c_void_p(prev.data_ptr()), matrix,
                                                C.byref(p), C.c_void_p(next_history.data_ptr()),
                                                None if out is None else C.c_void_p(out.data_ptr()),
                                                None if out_code is False else C.c_void_p(out_code.data_ptr()), sp))
    return History(c.result(next_history), world_to_pixel), (None if out_code is False else c.result(out_code))


__all__ = ["accumulate", "wtemporal_params", "sparse_weights", "history_bytes", "world_to_pixel", "History", "FILL_WEIGHT",
           "FRAMES", "PARAMS"]
