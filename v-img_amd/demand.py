"""The sampling mask of a sparse preview, decided before the frame is rendered: ctypes mirror of include/vimg_demand.h
(libvimg_demand.so, gfx950).

A frame library beside wtemporal.py's: a sparse preview samples one pixel in stride^2 on a lattice that
knows nothing about the history.  ``mask`` looks every pixel of the frame about to be rendered up in the previous history,
exactly as the accumulate call of that frame will, and asks for a sample now wherever the lookup finds less than
``min_history`` - a pixel the camera has just uncovered does not wait for its lattice turn.  The call only enqueues;
``read`` is the one place that waits.  The binding shares the render binding's tensor check and stream rule
(hip.FrameCall: hip._device_tensor, hip._Launch).  There is no CPU fallback.
"""
import ctypes as C

from . import _abi as abi
from .hip import FrameCall, FrameHistory, _checker, library_params

_lib = abi.demand_lib
_check = _checker(_lib, "vimg_demand_last_error")

FRAMES = ("normal", "position", "depth")
FLOATS = ("min_history", "sigma_normal", "sigma_plane")
COUNTS = ("masked", "needed", "extra", "live")


def params(stride=None, phase=None, **floats):
    """An abi.DemandParams: the library's defaults (vimg_demand_defaults; include/vimg_demand.h names them) with the given
    values in place of them: ``stride``, ``phase``, ``min_history``, ``sigma_normal``, ``sigma_plane``.  The library
    checks the ranges; here an integer field only has to fit its uint32."""
    return library_params("demand", abi.DemandParams, _lib().vimg_demand_defaults, FLOATS, list(floats.items()),
                          ("stride", stride, "0 or 2..4"), ("phase", phase, "0..stride^2 - 1"))


def new_counts(device="cuda"):
    """The four counters of a call on ``device``: int32 words holding uint32 ``masked``, ``needed``, ``extra``, ``live``."""
    import torch
    return torch.zeros(abi.DEMAND_COUNTS, dtype=torch.int32, device=device)


def _counts(counts):
    import torch
    if not isinstance(counts, torch.Tensor) or not counts.is_cuda or not counts.is_contiguous() or \
            counts.numel() * counts.element_size() != 4 * abi.DEMAND_COUNTS:
        raise ValueError(f"demand: counts must be a contiguous CUDA tensor of {4 * abi.DEMAND_COUNTS} bytes (demand.new_counts)")
    return counts


def mask(normal, position, depth, history=None, stride=2, phase=0, min_history=None, sigma_normal=None, sigma_plane=None,
         out=None, out_length=None, counts=None, stream=None):
    """Which pixels of the frame whose first-hit guides are ``normal``, ``position``, ``depth`` ([H, W, 3] float32) to sample
    (vimg_demand_mask): the lattice infill.lattice_mask(H, W, stride, phase) - ``stride`` 0: none - and every live pixel
    whose lookup in ``history`` (a temporal.History, or a moments.History, whose first three planes are read; None: no
    history, every live pixel is needed) finds a length below ``min_history``.  ``position`` and the sigmas are what the
    accumulate call of this frame will be given; then the lengths are that call's own.  Returns (mask [H, W] uint8,
    length [H, W] float32, counts): ``counts`` is a CUDA tensor of four int32 words that ``read`` turns into a dict.
    CUDA tensors are read where they are; numpy arrays are copied up, and with a numpy ``normal`` the mask and the lengths
    come back as numpy arrays (the counts stay on the device).  ``out``, ``out_length``: the CUDA tensors to write;
    ``out_length`` and ``counts`` may be False for none (None is then returned for it).  The parameters default to the
    library's (include/vimg_demand.h).  The call only enqueues, on ``stream`` or torch's current stream: read() is what
    waits."""
    shape = getattr(normal, "shape", None)
    if shape is None or len(shape) != 3 or shape[2] != 3:
        raise ValueError(f"demand normal: shape must be (H, W, 3), not {None if shape is None else tuple(shape)}")
    c = FrameCall("demand", normal)
    h, w = c.h, c.w
    p = params(stride, phase, min_history=min_history, sigma_normal=sigma_normal, sigma_plane=sigma_plane)
    t = c.frames(FRAMES, (normal, position, depth))
    if history is not None and not isinstance(history, FrameHistory):
        raise ValueError("demand: history must be a temporal.History or a moments.History")
    prev, matrix = c.history(history, type(history))
    out = c.output(out, "demand", "uint8", (h, w))
    if out_length is not False:
        out_length = c.output(out_length, "demand out_length", "float32", (h, w))
    if counts is not False:
        counts = c.own(new_counts()) if counts is None else c.use(_counts(counts))
    frames = abi.DemandFrames(width=w, height=h, **{k: v.data_ptr() for k, v in t.items()})
    with c.launch(stream) as sp:
        _check(_lib().vimg_demand_mask(C.byref(frames), None if prev is None else C.c_void_p(prev.data_ptr()), matrix, C.byref(p),
                                       C.c_void_p(out.data_ptr()), None if out_length is False else C.c_void_p(out_length.data_ptr()),
                                       None if counts is False else C.c_void_p(counts.data_ptr()), sp))
    return c.result(out), (None if out_length is False else c.result(out_length)), (None if counts is False else counts)


def read(counts):
    """The counters of a call as a dict: ``masked`` (pixels to sample), ``needed`` (live pixels with less than min_history),
    ``extra`` (needed pixels off the lattice: what the call adds to a lattice frame), ``live``.  Copies the four words to
    the host: the one call of this module that waits for the device."""
    words = _counts(counts).cpu().numpy().view("uint32")
    return {name: int(v) for name, v in zip(COUNTS, words)}


__all__ = ["mask", "params", "new_counts", "read", "FRAMES", "FLOATS", "COUNTS"]
