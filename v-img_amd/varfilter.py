"""The variance-guided a-trous filter over frames in device memory: ctypes mirror of include/vimg_varfilter.h
(libvimg_varfilter.so, gfx950).

A frame library beside filter.py's: the same frames, and beside them the variance of each pixel's
mean luminance, which a progressive accumulator knows (Progressive.variance) and which the filter estimates where it
does not.  The binding shares the render binding's tensor check and stream rule (hip.FrameCall: hip._device_tensor,
hip._Launch).  There is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _abi as abi
from .filter import FRAMES, GUIDES
from .hip import FrameCall, _Tensors, _checker, library_params

_lib = abi.varfilter_lib
_check = _checker(_lib, "vimg_varfilter_last_error")

FLOATS = ("sigma_luminance", "sigma_normal", "sigma_plane", "albedo_floor", "variance_floor")


def params(iterations=None, sigma_luminance=None, sigma_normal=None, sigma_plane=None, albedo_floor=None, variance_floor=None):
    """An abi.VarFilterParams: the library's defaults (vimg_varfilter_defaults; include/vimg_varfilter.h names them)
    with the given values in place of them."""
    return library_params("varfilter", abi.VarFilterParams, _lib().vimg_varfilter_defaults, FLOATS,
                          zip(FLOATS, (sigma_luminance, sigma_normal, sigma_plane, albedo_floor, variance_floor)),
                          ("iterations", iterations, "1..12"))


def workspace_bytes(width, height):
    return int(_lib().vimg_varfilter_workspace(width, height))


def atrous(color, normal, position, depth, albedo=None, variance=None, iterations=None, sigma_luminance=None, sigma_normal=None,
           sigma_plane=None, albedo_floor=None, variance_floor=None, out=None, out_variance=None, workspace=None, stream=None):
    """The variance-guided a-trous filter (vimg_varfilter_atrous) of a noisy ``color`` frame guided by the first-hit
    feature frames ``normal``, ``position``, ``depth`` and, for demodulation, ``albedo`` - all [H, W, 3] float32 - and
    by ``variance``, the [H, W] float32 variance of each pixel's mean luminance (Progressive.variance; NaN = unknown;
    None: every pixel's is estimated from its surroundings).  Returns (filtered [H, W, 3], its variance [H, W]).  CUDA
    tensors are read where they are and the results are CUDA tensors; numpy arrays are copied up, and with a numpy
    ``color`` numpy arrays come back.  The parameters default to the library's (include/vimg_varfilter.h).  ``out``
    may be ``color`` itself and ``out_variance`` may be ``variance`` itself; ``workspace``: a contiguous, 16-byte
    aligned CUDA tensor of at least workspace_bytes(W, H) bytes (64 per pixel), allocated here when None.  The call
    only enqueues, on ``stream`` or torch's current stream."""
    c = FrameCall("varfilter", color)
    h, w = c.h, c.w
    p = params(iterations, sigma_luminance, sigma_normal, sigma_plane, albedo_floor, variance_floor)
    t = c.frames(FRAMES, (color, normal, position, depth, albedo), optional=("albedo",))
    if variance is not None:
        t["variance"] = c.take(variance, "varfilter variance", ("float32",), (h, w))
    out = c.output(out, "varfilter", "float32", (h, w, 3))
    out_variance = c.output(out_variance, "varfilter out_variance", "float32", (h, w))
    workspace = c.workspace(workspace, workspace_bytes(w, h))
    frames = abi.VarFilterFrames(width=w, height=h, **{k: v.data_ptr() for k, v in t.items()})
    with c.launch(stream) as sp:
        _check(_lib().vimg_varfilter_atrous(C.byref(frames), C.byref(p), C.c_void_p(out.data_ptr()),
                                            C.c_void_p(out_variance.data_ptr()), C.c_void_p(workspace.data_ptr()),
                                            workspace.numel() * workspace.element_size(), sp))
    return c.result(out), c.result(out_variance)


def variance(count, batches, m2, out=None, stream=None):
    """The variance frame of an accumulator's state (vimg_varfilter_variance): ``count`` N and ``batches`` K, [H, W]
    uint32 (numpy) or int32 holding the same bits (torch has no uint32 arithmetic; numpy int32 too), and ``m2``
    [H, W] float32, as vimg_hip_progressive_state writes them.  Returns the [H, W] float32 variance of each pixel's
    mean luminance, NaN where K < 2 or N is 0.  Numpy in, numpy out; CUDA tensors in, a CUDA tensor out."""
    import torch
    shape = getattr(m2, "shape", None)
    if shape is None or len(shape) != 2:
        raise ValueError(f"varfilter variance m2: shape must be (H, W), not {None if shape is None else tuple(shape)}")
    h, w = int(shape[0]), int(shape[1])
    c = _Tensors(to_host=not isinstance(m2, torch.Tensor))
    as_i32 = lambda a: a.view(np.int32) if isinstance(a, np.ndarray) and a.dtype == np.uint32 else a
    n = c.take(as_i32(count), "varfilter variance count", ("int32",), (h, w))
    k = c.take(as_i32(batches), "varfilter variance batches", ("int32",), (h, w))
    m = c.take(m2, "varfilter variance m2", ("float32",), (h, w))
    out = c.output(out, "varfilter variance", "float32", (h, w))
    with c.launch(stream) as sp:
        _check(_lib().vimg_varfilter_variance(w, h, C.c_void_p(n.data_ptr()), C.c_void_p(k.data_ptr()), C.c_void_p(m.data_ptr()),
                                              C.c_void_p(out.data_ptr()), sp))
    return c.result(out)


__all__ = ["atrous", "params", "workspace_bytes", "variance", "GUIDES"]
