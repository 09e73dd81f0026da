"""Reconstruction of sparsely sampled frames in device memory: ctypes mirror of include/vimg_infill.h
(libvimg_infill.so, gfx950).

A frame library beside filter.py's: a masked progressive increment gives samples to some pixels - one
in four on a stride-2 lattice - and the first-hit feature frames describe every pixel; ``reconstruct`` fills the pixels
without samples from the sampled ones around them on the same surface.  The binding shares the render binding's tensor
check and stream rule (hip.FrameCall: hip._device_tensor, hip._Launch).  There is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _abi as abi
from .filter import FRAMES, GUIDES
from .hip import FrameCall, _checker, library_params

_lib = abi.infill_lib
_check = _checker(_lib, "vimg_infill_last_error")

FLOATS = ("sigma_normal", "sigma_plane", "albedo_floor")
MIN_STRIDE, MAX_STRIDE = 2, 4


def params(radius=None, sigma_normal=None, sigma_plane=None, albedo_floor=None):
    """An abi.InfillParams: the library's defaults (vimg_infill_defaults; include/vimg_infill.h names them) with the
    given values in place of them."""
    return library_params("infill", abi.InfillParams, _lib().vimg_infill_defaults, FLOATS,
                          zip(FLOATS, (sigma_normal, sigma_plane, albedo_floor)), ("radius", radius, f"1..{abi.INFILL_MAX_RADIUS}"))


def workspace_bytes(width, height):
    return int(_lib().vimg_infill_workspace(width, height))


def lattice_cell(stride, phase):
    """The cell (cx, cy) of the ``phase``-th lattice of ``stride``: (phase % stride, (phase // stride + phase % stride)
    % stride) - the diagonals of the stride x stride cell grid, one after the other.  Every cell is visited once in
    stride^2 phases, and the first ``stride`` phases already touch every row and every column of cells."""
    stride, phase = int(stride), int(phase)
    if not MIN_STRIDE <= stride <= MAX_STRIDE:
        raise ValueError(f"infill: stride must be {MIN_STRIDE}..{MAX_STRIDE}, not {stride}")
    if not 0 <= phase < stride * stride:
        raise ValueError(f"infill: phase must be 0..{stride * stride - 1} at stride {stride}, not {phase}")
    return phase % stride, (phase // stride + phase % stride) % stride


def lattice_mask(height, width, stride, phase, device="cuda"):
    """The [H, W] uint8 tensor on ``device`` (a CUDA tensor unless asked otherwise) that is 1 where
    (x % stride, y % stride) is ``lattice_cell(stride, phase)`` and 0 elsewhere: the mask of one sparse increment
    (Progressive.render's ``mask``).  Stride 2..4, phase 0..stride^2 - 1; the stride^2 phases partition the frame."""
    import torch
    cx, cy = lattice_cell(stride, phase)
    mask = torch.zeros((int(height), int(width)), dtype=torch.uint8, device=device)
    mask[cy::stride, cx::stride] = 1
    return mask


def reconstruct(color, normal, position, depth, count, albedo=None, radius=None, sigma_normal=None, sigma_plane=None,
                albedo_floor=None, out=None, out_code=None, workspace=None, stream=None):
    """Fills the pixels of ``color`` that have no samples (vimg_infill_reconstruct).  ``color`` and the first-hit
    feature frames ``normal``, ``position``, ``depth`` and, for demodulation, ``albedo`` are [H, W, 3] float32;
    ``count`` is [H, W], the samples each pixel has had - uint32 (numpy), int32 holding the same bits, or int64 as
    Progressive.counts() returns it.  A pixel with count 0 gets the guide-weighted tent mean of the sampled pixels of
    its surface within ``radius``, times its own albedo.  Returns (image [H, W, 3] float32, code [H, W] uint8: 0
    sampled, 1 guided, 2 unguided fallback, 3 hole).  CUDA tensors are read where they are and the results are CUDA
    tensors; numpy arrays are copied up, and with a numpy ``color`` numpy arrays come back.  The parameters default to
    the library's (include/vimg_infill.h).  ``out`` may be ``color`` itself; ``workspace``: a contiguous, 16-byte aligned
    CUDA tensor of at least workspace_bytes(W, H) bytes (48 per pixel), allocated here when None.  The call only
    enqueues, on ``stream`` or torch's current stream."""
    import torch
    c = FrameCall("infill", color)
    h, w = c.h, c.w
    p = params(radius, sigma_normal, sigma_plane, albedo_floor)
    t = c.frames(FRAMES, (color, normal, position, depth, albedo), optional=("albedo",))
    if isinstance(count, np.ndarray) and count.dtype in (np.uint32, np.int64):
        count = count.astype(np.uint32).view(np.int32)
    elif isinstance(count, torch.Tensor) and count.dtype == torch.int64:
        with torch.cuda.stream(stream):          # (None: torch's current stream, where counts() widened it)
            count = count.to(torch.int32)
    t["count"] = c.take(count, "infill count", ("int32",), (h, w))
    out = c.output(out, "infill", "float32", (h, w, 3))
    out_code = c.output(out_code, "infill out_code", "uint8", (h, w))
    workspace = c.workspace(workspace, workspace_bytes(w, h))
    frames = abi.InfillFrames(width=w, height=h, **{k: v.data_ptr() for k, v in t.items()})
    with c.launch(stream) as sp:
        _check(_lib().vimg_infill_reconstruct(C.byref(frames), C.byref(p), C.c_void_p(out.data_ptr()),
                                              C.c_void_p(out_code.data_ptr()), C.c_void_p(workspace.data_ptr()),
                                              workspace.numel() * workspace.element_size(), sp))
    return c.result(out), c.result(out_code)


__all__ = ["reconstruct", "params", "workspace_bytes", "lattice_cell", "lattice_mask", "GUIDES"]
