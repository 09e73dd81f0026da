"""Histogram auto-exposure of a frame in device memory, its state kept there from frame to frame: ctypes mirror of
include/vimg_exposure.h (libvimg_exposure.so, gfx950).

A frame library beside despeckle.py's: the previews return linear HDR radiance, and ``adapt`` gives it a
brightness - it meters the frame's luminance into a log2 histogram, takes the mean of the ranks between two permilles
(which one firefly cannot move, where a maximum is the firefly), moves the exposure in ``state`` toward key / metered and
scales the frame by it.  The exposure never visits the host: ``adapt`` only enqueues, and ``read`` is the one place that
waits.  The binding shares the render binding's tensor check and stream rule (hip.FrameCall: hip._device_tensor,
hip._Launch).  There is no CPU fallback.
"""
import ctypes as C

from . import _abi as abi
from .hip import FrameCall, _checker, library_params

_lib = abi.exposure_lib
_check = _checker(_lib, "vimg_exposure_last_error")

FLOATS = ("key", "min_exposure", "max_exposure", "rate_brighten", "rate_darken")
STATE_WORDS = abi.EXPOSURE_STATE_BYTES // 4


def params(low_permille=None, high_permille=None, **floats):
    """An abi.ExposureParams: the library's defaults (vimg_exposure_defaults; include/vimg_exposure.h names them) with the
    given values in place of them: ``low_permille``, ``high_permille``, ``key``, ``min_exposure``, ``max_exposure``,
    ``rate_brighten``, ``rate_darken``.  The library checks the ranges; here an integer field only has to fit its uint32."""
    return library_params("exposure", abi.ExposureParams, _lib().vimg_exposure_defaults, FLOATS, list(floats.items()),
                          ("low_permille", low_permille, "0..high_permille - 1"),
                          ("high_permille", high_permille, "low_permille + 1..1000"))


def new_state(device="cuda"):
    """A fresh exposure state on ``device``: abi.EXPOSURE_STATE_BYTES zero bytes, as 260 int32 words (abi.ExposureState
    names them).  Its exposure is 1 until a call has metered something."""
    import torch
    return torch.zeros(STATE_WORDS, dtype=torch.int32, device=device)


def _state(state):
    import torch
    if not isinstance(state, torch.Tensor) or not state.is_cuda or not state.is_contiguous() or \
            state.numel() * state.element_size() != abi.EXPOSURE_STATE_BYTES:
        raise ValueError(f"exposure: state must be a contiguous CUDA tensor of {abi.EXPOSURE_STATE_BYTES} bytes (exposure.new_state)")
    return state


def adapt(color, depth=None, state=None, out=None, stream=None, **params_kw):
    """Meters ``color``, moves the exposure in ``state`` and scales the frame by it (vimg_exposure_adapt).  ``color`` and,
    to keep misses out of the metering, the first-hit ``depth`` frame are [H, W, 3] float32.  ``state``: new_state()'s
    tensor, carried from call to call - None: a fresh one, so the frame is scaled to its own target.  ``out``: None -
    meter only, nothing is written but the state; True - a new frame; a tensor - that one, which may be ``color`` itself.
    Returns (the scaled [H, W, 3] image or None, state).  CUDA tensors are read where they are and the result is a CUDA
    tensor; numpy arrays are copied up, and with a numpy ``color`` a numpy array comes back (the state stays on the
    device).  ``params_kw``: the parameters of ``params``, which default to the library's (include/vimg_exposure.h).
    The call only enqueues, on ``stream`` or torch's current stream: read() is what waits."""
    c = FrameCall("exposure", color)
    h, w = c.h, c.w
    p = params(**params_kw)
    t = c.frames(("color", "depth"), (color, depth), optional=("depth",))
    state = c.own(new_state()) if state is None else c.use(_state(state))
    if out is not None:
        out = c.output(None if out is True else out, "exposure", "float32", (h, w, 3))
    frames = abi.ExposureFrames(width=w, height=h, **{k: v.data_ptr() for k, v in t.items()})
    with c.launch(stream) as sp:
        _check(_lib().vimg_exposure_adapt(C.byref(frames), C.byref(p), C.c_void_p(state.data_ptr()),
                                          None if out is None else C.c_void_p(out.data_ptr()), sp))
    return None if out is None else c.result(out), state


def read(state):
    """The scalars of ``state`` as a dict: ``exposure`` (what the last call scaled by; 1.0 for a state that has metered
    nothing yet), ``frames``, ``metered``, ``counted``.  Copies the state to the host: the one call of this module that
    waits for the device."""
    s = abi.ExposureState.from_buffer_copy(_state(state).cpu().numpy().tobytes())
    return {"exposure": float(s.exposure) if s.frames else 1.0, "frames": int(s.frames), "metered": float(s.metered),
            "counted": int(s.counted)}


__all__ = ["adapt", "new_state", "params", "read"]
