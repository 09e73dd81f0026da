"""Filters over frames in device memory: ctypes mirror of include/vimg_filter.h (libvimg_filter.so, gfx950).

A library of its own beside the render library: a filter reads frames, never a scene.  The
binding shares the render binding's tensor check and stream rule (hip._device_tensor, hip._Launch), so a filter
call is ordered against torch exactly as a render is.  There is no CPU fallback.
"""
import ctypes as C

from . import _abi as abi
from .hip import HipError, _Launch, _device_tensor

FRAMES = ("color", "normal", "position", "depth", "albedo")
GUIDES = ("albedo", "normal", "position", "depth")     # the feature frames the filter reads beside the colour


def _lib():
    return abi.filter_lib()


def _check(rc):
    if rc < 0:
        raise HipError(f"[{rc}] " + _lib().vimg_filter_last_error().decode())
    return rc


def atrous_params(iterations=None, sigma_color=None, sigma_normal=None, sigma_plane=None, albedo_floor=None):
    """An abi.AtrousParams: the library's defaults (vimg_filter_atrous_defaults; include/vimg_filter.h names them) with
    the given values in place of them."""
    p = abi.AtrousParams()
    _lib().vimg_filter_atrous_defaults(C.byref(p))
    if iterations is not None:
        if not 0 <= int(iterations) < 2 ** 32:
            raise ValueError(f"atrous: iterations must be 1..12, not {iterations}")
        p.iterations = int(iterations)
    for name, v in (("sigma_color", sigma_color), ("sigma_normal", sigma_normal), ("sigma_plane", sigma_plane),
                    ("albedo_floor", albedo_floor)):
        if v is not None:
            setattr(p, name, float(v))
    return p


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
    import torch
    shape = getattr(color, "shape", None)
    if shape is None or len(shape) != 3 or shape[2] != 3:
        raise ValueError(f"atrous color: shape must be (H, W, 3), not {None if shape is None else tuple(shape)}")
    h, w = int(shape[0]), int(shape[1])
    params = atrous_params(iterations, sigma_color, sigma_normal, sigma_plane, albedo_floor)
    made, used, t = [], [], {}
    for name, a in zip(FRAMES, (color, normal, position, depth, albedo)):
        if a is None and name == "albedo":
            continue
        t[name], host = _device_tensor(a, f"atrous {name}", ("float32",), (h, w, 3))
        (made if host else used).append(t[name])
    to_host = not isinstance(color, torch.Tensor)
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        made.append(out)
    else:
        used.append(_device_tensor(out, "atrous", ("float32",), (h, w, 3), out=True)[0])
    if workspace is None:
        workspace = torch.empty((atrous_workspace_bytes(w, h),), dtype=torch.uint8, device="cuda")
        made.append(workspace)
    else:
        if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or not workspace.is_contiguous():
            raise ValueError("atrous: workspace must be a contiguous CUDA tensor")
        used.append(workspace)
    frames = abi.FilterFrames(width=w, height=h, **{k: v.data_ptr() for k, v in t.items()})
    with _Launch(stream, made, used, to_host=to_host) as sp:
        _check(_lib().vimg_filter_atrous(C.byref(frames), C.byref(params), C.c_void_p(out.data_ptr()),
                                         C.c_void_p(workspace.data_ptr()), workspace.numel() * workspace.element_size(), sp))
    return out.cpu().numpy() if to_host else out


__all__ = ["atrous", "atrous_params", "atrous_workspace_bytes", "GUIDES"]
