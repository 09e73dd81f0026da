"""GPU side of the boundary: ctypes mirror of include/vimg_hip.h (libvimg_hip.so, gfx950).

Mirrors the reference's hot-path entry points: ``render`` = scene_integrator
(reference include/integrators.h:36-153), ``trace_pixel`` = trace_pixel (:181-220).
torch is used only as the owner of device memory and streams; there is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _abi as abi
from .host import HostScene, camera_lookat, make_params


# floats per item of DeviceScene.probe, kind -> (in, out): the n_in / n_out tables of vimg_hip_probe (csrc/vimg_hip.hip)
PROBE_IO = {1: (4, 8), 2: (6, 28), 3: (7, 1), 4: (12, 5), 5: (8, 7), 6: (4, 10), 7: (5, 4), 8: (1, 5), 9: (8, 8), 10: (12, 8), 11: (5, 1)}
PROBE_LAUNCH_BUILD = 11


class HipError(RuntimeError):
    pass


def _lib():
    return abi.hip_lib()


def _checker(lib, last_error):
    """The return-code check of the library ``lib()`` (abi.hip_lib, ...), whose message function ``last_error`` names."""
    def check(rc):
        if rc < 0:
            raise HipError(f"[{rc}] " + getattr(lib(), last_error)().decode())
        return rc
    return check


_check = _checker(_lib, "vimg_hip_last_error")


_side = None


class _Launch:
    """The one stream rule of the binding: the stream a call with torch tensors enqueues on, and what
    orders its tensors against it.  ``stream=None`` means torch's CURRENT stream, never the library's private one
    (which is non-blocking and would not be ordered against the fill of `out` or against torch consumers of the
    result).  The legacy null stream has no handle the library could tell from "no stream given", so work for it
    goes to a side stream that waits for the null stream before the launch and that the null stream waits for after.

    ``made``: the tensors this call allocated or copied up from numpy, ``used``: the caller's.  Both kinds were
    made on torch's current stream, so a launch on another stream first waits for the current one when there are
    ``made`` tensors (it neither reads a copy not yet made nor writes memory the caching allocator handed out while
    current-stream work on it is still pending), and afterwards records every tensor on the stream that ran it:
    the allocator must not hand their memory out again before that stream has passed the launch.  ``to_host``:
    the results go back to numpy on the current stream, which waits for the launch first.  On the current stream
    itself none of this is needed, and nothing is done."""

    def __init__(self, stream, made=(), used=(), to_host=False):
        import torch
        global _side
        self.cur = stream if stream is not None else torch.cuda.current_stream()
        self.side = None
        if self.cur.cuda_stream == 0:
            if _side is None:
                _side = torch.cuda.Stream()
            self.side = _side
        self.home = None       # torch's current stream, when the launch goes to another one
        if stream is not None and (made or used):
            home = torch.cuda.current_stream()
            if home.cuda_stream != stream.cuda_stream:
                self.home, self.made, self.used, self.to_host = home, made, used, to_host

    def __enter__(self):
        if self.home is not None and self.made:
            self.cur.wait_stream(self.home)
        if self.side is not None:
            self.side.wait_stream(self.cur)
            return C.c_void_p(self.side.cuda_stream)
        return C.c_void_p(self.cur.cuda_stream)

    def __exit__(self, *exc):
        if self.side is not None:
            self.cur.wait_stream(self.side)
        if self.home is not None:
            ran = self.side if self.side is not None else self.cur
            for t in (*self.made, *self.used):
                if t is not None and t.numel():
                    t.record_stream(ran)
            if self.to_host:
                self.home.wait_stream(self.cur)
        return False


def _upload(a):
    """A numpy array's device copy (a blocking copy on torch's current stream)."""
    import torch
    return torch.from_numpy(a).to("cuda")


def _device_tensor(a, what, dtypes, shape, aligned=False, out=False):
    """(device tensor, came from numpy) for an argument of a launch: a CUDA tensor on the current device as it is,
    a numpy array copied up (a bool one viewed as uint8).  ``dtypes``: the names allowed ("float32", ...);
    ``shape``: None leaves a dimension open (the N of [N, 8]); ``aligned``: the data must be 16-byte aligned.
    Type, dtype and a numpy array's shape are checked before anything is copied.  ``out``: a caller's output
    buffer - a tensor of exactly dtypes[0] and ``shape``, refused in one sentence."""
    import torch

    def said():      # (only a refusal spells the shape out)
        return str(tuple("N" if d is None else d for d in shape)).replace("'", "")

    def bad(why):
        if out:
            why = f"out must be a contiguous torch.{dtypes[0]} CUDA tensor of shape {said()} on the current device"
        return ValueError(f"{what}: {why}")

    def fits(got):
        return len(got) == len(shape) and all(w is None or w == g for w, g in zip(shape, got))

    if isinstance(a, np.ndarray) and not out:
        if a.dtype.name not in dtypes:
            raise bad(f"dtype must be {' or '.join(dtypes)}, not {a.dtype}")
        if not fits(a.shape):
            raise bad(f"shape must be {said()}, not {tuple(a.shape)}")
        a = np.ascontiguousarray(a)
        t, host = _upload(a.view(np.uint8) if a.dtype == np.bool_ else a), True
    elif isinstance(a, torch.Tensor):
        if str(a.dtype)[len("torch."):] not in (dtypes[:1] if out else dtypes):
            raise bad(f"dtype must be {' or '.join(dtypes)}, not {a.dtype}")
        if not a.is_cuda or a.device.index != torch.cuda.current_device():
            raise bad(f"the tensor must be on the current CUDA device, not {a.device}")
        if not a.is_contiguous():
            raise bad("the tensor must be contiguous")
        if not fits(a.shape):
            raise bad(f"shape must be {said()}, not {tuple(a.shape)}")
        t, host = a, False
    else:
        raise bad(f"expected a torch CUDA tensor or a numpy array, not {type(a).__name__}")
    if aligned and t.numel() and t.data_ptr() % 16:
        raise ValueError(f"{what}: out must be 16-byte aligned" if out else f"{what}: the tensor's data must be 16-byte aligned")
    return t, host


class _Tensors:
    """The tensors of one call, collected as they are taken and sorted into the ``made`` / ``used`` of its _Launch:
    ``made`` is what the call copied up from numpy or allocated, ``used`` what the caller handed in.  ``to_host``:
    numpy in, numpy out - the call's input came from numpy, so ``result`` takes its output back there."""

    def __init__(self, to_host=False):
        self.made, self.used, self.to_host = [], [], to_host

    def take(self, a, what, dtypes, shape, aligned=False):
        """An input, through _device_tensor: a numpy array's device copy is made, a CUDA tensor is used."""
        t, host = _device_tensor(a, what, dtypes, shape, aligned)
        (self.made if host else self.used).append(t)
        return t

    def own(self, t):          # a tensor this call allocated
        self.made.append(t)
        return t

    def use(self, t):          # a caller's tensor, as it is
        self.used.append(t)
        return t

    def output(self, out, what, dtype, shape, aligned=False):
        """The output of the call: allocated when ``out`` is None, else the caller's buffer, which must be exactly a
        torch.``dtype`` CUDA tensor of ``shape`` (_device_tensor's out=True)."""
        if out is None:
            import torch
            return self.own(torch.empty(shape, dtype=getattr(torch, dtype), device="cuda"))
        return self.use(_device_tensor(out, what, (dtype,), shape, aligned, out=True)[0])

    def launch(self, stream):
        return _Launch(stream, self.made, self.used, to_host=self.to_host)

    def result(self, t):
        return t.cpu().numpy() if self.to_host else t


class FrameCall(_Tensors):
    """The tensors of one call of the frame library ``what`` ("atrous", "temporal") on frames of ``color``'s shape."""

    def __init__(self, what, color):
        import torch
        super().__init__(to_host=not isinstance(color, torch.Tensor))
        shape = getattr(color, "shape", None)
        if shape is None or len(shape) != 3 or shape[2] != 3:
            raise ValueError(f"{what} color: shape must be (H, W, 3), not {None if shape is None else tuple(shape)}")
        self.what, self.h, self.w = what, int(shape[0]), int(shape[1])

    def frames(self, names, arrays, optional=()):
        """name -> device tensor of the [H, W, 3] float32 frames; a None one out of ``optional`` is left out."""
        shape = (self.h, self.w, 3)
        return {name: self.take(a, f"{self.what} {name}", ("float32",), shape)
                for name, a in zip(names, arrays) if not (a is None and name in optional)}

    def history(self, history, cls):
        """(device tensor, the 12 floats of its matrix) of the ``history`` an accumulate call reprojects, which must be
        a ``cls`` (a FrameHistory class) that knows its matrix; (None, None) without one."""
        if history is None:
            return None, None
        if not isinstance(history, cls):
            raise ValueError(f"{self.what}: history must be a {cls.__module__.rsplit('.', 1)[-1]}.{cls.__name__}")
        if history.world_to_pixel is None:
            raise ValueError(f"{self.what}: the history does not know its world_to_pixel matrix")
        prev = self.take(history.tensor, f"{self.what} history", ("float32",), (cls.PLANES, self.h, self.w, 4), aligned=True)
        return prev, (abi.f32 * 12)(*history.world_to_pixel.tolist())

    def rewritten(self, history, t):
        """The ``history`` a call rewrote in place through ``t``, what ``take`` made of its tensor: ``history`` itself
        when that is its own CUDA tensor; when it held a numpy array, a new one of its class around ``t``'s copy."""
        return history if t is history.tensor else type(history)(t.cpu().numpy(), history.world_to_pixel)

    def workspace(self, workspace, nbytes):
        """The caller's ``workspace`` as it is, or ``nbytes`` bytes of this call's own when None."""
        import torch
        if workspace is None:
            return self.own(torch.empty((nbytes,), dtype=torch.uint8, device="cuda"))
        if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or not workspace.is_contiguous():
            raise ValueError(f"{self.what}: workspace must be a contiguous CUDA tensor")
        return self.use(workspace)


class FrameHistory:
    """What the histories of the accumulating frame libraries share (temporal.History, moments.History): ``tensor``
    [PLANES, H, W, 4] float32, whose planes open with A = {rgb, length}, G0 = {normal, depth}, G1 = {position, 0}, and
    ``world_to_pixel``, the matrix of the camera its frame was rendered under (None: unknown, the history cannot be
    reprojected).  ``color`` [H, W, 3] and ``length`` [H, W] are views."""
    PLANES = None

    def __init__(self, tensor, world_to_pixel=None):
        if len(tensor.shape) != 4 or tensor.shape[0] != self.PLANES or tensor.shape[3] != 4:
            raise ValueError(f"History: shape must be ({self.PLANES}, H, W, 4), not {tuple(tensor.shape)}")
        self.tensor = tensor
        self.world_to_pixel = None if world_to_pixel is None else np.ascontiguousarray(world_to_pixel, dtype=np.float32).reshape(12)

    @property
    def color(self):
        return self.tensor[0, :, :, :3]

    @property
    def length(self):
        return self.tensor[0, :, :, 3]


def library_params(what, struct, defaults, floats, given, *counts):
    """An abi ``struct`` of parameters: the library's defaults (``defaults`` fills them in) with the values of ``given``
    ((name, value) pairs; None keeps the default) in place of them.  ``floats`` are the names ``given`` may hold - a
    call's keywords with another are refused - and each of ``counts`` = (name, value, "1..12") is one of the library's
    integer fields with the range its sentence names: the library checks that range, here the value only has to fit
    the field's uint32.  The integer fields are looked at first, in the order given."""
    p = struct()
    defaults(C.byref(p))
    for name, v, allowed in counts:
        if v is not None:
            if not 0 <= int(v) < 2 ** 32:
                raise ValueError(f"{what}: {name} must be {allowed}, not {v}")
            setattr(p, name, int(v))
    for name, v in given:
        if name not in floats:
            raise TypeError(f"{what}: unknown parameters {sorted(n for n, _ in given if n not in floats)}; expected some of {floats}")
        if v is not None:
            setattr(p, name, float(v))
    return p


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def device_count():
    return _check(_lib().vimg_hip_device_count())


def init(device=0):
    _check(_lib().vimg_hip_init(device))


class DeviceScene:
    """A scene resident in HBM (vimg_hip_scene_upload_opts).  `options`: abi.HipOptions, or keyword
    arguments for one (scheduler="lane" | "cu", pool_segments=..., ...); nothing given
    = the library's policy."""

    def __init__(self, host_scene: HostScene, options=None, **opt_kw):
        self._lib = _lib()
        h = C.c_void_p()
        if options is None and opt_kw:
            options = abi.HipOptions(**opt_kw)
        self.options = options
        _check(self._lib.vimg_hip_scene_upload_opts(host_scene.view, C.byref(options) if options is not None else None,
                                                    C.byref(h)))
        self._h = h
        self.resolution = host_scene.resolution
        v = host_scene.view.contents
        self.num_vertices, self.num_spheres = int(v.num_vertices), int(v.num_spheres)
        self.num_materials, self.num_textures = int(v.num_materials), int(v.num_textures)
        self._image_sizes = {i: (int(v.textures[i].height), int(v.textures[i].width)) for i in range(v.num_textures)
                             if v.textures[i].type == abi.TEX_IMAGE}
        self.camera = abi.Camera.from_buffer_copy(v.camera)      # the camera of the next launch (set_camera replaces it)
        self.generation = 0      # counts the edits of the resident scene: what a cached feature frame was rendered from
        # the vertex and sphere tables update_geometry / update_materials were last given, as device tensors (None: not
        # since the upload).  A new tensor object per call, never written in place: a held reference is a snapshot
        self.vertices_given, self.spheres_given = None, None

    @property
    def bytes(self):
        return int(self._lib.vimg_hip_scene_bytes(self._h))

    @property
    def kernel(self):
        return self._lib.vimg_hip_scene_kernel(self._h).decode()

    def kernel_for(self, params):
        """Name of the kernel a launch with these parameters gets (the scheduler is chosen per launch)."""
        return self._lib.vimg_hip_launch_kernel(self._h, C.byref(params)).decode()

    def plain_fold_for(self, params):
        """The launch-constant options compiled into the build a frame with these parameters runs (probe 11: a mask of
        plain_build.h's PF_* bits; 0 = the general build)."""
        p = params
        return int(self.probe(PROBE_LAUNCH_BUILD, [[p.integrator, p.samples, p.depth & 0xFFFFFF, p.tile_rank, p.tile_world]])[0, 0])

    def shard_pixels(self, params):
        return _check(self._lib.vimg_hip_shard_pixels(self._h, C.byref(params)))

    def render(self, params, out=None, stats=True, stream=None):
        """Blocking render into a torch CUDA tensor (allocated when ``out`` is None).

        tile_world == 1: returns [H, W, 3] in the reference layout (row 0 = top).
        tile_world  > 1: returns the shard's compact [shard_pixels, 3] buffer."""
        c = _Tensors()
        out = c.own(self._new_output(params)) if out is None else c.use(out)
        st = abi.RenderStats()
        with c.launch(stream) as sp:
            _check(self._lib.vimg_hip_render(self._h, C.byref(params), C.c_void_p(out.data_ptr()), sp,
                                             C.byref(st) if stats else None))
        return (out, st) if stats else out

    def render_features(self, params, features=("albedo", "normal", "depth"), out=None, stream=None):
        """First-hit feature buffers of the frame (or shard) ``params`` describes: a dict name -> float32 CUDA
        tensor in ``render``'s shapes, one launch per feature with ``params``' samples and shard
        (``params.integrator`` is ignored).  ``features``: names out of abi.FEATURES - albedo, normal (the raw
        shading normal), depth, position, uv, coverage; a miss contributes 0 to each.  ``out``: a dict with a
        tensor to write for some or all of the names."""
        unknown = [f for f in features if f not in abi.FEATURES]
        if unknown:
            raise ValueError(f"render_features: expected names out of {abi.FEATURES}, not {unknown}")
        w, h = self.resolution
        p = abi.RenderParams.from_buffer_copy(params)
        p.integrator = abi.INTEGRATOR_COVERAGE      # (the caller's integrator is not even checked)
        shape = (h, w, 3) if p.tile_world == 1 else (self.shard_pixels(p), 3)
        res = {}
        for name in features:
            p.integrator = abi.INTEGRATORS[name]
            given = None if out is None else out.get(name)
            if given is not None:
                given = _device_tensor(given, f"render_features[{name}]", ("float32",), shape, out=True)[0]
            res[name] = self.render(p, out=given, stats=False, stream=stream)
        return res

    def render_denoised(self, params, out=None, stream=None, variance_guided=False, despeckle=None, exposure=None, **filter_kw):
        """``render`` followed by the a-trous filter (vimg_amd.filter.atrous, include/vimg_filter.h) guided by the
        frame's own feature frames: exactly render(params) + render_features(params, ("albedo", "normal",
        "position", "depth")) + filter.atrous(..., **filter_kw).  ``variance_guided``: the variance-guided filter
        (vimg_amd.varfilter.atrous, include/vimg_varfilter.h) instead, with ``filter_kw`` its parameters; a one-shot
        render has no variance, so every pixel's is estimated from its surroundings.  ``despeckle`` (True: the library's
        defaults; a dict: its parameters; None or False: no call): the rendered frame's fireflies are clamped
        (vimg_amd.despeckle.clamp, include/vimg_despeckle.h) before the filter.  ``exposure`` (True, a dict, None or
        False likewise): the filtered frame is scaled in place by the exposure it is metered to, from a fresh state
        (vimg_amd.exposure.adapt, include/vimg_exposure.h).  Returns the filtered [H, W, 3] image (``out`` when given);
        whole frames only."""
        from . import preview
        if params.tile_world != 1:
            raise ValueError("render_denoised: the filter reads whole frames, not shards (tile_world must be 1)")
        clamp, exposed = preview.despeckle_kw(despeckle, "render_denoised"), preview.exposure_kw(exposure, "render_denoised")
        noisy = self.render(params, stats=False, stream=stream)
        guides = self.render_features(params, preview.GUIDES, stream=stream)
        preview.clamp_fireflies(noisy, guides, clamp, stream=stream)
        return preview.expose(preview.denoise(noisy, guides, variance_guided, out=out, stream=stream, **filter_kw), exposed, stream=stream)

    def temporal_preview(self, params, samples=4, denoise=True, feature_samples=4, variance_guided=False, sparse=None,
                         fill_weight=None, antilag=False, motion=None, despeckle=None, exposure=None, demand=None, rectify=None,
                         **temporal_kw):
        """A preview that survives a moving camera: a vimg_amd.preview.TemporalPreview of this scene, which tells what its
        ``frame()`` returns and what every argument chooses (``temporal_kw`` also carries ``filter_kw`` and
        ``scale_sigma_color``).  Whole frames only."""
        from . import preview
        return preview.TemporalPreview(self, params, samples=samples, denoise=denoise, feature_samples=feature_samples,
                                       variance_guided=variance_guided, sparse=sparse, fill_weight=fill_weight, antilag=antilag,
                                       motion=motion, despeckle=despeckle, exposure=exposure, demand=demand, rectify=rectify, **temporal_kw)

    def render_sparse(self, params, stride=2, **kw):
        """A sparse preview in one call: a fresh accumulator, one ``Progressive.render_sparse(params.samples, stride,
        **kw)`` - ``params.samples`` samples for one pixel in stride^2, the others filled from the feature frames
        (vimg_amd.infill, include/vimg_infill.h) - and the accumulator closed.  Returns the [H, W, 3] image."""
        acc = self.progressive(params)
        try:
            return acc.render_sparse(params.samples, stride=stride, **kw)
        finally:
            acc.close()

    def _new_output(self, params, zero_slab=True):
        """A frame [H, W, 3] for these parameters, or the shard's compact slab [shard_pixels, 3] when tile_world > 1
        (zeroed, when asked: a ragged shard has slots off the image that no launch writes)."""
        import torch
        w, h = self.resolution
        if params.tile_world == 1:
            return torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        return (torch.zeros if zero_slab else torch.empty)((self.shard_pixels(params), 3), dtype=torch.float32, device="cuda")

    def update_geometry(self, vertices=None, normals=None, spheres=None, stream=None):
        """New positions for the resident scene (vimg_hip_scene_update_geometry): vertices and normals
        [num_vertices, 3], spheres [num_spheres, 4] (centre, radius), float32; None = unchanged.  The records
        baked from positions and the tree's boxes are rebuilt on the GPU; the call returns when the scene is
        consistent.  Progressive accumulators of the scene must be reset afterwards."""
        self.update_materials(vertices=vertices, normals=normals, spheres=spheres, stream=stream)

    @staticmethod
    def _record_table(records, n, ctype, what):
        """A ctypes array of n `ctype` records from a ctypes array or a sequence of records."""
        if len(records) != n:
            raise ValueError(f"{what}: expected {n} records, got {len(records)}")
        if isinstance(records, C.Array) and records._type_ is ctype:
            return records
        return (ctype * max(n, 1))(*records)

    def _fill_material_update(self, upd, table, keep, materials, textures, lights, background, images):
        if materials is not None:
            arr = self._record_table(materials, self.num_materials, abi.Material, "materials")
            keep.append(arr)
            upd.materials = C.cast(arr, C.POINTER(abi.Material))
        if textures is not None:
            arr = self._record_table(textures, self.num_textures, abi.Texture, "textures")
            keep.append(arr)
            upd.textures = C.cast(arr, C.POINTER(abi.Texture))
        if lights is not None:
            arr = self._record_table(lights, len(lights), abi.Light, "lights")
            keep.append(arr)
            upd.lights = C.cast(arr, C.POINTER(abi.Light))
            upd.num_lights, upd.set_lights = len(lights), 1
        if background is not None:
            bg = abi.Background.from_buffer_copy(background)
            keep.append(bg)
            upd.background = C.pointer(bg)
        if images:
            arr = (abi.TextureImage * len(images))()
            for k, (tex, img) in enumerate(images.items()):
                if tex not in self._image_sizes:
                    raise ValueError(f"images: texture {tex} is not an image texture of the scene")
                h, w = self._image_sizes[tex]
                arr[k].texture = int(tex)
                arr[k].level0 = table(img.reshape(-1, 3) if tuple(img.shape) == (h, w, 3) else img, h * w, 3, f"images[{tex}]")
            keep.append(arr)
            upd.images = C.cast(arr, C.POINTER(abi.TextureImage))
            upd.num_images = len(images)

    def update_materials(self, materials=None, textures=None, lights=None, background=None, images=None, stream=None,
                         vertices=None, normals=None, spheres=None):
        """New materials, texture records, emitters, background and image contents for the resident scene (the
        material fields of vimg_hip_scene_update_geometry); None = unchanged.  ``materials`` / ``textures``: the whole
        tables (abi.Material / abi.Texture records, as HostScene.materials() / .textures() return them);
        ``lights``: a new emitter list of abi.Light, ``[]`` for a scene without emitters; ``background``: an
        abi.Background that keeps type, env_tex and CDF offsets; ``images``: {texture index: [H, W, 3] float32} - a
        CUDA tensor is read where it is, a numpy array is copied up - whose mip chains (and, for the env map, sampling
        CDFs) are rebuilt on the GPU.  Positions (as for update_geometry) may ride in the same call.  Afterwards the
        scene is the upload of the host scene edited the same way; progressive accumulators must be reset."""
        upd = abi.GeometryUpdate()
        c, keep = _Tensors(), []     # the device tables (copies of numpy ones, the caller's tensors), the ctypes tables
        given = {}                   # the position tables of this call, for vertices_given / spheres_given

        def table(a, rows, cols, what):
            return _ptr(c.take(a, what, ("float32",), (rows, cols)))

        for name, a, rows, cols in (("vertices", vertices, self.num_vertices, 3), ("normals", normals, self.num_vertices, 3),
                                    ("spheres", spheres, self.num_spheres, 4)):
            if a is not None:
                t = c.take(a, name, ("float32",), (rows, cols))
                setattr(upd, name, _ptr(t))
                if name != "normals":      # the uploaded copy of a numpy table, a clone of a caller's tensor
                    given[name] = t if isinstance(a, np.ndarray) else t.clone()
        self._fill_material_update(upd, table, keep, materials, textures, lights, background, images)
        self.generation += 1
        with c.launch(stream) as sp:     # (blocking: the tables stay alive until it returns)
            _check(self._lib.vimg_hip_scene_update_geometry(self._h, C.byref(upd), sp))
        self.vertices_given = given.get("vertices", self.vertices_given)
        self.spheres_given = given.get("spheres", self.spheres_given)

    def update_from(self, host_scene, stream=None):
        """The four tables of ``host_scene`` (materials, texture records, emitters, background) as they now stand:
        after HostScene.set_materials / set_texture_colors / set_background on the scene this one was uploaded from.
        Image contents are not read from the host: pass them with update_materials(images=...)."""
        self.update_materials(materials=host_scene.materials(), textures=host_scene.textures(), lights=list(host_scene.lights()),
                              background=host_scene.background(), stream=stream)

    def rebuild_bvh(self, builder="ploc", stream=None):
        """A new tree over the scene's primitives as they now stand (vimg_hip_scene_rebuild_bvh): built by the GPU
        builder ``builder`` ("ploc" or "lbvh") from the resident positions and baked into the device layout by
        kernels.  Afterwards the scene is the upload of the same host scene after build_bvh_with(ploc_builder())
        (or lbvh_builder()).  Blocking; progressive accumulators of the scene must be reset afterwards."""
        if builder not in abi.BUILDERS:
            raise ValueError(f"builder: expected one of {sorted(abi.BUILDERS)}, not {builder!r}")
        opts = abi.RebuildOptions(builder=abi.BUILDERS[builder])
        self.generation += 1
        with _Launch(stream) as sp:
            _check(self._lib.vimg_hip_scene_rebuild_bvh(self._h, C.byref(opts), sp))

    def bvh_cost(self, stream=None):
        """Surface-area cost of the scene's tree under the reference's model (vimg_hip_scene_bvh_cost): it rises
        when update_geometry stretches the tree over moved geometry; rebuild_bvh brings it back."""
        cost = C.c_double()
        with _Launch(stream) as sp:
            _check(self._lib.vimg_hip_scene_bvh_cost(self._h, sp, C.byref(cost)))
        return float(cost.value)

    def set_camera(self, look_from, look_at=None, up=None, vfov_deg=None, aperture_radius=0.0, focal_dist=1.0):
        """A new camera at the scene's resolution (vimg_hip_scene_set_camera): look-at arguments as
        HostScene.set_camera without the resolution, or an abi.Camera.  Progressive accumulators of the scene
        must be reset afterwards."""
        if isinstance(look_from, abi.Camera):
            cam = look_from
        else:
            cam = camera_lookat(look_from, look_at, up, vfov_deg, self.resolution, aperture_radius, focal_dist)
        self.generation += 1
        _check(self._lib.vimg_hip_scene_set_camera(self._h, C.byref(cam)))
        self.camera = abi.Camera.from_buffer_copy(cam)

    # ---- ray queries (vimg_hip_trace_rays, _occluded, _camera_rays) ----------------------------------
    @staticmethod
    def _query(a, cols, what):
        """(the call's _Tensors, the [N, cols] float32 input of a query, 16-byte aligned, N)."""
        c = _Tensors(to_host=isinstance(a, np.ndarray))
        t = c.take(a, what, ("float32",), (None, cols), aligned=True)
        return c, t, t.shape[0]

    def trace_rays(self, rays, info=False, out=None, stream=None):
        """Closest hits of ``rays`` ([N, 8] float32 laid out as VimgRay: org xyz, t_min, dir xyz, t_max) against the
        resident scene (vimg_hip_trace_rays): a RayHits with t [N] (+inf for a miss), prim [N] int32 (-1 for a
        miss), bary [N, 2] (weights of a triangle's 2nd and 3rd vertex), and with ``info`` also p, ns, ng [N, 3],
        uv [N, 2], mat [N] int32.  A CUDA tensor is used as it is and the results are views of device buffers,
        ordered on ``stream`` (torch's current one by default); a numpy array is copied up and numpy arrays come
        back.  ``out``: the [N, 4] float32 hit buffer, or (hits, [N, 12] info buffer) with ``info``."""
        c, r, n = self._query(rays, 8, "rays")
        hits_out, info_out = (out if info and out is not None else (out, None))
        hits = c.output(hits_out, "trace_rays", "float32", (n, 4), aligned=True)
        rec = c.output(info_out, "trace_rays info", "float32", (n, 12), aligned=True) if info else None
        with c.launch(stream) as sp:
            _check(self._lib.vimg_hip_trace_rays(self._h, _ptr(r), n, _ptr(hits), _ptr(rec), sp))
        return RayHits.of(hits, rec, c.to_host)

    def occluded(self, rays, out=None, stream=None):
        """The render's shadow test on ``rays`` ([N, 8] float32, VimgRay; vimg_hip_occluded): bool [N], True when
        anything lies in [t_min, t_max].  CUDA tensor in, CUDA tensor out (a view of ``out``, [N] uint8, when
        given); numpy in, numpy out."""
        import torch
        c, r, n = self._query(rays, 8, "rays")
        flags = c.output(out, "occluded", "uint8", (n,))
        with c.launch(stream) as sp:
            _check(self._lib.vimg_hip_occluded(self._h, _ptr(r), n, _ptr(flags), sp))
        return c.result(flags.view(torch.bool))

    def camera_rays(self, samples, out=None, stream=None):
        """The camera's rays (vimg_hip_camera_rays) for ``samples`` [N, 4] float32 {x, y, lens_u, lens_v} (pixel
        coordinates, lens samples): [N, 8] float32 VimgRay records with t_min 1e-4 and t_max +inf - the input of
        trace_rays for picking.  CUDA tensor in, CUDA tensor out; numpy in, numpy out."""
        c, smp, n = self._query(samples, 4, "samples")
        rays = c.output(out, "camera_rays", "float32", (n, 8), aligned=True)
        with c.launch(stream) as sp:
            _check(self._lib.vimg_hip_camera_rays(self._h, _ptr(smp), n, _ptr(rays), sp))
        return c.result(rays)

    def progressive(self, params):
        """An accumulator for this frame (or shard) rendered a few samples at a time (vimg_hip_progressive_*):
        after increments n_1 .. n_k the image is bit for bit ``render`` at n_1 + .. + n_k samples.
        ``params.samples`` is ignored; the other fields are fixed for the accumulator's life."""
        return Progressive(self, params)

    def render_async(self, params, out, stream=None):
        with _Launch(stream, used=[out]) as sp:
            _check(self._lib.vimg_hip_render_async(self._h, C.byref(params),
                                                   C.c_void_p(out.data_ptr()), sp))

    def check(self):
        """After render_async and a synchronisation of its stream: raises HipError when a launch of this
        scene gave its frame up (the kernel's watchdog), before the frame is used, gathered or timed."""
        _check(self._lib.vimg_hip_check(self._h))

    def render_to_host(self, params, stats=True):
        """Render and copy the framebuffer to a numpy array [H, W, 3] (no torch needed)."""
        w, h = self.resolution
        out = np.empty((h, w, 3), dtype=np.float32)
        st = abi.RenderStats()
        _check(self._lib.vimg_hip_render_to_host(self._h, C.byref(params),
                                                 out.ctypes.data_as(abi.Pf32),
                                                 C.byref(st) if stats else None))
        return (out, st) if stats else out

    def render_heatmap(self, params, factor=-1.0, out=None, stream=None):
        """BVH traversal-cost picture (reference heatmap_img) into a torch CUDA tensor [H, W, 3]
        (or the compact shard slab when params.tile_world > 1)."""
        c = _Tensors()
        out = c.own(self._new_output(params, zero_slab=False)) if out is None else c.use(out)
        with c.launch(stream) as sp:
            _check(self._lib.vimg_hip_render_heatmap(self._h, C.byref(params), factor,
                                                     C.c_void_p(out.data_ptr()), sp))
        return out

    def trace_pixel(self, params, x, y):
        out = np.zeros(3, dtype=np.float32)
        _check(self._lib.vimg_hip_trace_pixel(self._h, C.byref(params), x, y,
                                              out.ctypes.data_as(abi.Pf32)))
        return out

    def assemble_shards(self, gathered, world, shard_stride_pixels, out=None, stream=None):
        import torch
        w, h = self.resolution
        c = _Tensors()
        out = c.own(torch.empty((h, w, 3), dtype=torch.float32, device="cuda")) if out is None else c.use(out)
        c.use(gathered)
        with c.launch(stream) as sp:
            _check(self._lib.vimg_hip_assemble_shards(self._h, world, shard_stride_pixels,
                                                      C.c_void_p(gathered.data_ptr()),
                                                      C.c_void_p(out.data_ptr()), sp))
        return out

    def time_renders(self, params, out, steps):
        ms = np.zeros(steps, dtype=np.float32)
        _check(self._lib.vimg_hip_time_renders(self._h, C.byref(params),
                                               C.c_void_p(out.data_ptr()), steps,
                                               ms.ctypes.data_as(abi.Pf32)))
        return ms

    def probe(self, kind, inputs):
        """Unit-level test hook (vimg_hip_probe): per item n_in floats in, n_out floats out."""
        n_in, n_out = PROBE_IO[kind]
        a = np.ascontiguousarray(inputs, dtype=np.float32).reshape(-1, n_in)
        out = np.zeros((a.shape[0], n_out), dtype=np.float32)
        _check(self._lib.vimg_hip_probe(self._h, kind, a.shape[0], a.ctypes.data_as(abi.Pf32), out.ctypes.data_as(abi.Pf32)))
        return out

    def close(self):
        if self._h:
            self._lib.vimg_hip_scene_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GuideCache:
    """Feature frames of a resident scene, rendered once and kept until the scene is edited: ``get`` renders the frames
    ``names`` of ``params`` at ``samples`` samples (render_features' dict) when (DeviceScene.generation, samples, names)
    is not what ``held`` - (key, frames), or None: nothing, set it to drop them - was rendered from.  One per owner."""

    def __init__(self, dev):
        self._dev, self.held = dev, None

    def get(self, params, samples, names, stream=None):
        key = (self._dev.generation, int(samples), tuple(names))
        if self.held is None or self.held[0] != key:
            p = abi.RenderParams.from_buffer_copy(params)
            p.samples = int(samples)
            self.held = (key, self._dev.render_features(p, names, stream=stream))
        return self.held[1]


class RayHits:
    """Result of DeviceScene.trace_rays: t [N], prim [N] int32 (-1 = miss), bary [N, 2]; with info also p, ns, ng
    [N, 3], uv [N, 2], mat [N] int32 (zeros for a miss).  Views of the device buffers (torch) or numpy arrays."""
    FIELDS = ("t", "prim", "bary", "p", "ns", "ng", "uv", "mat")

    def __init__(self, **kw):
        for k in self.FIELDS:
            setattr(self, k, kw.get(k))

    @classmethod
    def of(cls, hits, info, host):
        import torch
        if host:
            hits = hits.cpu().numpy()
            info = None if info is None else info.cpu().numpy()
            as_i32 = lambda a: a.view(np.int32)
        else:
            as_i32 = lambda a: a.view(torch.int32)
        f = dict(t=hits[:, 0], prim=as_i32(hits)[:, 1], bary=hits[:, 2:4])
        if info is not None:
            f.update(p=info[:, 0:3], ns=info[:, 3:6], ng=info[:, 6:9], uv=info[:, 9:11], mat=as_i32(info)[:, 11])
        return cls(**f)

    def __repr__(self):
        return f"RayHits(n={len(self.t)}, info={self.p is not None})"


class Progressive:
    """A frame of one DeviceScene rendered in increments (DeviceScene.progressive).  Every call is ordered
    on torch's stream the way DeviceScene.render is."""

    def __init__(self, dev, params):
        self._lib = dev._lib
        self._dev = dev              # (keeps the scene alive while the accumulator is)
        self.params = abi.RenderParams.from_buffer_copy(params)
        h = C.c_void_p()
        _check(self._lib.vimg_hip_progressive_create(dev._h, C.byref(self.params), C.byref(h)))
        self._h = h
        self._guide_cache = GuideCache(dev)
        self._sparse_calls = 0       # render_sparse calls since creation or the last reset: the next lattice phase

    @property
    def _guides(self):           # (key, the four feature frames) of the last preview, or None
        return self._guide_cache.held

    def _handle(self):
        if not self._h:
            raise HipError("progressive accumulator used after close()")
        return self._h

    @property
    def samples(self):
        """Samples per pixel so far (after masked increments: the largest count of any pixel)."""
        return int(self._lib.vimg_hip_progressive_samples(self._handle()))

    @property
    def launches(self):
        """Render launches of the successful increments since creation or the last reset."""
        return int(self._lib.vimg_hip_progressive_launches(self._handle()))

    @property
    def pixel_shape(self):
        """Shape of a per-pixel buffer of this accumulator: (H, W), or (shard_pixels,) when tile_world > 1."""
        w, ht = self._dev.resolution
        return (ht, w) if self.params.tile_world == 1 else (self._dev.shard_pixels(self.params),)

    def render(self, samples, out=None, stats=False, stream=None, mask=None):
        """Adds `samples` samples per pixel and returns the running mean in ``DeviceScene.render``'s shapes
        ([H, W, 3], or the shard's compact [shard_pixels, 3] when tile_world > 1), with this increment's
        RenderStats when ``stats``.  ``out=False``: advance only, nothing is written or returned but the stats.
        ``mask`` (uint8 or bool, ``pixel_shape``; CUDA tensor or numpy array): only the pixels whose entry is
        non-zero get the samples (vimg_hip_progressive_render_masked); every pixel's mean is returned, each
        bit for bit ``DeviceScene.render`` at that pixel's own count."""
        h = self._handle()
        c = _Tensors()
        if out is None:
            out = c.own(self._dev._new_output(self.params))
        elif out is not False:
            c.use(out)
        if mask is not None:
            m = c.take(mask, "mask", ("uint8", "bool"), self.pixel_shape)
        st = abi.RenderStats()
        with c.launch(stream) as sp:
            _check(self._lib.vimg_hip_progressive_render_masked(self._dev._h, h, int(samples),
                                                                None if mask is None else C.c_void_p(m.data_ptr()),
                                                                None if out is False else C.c_void_p(out.data_ptr()), sp,
                                                                C.byref(st) if stats else None))
        img = None if out is False else out
        return (img, st) if stats else img

    def preview(self, samples, out=None, stream=None, feature_samples=4, variance_guided=False, despeckle=None, **filter_kw):
        """``render(samples)`` followed by the a-trous filter (vimg_amd.filter.atrous) on the running mean: the
        denoised picture of the frame so far.  The accumulator is advanced exactly as by ``render`` and keeps the
        unfiltered sums, so later increments and renders give the bits they would have given.  The guides -
        render_features(("albedo", "normal", "position", "depth")) at ``feature_samples`` samples - do not depend on
        the increments: they are rendered once and kept until the scene is edited (DeviceScene.generation).
        Whole frames only.  ``filter_kw``: the parameters of filter.atrous.  ``variance_guided``: render(samples) +
        ``variance()`` + the variance-guided filter (vimg_amd.varfilter.atrous, ``filter_kw`` its parameters) on the
        same guides - each pixel is filtered by its own noise, whatever its count.  ``despeckle`` (True: the library's
        defaults; a dict: its parameters; None or False: no call): the fireflies of the running mean ``render``
        returned - a frame of its own, the sums are not touched - are clamped (vimg_amd.despeckle.clamp,
        include/vimg_despeckle.h) before the filter."""
        from . import preview
        if self.params.tile_world != 1:
            raise ValueError("preview: the filter reads whole frames, not shards (tile_world must be 1)")
        clamp = preview.despeckle_kw(despeckle, "preview")
        noisy = self.render(samples, stream=stream)
        g = self._guide_cache.get(self.params, feature_samples, preview.GUIDES, stream=stream)
        preview.clamp_fireflies(noisy, g, clamp, stream=stream)
        return preview.denoise(noisy, g, variance_guided, variance=self.variance(stream) if variance_guided else None, out=out,
                               stream=stream, **filter_kw)

    def render_sparse(self, samples, stride=2, radius=None, out=None, stream=None, feature_samples=4, **infill_kw):
        """``samples`` more samples for ONE pixel in stride^2 - the lattice infill.lattice_mask(H, W, stride, phase)
        with phase = (calls since creation or reset) % stride^2 - and the picture with the other pixels filled from
        the feature frames (vimg_amd.infill.reconstruct on the guides ``preview`` keeps, and ``counts()``).  The
        pixels of one lattice stand at one count, so each call is one render launch; after stride^2 calls every pixel
        has had ``samples`` more and the picture is ``render``'s bit for bit.  The accumulator keeps the plain sums:
        later increments and renders give the bits they would have given.  ``radius``: the reach of the fill, default
        ``stride``; ``infill_kw``: the other parameters of infill.reconstruct.  Keep to one ``stride`` between resets.
        Returns the [H, W, 3] image (``out`` when given); whole frames only."""
        import torch
        from . import infill
        if self.params.tile_world != 1:
            raise ValueError("render_sparse: the fill reads whole frames, not shards (tile_world must be 1)")
        stride = int(stride)
        h, w = self.pixel_shape
        with torch.cuda.stream(stream):          # (the mask is filled where the increment reads it)
            mask = infill.lattice_mask(h, w, stride, self._sparse_calls % (stride * stride))
        noisy = self.render(samples, stream=stream, mask=mask)
        self._sparse_calls += 1
        g = self._guide_cache.get(self.params, feature_samples, infill.GUIDES, stream=stream)
        return infill.reconstruct(noisy, g["normal"], g["position"], g["depth"], self.counts(stream), albedo=g["albedo"],
                                  radius=stride if radius is None else radius, out=out, stream=stream, **infill_kw)[0]

    def state(self, stream=None):
        """The per-pixel records (vimg_hip_progressive_state) as CUDA tensors in ``pixel_shape``: a dict with
        ``sum`` [.., 3] float32 (running sums), ``count`` int64 N, ``batches`` int64 K (increments the pixel
        took part in; both are uint32 in the library, widened here because torch has no such type) and ``m2``
        float32."""
        return self._read_state(("sum", "count", "batches", "m2"), stream)

    def _read_state(self, fields, stream):
        """The `fields` of the pixel records, one launch of vimg_hip_progressive_state; the two uint32 ones widened."""
        import torch
        h = self._handle()
        shp = self.pixel_shape
        t = {k: torch.zeros(shp + ((3,) if k == "sum" else ()), dtype=torch.float32 if k in ("sum", "m2") else torch.int32,
                            device="cuda") for k in fields}
        launch = _Launch(stream, made=list(t.values()))
        with launch as sp:
            _check(self._lib.vimg_hip_progressive_state(h, *(_ptr(t.get(k)) for k in ("sum", "count", "batches", "m2")), sp))
        with torch.cuda.stream(launch.cur if launch.home is not None else None):   # (the launch only enqueues: widen where it runs)
            for k in t.keys() & {"count", "batches"}:
                t[k] = t[k].to(torch.int64) & 0xFFFFFFFF
        return t

    def counts(self, stream=None):
        """Samples each pixel has had: int64 CUDA tensor in ``pixel_shape`` (uint32 in the library)."""
        return self._read_state(("count",), stream)["count"]

    def error(self, stream=None):
        """Estimated relative standard error of each pixel's mean luminance (vimg_hip_progressive_error): float32
        CUDA tensor in ``pixel_shape``, +inf for pixels that took part in fewer than two increments."""
        import torch
        h = self._handle()
        e = torch.zeros(self.pixel_shape, dtype=torch.float32, device="cuda")
        with _Launch(stream, made=[e]) as sp:
            _check(self._lib.vimg_hip_progressive_error(h, C.c_void_p(e.data_ptr()), sp))
        return e

    def variance(self, stream=None):
        """Estimated variance of each pixel's mean luminance (vimg_varfilter_variance of the records): [H, W] float32
        CUDA tensor, NaN for pixels that took part in fewer than two increments - the quantity under the square root
        of ``error()``, and what vimg_amd.varfilter.atrous takes as ``variance``.  Whole frames only."""
        import torch
        from . import varfilter
        h = self._handle()
        if self.params.tile_world != 1:
            raise ValueError("variance: the variance frame is a whole frame's, not a shard's (tile_world must be 1)")
        # the library's own uint32 buffers (as int32: the same bits), not _read_state's widened ones
        n, k = (torch.zeros(self.pixel_shape, dtype=torch.int32, device="cuda") for _ in range(2))
        m2 = torch.zeros(self.pixel_shape, dtype=torch.float32, device="cuda")
        with _Launch(stream, made=[n, k, m2]) as sp:
            _check(self._lib.vimg_hip_progressive_state(h, None, _ptr(n), _ptr(k), _ptr(m2), sp))
        return varfilter.variance(n, k, m2, out=m2, stream=stream)

    def select(self, target, max_samples, out=None, stream=None):
        """(mask, active): the uint8 mask of the pixels that still need samples - error above ``target`` and count
        below ``max_samples``, or fewer than two increments so far - and how many there are
        (vimg_hip_progressive_select)."""
        import torch
        h = self._handle()
        c = _Tensors()
        if out is None:
            out = c.own(torch.zeros(self.pixel_shape, dtype=torch.uint8, device="cuda"))
        else:
            out = c.take(out, "mask", ("uint8", "bool"), self.pixel_shape)
        n = abi.u32(0)
        with c.launch(stream) as sp:
            _check(self._lib.vimg_hip_progressive_select(h, float(target), int(max_samples), C.c_void_p(out.data_ptr()), sp,
                                                         C.byref(n)))
        return out, int(n.value)

    def render_adaptive(self, target, step, max_samples, min_samples=None, out=None, stream=None, progress=None):
        """Samples until every pixel's error is at most ``target`` or its count is ``max_samples``: unmasked
        increments of ``step`` up to ``min_samples`` (default 2 * step), then select -> masked increment of
        ``step`` until no pixel is active.  A pixel that drops out stays out, so the active pixels all stand at
        one count and every step is one launch.  ``max_samples`` and ``min_samples`` must be multiples of
        ``step``, min_samples >= 2 * step (the error needs two increments).  Returns the image; ``counts()``
        tells what each pixel got.  ``progress(samples, active)`` is called after every step."""
        step, max_samples = int(step), int(max_samples)
        min_samples = 2 * step if min_samples is None else int(min_samples)
        if step <= 0 or min_samples < 2 * step or min_samples % step or max_samples % step or max_samples < min_samples:
            raise ValueError("render_adaptive: step > 0, min_samples and max_samples multiples of step, "
                             "2 * step <= min_samples <= max_samples")
        if not target >= 0:
            raise ValueError("render_adaptive: target must be >= 0")
        if out is None:
            out = self._dev._new_output(self.params)
        wrote = False
        while self.samples < min_samples:
            self.render(step, out=out, stream=stream)
            wrote = True
            if progress:
                progress(self.samples, int(np.prod(self.pixel_shape)))
        mask = None
        while True:
            mask, active = self.select(target, max_samples, out=mask, stream=stream)
            if active == 0:
                break
            self.render(step, out=out, stream=stream, mask=mask)
            wrote = True
            if progress:
                progress(self.samples, active)
        if not wrote:     # nothing left to do: the all-zero mask renders nothing and writes every pixel's mean
            self.render(step, out=out, stream=stream, mask=mask)
        return out

    def reset(self, stream=None):
        """Back to 0 samples: the next increment seeds every pixel again."""
        h = self._handle()
        with _Launch(stream):
            _check(self._lib.vimg_hip_progressive_reset(h))
        self._sparse_calls = 0

    def close(self):
        if self._h:
            self._lib.vimg_hip_progressive_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def post_rgb8(image, tonemapper=1, stream=None):
    """Tonemap (0 clamp, 1 AgX, 2 Reinhard, 3 ACES) + sRGB + 8-bit quantise a [H, W, 3] float32 frame on the GPU
    (vimg_hip_post_rgb8): a contiguous CUDA tensor on the current device gives a [H, W, 3] uint8 CUDA tensor, a numpy
    frame is copied up and its bytes come back as numpy."""
    import torch
    if isinstance(tonemapper, bool) or not isinstance(tonemapper, (int, np.integer)) or not 0 <= tonemapper <= 3:
        raise ValueError(f"post_rgb8: tonemapper must be 0 (clamp), 1 (AgX), 2 (Reinhard) or 3 (ACES), not {tonemapper!r}")
    shape = getattr(image, "shape", None)
    if shape is None or len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"post_rgb8 image: shape must be (H, W, 3), not {None if shape is None else tuple(shape)}")
    h, w = int(shape[0]), int(shape[1])
    ts = _Tensors(to_host=not isinstance(image, torch.Tensor))
    frame = ts.take(image, "post_rgb8 image", ("float32",), (h, w, 3))
    out = ts.output(None, "post_rgb8 out", "uint8", (h, w, 3))
    with ts.launch(stream) as sp:
        _check(_lib().vimg_hip_post_rgb8(_ptr(frame), w, h, int(tonemapper), _ptr(out), sp))
    return ts.result(out)


__all__ = ["DeviceScene", "Progressive", "RayHits", "post_rgb8", "HipError", "device_count", "init", "make_params"]


# ---- the pre-step of the path on the GPU (include/vimg_hip.h) ----------
def build_mip_chain(level0, wrap_u=abi.WRAP_REPEAT, wrap_v=abi.WRAP_REPEAT):
    """All mip levels of an [H, W, 3] float image, level 0 first: (flat [texels, 3] array,
    list of per-level (offset_in_texels, w, h))."""
    lib = abi.hip_lib()
    img = np.ascontiguousarray(level0, dtype=np.float32)
    h, w = img.shape[:2]
    n_levels = abi.u32(0)
    texels = int(lib.vimg_hip_mip_chain_texels(w, h, C.byref(n_levels)))
    out = np.empty((texels, 3), dtype=np.float32)
    _check(lib.vimg_hip_build_mip_chain(w, h, img.ctypes.data_as(abi.Pf32), wrap_u, wrap_v,
                                        out.ctypes.data_as(abi.Pf32)))
    levels, off, lw, lh = [], 0, w, h
    for _ in range(n_levels.value):
        levels.append((off, lw, lh))
        off += lw * lh
        lw, lh = max(lw // 2, 1), max(lh // 2, 1)
    return out, levels


def build_env_cdfs(img):
    """(row_cdf [H+1], col_cdfs [H, W+1]) of a lat-long [H, W, 3] float image."""
    lib = abi.hip_lib()
    a = np.ascontiguousarray(img, dtype=np.float32)
    h, w = a.shape[:2]
    row = np.empty(h + 1, dtype=np.float32)
    col = np.empty((h, w + 1), dtype=np.float32)
    _check(lib.vimg_hip_build_env_cdfs(a.ctypes.data_as(abi.Pf32), w, h, row.ctypes.data_as(abi.Pf32),
                                       col.ctypes.data_as(abi.Pf32)))
    return row, col


def lut8_to_float(values_u8, lut256):
    lib = abi.hip_lib()
    a = np.ascontiguousarray(values_u8, dtype=np.uint8)
    lut = np.ascontiguousarray(lut256, dtype=np.float32)
    assert lut.size == 256
    out = np.empty(a.shape, dtype=np.float32)
    _check(lib.vimg_hip_lut8_to_float(a.ctypes.data_as(C.POINTER(C.c_uint8)), a.size,
                                      lut.ctypes.data_as(abi.Pf32), out.ctypes.data_as(abi.Pf32)))
    return out


def rgb8_to_normal(rgb8, scale=1.0):
    lib = abi.hip_lib()
    a = np.ascontiguousarray(rgb8, dtype=np.uint8)
    assert a.shape[-1] == 3
    out = np.empty(a.shape, dtype=np.float32)
    _check(lib.vimg_hip_rgb8_to_normal(a.ctypes.data_as(C.POINTER(C.c_uint8)), a.size // 3, scale,
                                       out.ctypes.data_as(abi.Pf32)))
    return out


def install_gpu_precompute(enable=True):
    """Make libvimg_host build mip chains and env-map CDFs with the GPU kernels (or, with
    enable=False, with its own loops again)."""
    host = abi.host_lib()
    if not enable:
        host.vimg_host_set_precompute(None, None)
        return
    lib = abi.hip_lib()
    host.vimg_host_set_precompute(C.cast(lib.vimg_hip_build_mip_chain, C.c_void_p),
                                  C.cast(lib.vimg_hip_build_env_cdfs, C.c_void_p))


def lbvh_builder():
    """Function pointer of the GPU LBVH builder for HostScene.build_bvh_with()."""
    return C.cast(abi.hip_lib().vimg_hip_build_lbvh, C.c_void_p)


def ploc_builder():
    """Function pointer of the GPU PLOC + SAH-leaf builder for HostScene.build_bvh_with()."""
    return C.cast(abi.hip_lib().vimg_hip_build_ploc, C.c_void_p)
