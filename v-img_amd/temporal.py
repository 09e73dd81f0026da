"""Temporal accumulation over frames in device memory: ctypes mirror of include/vimg_temporal.h
(libvimg_temporal.so, gfx950).

The third scene-free library: the last preview is reprojected into a moved camera by the `position`
frame and blended with the current frame where normal and position say it is the same surface.  The binding shares the
render binding's tensor check and stream rule (hip.FrameCall: hip._device_tensor, hip._Launch).  There is no CPU
fallback.
"""
import ctypes as C
import math

import numpy as np

from . import _abi as abi
from .hip import FrameCall, FrameHistory, GuideCache, _checker, library_params

FRAMES = ("color", "normal", "position", "depth")
PARAMS = ("max_history", "current_weight", "sigma_normal", "sigma_plane")


_lib = abi.temporal_lib
_check = _checker(_lib, "vimg_temporal_last_error")


def temporal_params(max_history=None, current_weight=None, sigma_normal=None, sigma_plane=None):
    """An abi.TemporalParams: the library's defaults (vimg_temporal_defaults; include/vimg_temporal.h names them) with
    the given values in place of them."""
    return _params(zip(PARAMS, (max_history, current_weight, sigma_normal, sigma_plane)))


def _params(given):
    return library_params("temporal", abi.TemporalParams, _lib().vimg_temporal_defaults, PARAMS, given)


def history_bytes(width, height):
    return int(_lib().vimg_temporal_history_bytes(width, height))


def world_to_pixel(camera):
    """The 12 float32 of vimg_temporal_accumulate's matrix (row-major 3 x 4) for an abi.Camera: a world-space point
    goes to (hx, hy, hw) with column hx / hw and row hy / hw in FRAME ARRAY coordinates - column = the renderer's
    sample x, row = res_y - sample y, because vimg_hip_render stores sample row y at array row H - 1 - y.  The pinhole
    through the lens centre (with aperture_radius > 0 this is the mapping of the lens centre), the inverse of the
    rigid cam_to_world, the image plane of the reference's TLCam (height 2 tan(vfov / 2), width ratio times that, rays
    along -z).  Computed in float64 and rounded once."""
    c2w = np.array(list(camera.cam_to_world), dtype=np.float64).reshape(4, 4).T      # glm column-major
    rot, org = c2w[:3, :3], c2w[:3, 3]
    w2c = np.concatenate([rot.T, -(rot.T @ org)[:, None]], axis=1)                    # camera-space point = w2c [P; 1]
    w, h = float(camera.res_x), float(camera.res_y)
    ph = 2.0 * math.tan(math.radians(float(camera.vfov_deg)) / 2.0)
    pw = (w / h) * ph
    m = np.stack([(w / pw) * w2c[0] - (w / 2.0) * w2c[2],        # sample x = w (x_dir / pw + 1/2),  x_dir = Pc.x / -Pc.z
                  -(h / ph) * w2c[1] - (h / 2.0) * w2c[2],       # row = h - sample y = h (1/2 - y_dir / ph)
                  -w2c[2]])
    return m.astype(np.float32).reshape(12)


class History(FrameHistory):
    """One history of vimg_temporal_accumulate: ``tensor`` [3, H, W, 4] float32 (planes A = {rgb, length},
    G0 = {normal, depth}, G1 = {position, 0}; a CUDA tensor, or a numpy array after a call with numpy frames) and
    ``world_to_pixel``, the matrix of the camera its frame was rendered under (None: unknown, the history cannot be
    reprojected).  ``color`` [H, W, 3] and ``length`` [H, W] are views."""
    PLANES = 3


def accumulate(color, normal, position, depth, history=None, world_to_pixel=None, out=None, next_history=None, stream=None,
               **params):
    """One step of temporal accumulation (vimg_temporal_accumulate): the current ``color`` frame with its first-hit
    frames ``normal``, ``position``, ``depth`` - all [H, W, 3] float32, as DeviceScene.render and render_features
    return them - blended with ``history``, the History of the frame before (None: no history), which is looked up
    where ``history.world_to_pixel`` sends each pixel's position.  Returns the next History; ``world_to_pixel`` is the
    matrix of the CURRENT camera (temporal.world_to_pixel(camera)), which the result remembers for the next step.
    CUDA tensors are read where they are; numpy arrays are copied up, and with a numpy ``color`` the History holds a
    numpy array.  ``out``: a [H, W, 3] float32 CUDA tensor that gets the accumulated colour as packed triples, which
    may be ``color`` itself; ``next_history``: the [3, H, W, 4] float32 CUDA tensor to write (not the one ``history``
    holds), allocated when None.  ``params``: max_history, current_weight, sigma_normal, sigma_plane, default the
    library's (include/vimg_temporal.h).  The call only enqueues, on ``stream`` or torch's current stream."""
    c = FrameCall("temporal", color)
    h, w = c.h, c.w
    p = _params(params.items())
    t = c.frames(FRAMES, (color, normal, position, depth))
    prev, matrix = c.history(history, History)
    next_history = c.output(next_history, "temporal next_history", "float32", (3, h, w, 4), aligned=True)
    if out is not None:
        c.output(out, "temporal", "float32", (h, w, 3))
    frames = abi.TemporalFrames(width=w, height=h, **{k: v.data_ptr() for k, v in t.items()})
    with c.launch(stream) as sp:
        _check(_lib().vimg_temporal_accumulate(C.byref(frames), None if prev is None else C.c_void_p(prev.data_ptr()), matrix,
                                               C.byref(p), C.c_void_p(next_history.data_ptr()),
                                               None if out is None else C.c_void_p(out.data_ptr()), sp))
    return History(c.result(next_history), world_to_pixel)


class TemporalPreview:
    """The preview of a resident scene whose camera moves (DeviceScene.temporal_preview): one Progressive, two history
    buffers and the a-trous workspace.  ``frame()`` returns the [H, W, 3] preview of the scene as it now stands.

    When the scene changed since the last frame (DeviceScene.generation: set_camera, update_*, rebuild_bvh) the
    accumulator is reset, the guides are rendered again, ``samples`` samples are rendered and blended with the last
    frame's history, reprojected by the last camera's matrix, at current_weight 1.  When nothing changed the
    accumulator goes on - it stays bit for bit what a Progressive alone would hold - and the running mean of its k
    increments is blended, at current_weight k, with the history frozen at the last change: the picture converges to
    the plain progressive image without a pop.  With ``denoise`` the a-trous filter runs on the accumulated colour for
    the output only; the history keeps unfiltered radiance.  The filter's sigma_color (``filter_kw``'s, or the filter
    library's default) is divided by sqrt(n), n = the frames accumulated since the last reset(), at most max_history:
    its colour term measures colour differences against the noise it expects, and the noise of n accumulated frames is
    1 / sqrt(n) of one frame's, so the filter does less as the history does more (the first frame is filtered as
    Progressive.preview filters it).  It is one factor for the picture: pixels that have just started over are filtered
    as lightly as the rest.  ``scale_sigma_color=False`` passes sigma_color as it is.

    ``variance_guided`` (with ``denoise``) lifts that limit: the histories carry the moments of luminance
    (vimg_amd.moments, include/vimg_moments.h; ``temporal_kw`` then takes min_history too), a frame is acc.render,
    acc.variance() once this camera position has had two increments (else no variance frame), moments.accumulate and
    varfilter.atrous on the accumulated colour with the variance the moments give - NaN where the history is shorter
    than min_history, which the filter estimates from the pixel's surroundings.  ``filter_kw`` are then
    varfilter.atrous's parameters, ``scale_sigma_color`` is refused, and ``history`` is a moments.History.  The
    accumulated colour, the history lengths and the accumulator are bit for bit what they are without it.

    ``sparse`` (a stride 2..4): a frame samples ONE pixel in sparse^2 and the history supplies the
    rest.  A frame() is then: the lattice infill.lattice_mask(H, W, sparse, phase) with phase = (frames since reset())
    mod sparse^2 - a camera change does not restart it, so a moving camera still visits every cell - one
    acc.render(samples, mask=lattice), infill.reconstruct with acc.counts(), the cached guides, the albedo and
    radius = sparse, wtemporal.sparse_weights (a pixel with samples weighs its increments, a filled one
    ``fill_weight``, default wtemporal.FILL_WEIGHT, a fallback or a hole 0) and wtemporal.accumulate
    (include/vimg_wtemporal.h) in place of accumulate: a sampled pixel blends as ever, a filled pixel takes its
    reprojected history where it has one, and the fill is used only where the history has nothing.  After sparse^2
    frames of a standing camera the accumulator is bit for bit a Progressive after one render(samples).  ``history``
    stays a History; ``variance_guided`` is refused with it (the moments history is not weighted per pixel).

    ``antilag`` (True: the library's defaults; a dict: antilag.rescale's parameters): on the frame()
    on which the scene had changed and a history freezes, that frozen history's lengths are rescaled once
    (vimg_amd.antilag, include/vimg_antilag.h) - after this camera's first increment is rendered (with ``sparse``:
    rendered and filled) and before it is accumulated, against that increment and under the current camera's matrix:
    where the new picture disagrees with the history by more than its noise the lengths are cut, to 0 where it clearly
    does, and accumulate's taps there find a short history or none; everywhere else they find what they found before.
    ``last_scale`` is the [H, W] scale frame of the last such call, in the frozen history's pixel coordinates (None
    before the first).  Standing frames make no call and the accumulator stays bit for bit a Progressive.  With
    ``variance_guided`` only plane A's lengths are rescaled, NOT the moments of plane M: a scaled length below
    min_history makes the variance NaN there, which the filter estimates from the pixel's surroundings.

    ``motion`` (the HostScene the DeviceScene was uploaded from, whose positions must be the resident ones at this
    moment; it is read once, here, for motion.SceneTables): a history is reprojected THROUGH the
    displacement of moved geometry.  On a frame() on which the scene had changed and a history freezes, the positions
    DeviceScene.update_geometry / update_materials were last given are compared, as objects, with those of the frozen
    history's frame - two updates between two frames are one displacement.  If neither table changed (set_camera, a
    material edit, rebuild_bvh) no motion call is made and the frame is what it is without ``motion``, bit for bit.
    Otherwise camera_rays(motion.centre_samples) (kept per camera) and trace_rays give every pixel's centre hit on the
    scene as it now stands, and motion.previous_position (vimg_amd.motion, include/vimg_motion.h) gives Q, where each
    pixel's surface point was; Q is kept until the next change, for the standing frames that blend
    against the same frozen history.  The accumulate call - accumulate, moments.accumulate or wtemporal.accumulate,
    unchanged - gets Q as its position frame, and right after it plane G1 of the history it wrote is set back to the
    current position frame, so the next frame finds the current world there; where nothing moved Q is the position
    frame's bits and that copy writes what stands there.  The filter, the infill and antilag.rescale keep the current
    position frame.  ``last_motion_code`` is the [H, W] uint8 code frame of the last motion call (None before the
    first).  ``antilag`` goes with ``motion`` unchanged: it projects the HISTORY's positions under the current camera,
    so its pairs on a moved object fail its same-surface test and such pixels neither trigger nor are cut; the
    object's old shadow on static surfaces still is.

    Limits: without ``antilag``, history from before a material edit is reprojected all the same and fades at
    1 / max_history per frame (``reset()`` drops all of it), and so is history from before a geometry edit, which
    without ``motion`` is moreover looked up where the surface now is, not where it was; with ``antilag``, a change
    smaller than the noise of one increment over the test's window is not seen and fades as before; a thin lens is
    treated as its pinhole; see include/vimg_temporal.h.  With ``motion``: normals are taken as the current ones - a
    rotation by theta per frame passes the same-surface test while 1 - cos(theta) < sigma_normal, about 25 degrees at
    the default 0.1; the displacement is that of the pixel-CENTRE hit, applied to an antialiased mean, so silhouette
    pixels mostly start over, as they already do; the default sigma_plane rejects the neighbouring taps of strongly
    curved surfaces at low resolution whether or not they move; shading is still reprojected radiance - a moved
    object's lighting lags as any edit's does."""

    def __init__(self, dev, params, samples=4, denoise=True, feature_samples=4, filter_kw=None, scale_sigma_color=None,
                 variance_guided=False, sparse=None, fill_weight=None, antilag=False, motion=None, **temporal_kw):
        import torch
        from . import filter as flt
        if params.tile_world != 1:
            raise ValueError("temporal_preview: reprojection reads whole frames, not shards (tile_world must be 1)")
        if int(samples) < 1 or int(feature_samples) < 1:
            raise ValueError("temporal_preview: samples and feature_samples must be at least 1")
        self.variance_guided = bool(variance_guided)
        if self.variance_guided and not denoise:
            raise ValueError("temporal_preview: variance_guided chooses the filter, so it needs denoise=True")
        if self.variance_guided and scale_sigma_color is not None:
            raise ValueError("temporal_preview: scale_sigma_color belongs to the fixed filter; the variance-guided filter has no "
                             "sigma_color")
        self.sparse, self.fill_weight = None, None
        if sparse is not None:
            from . import infill, wtemporal
            if self.variance_guided:
                raise ValueError("temporal_preview: sparse does not go with variance_guided: the moments history has no "
                                 "per-pixel weights")
            infill.lattice_cell(sparse, 0)           # (refuses a stride outside 2..4)
            self.sparse = int(sparse)
            self.fill_weight = wtemporal.FILL_WEIGHT if fill_weight is None else float(fill_weight)
            if not self.fill_weight >= 0.0:
                raise ValueError(f"temporal_preview: fill_weight must be >= 0, not {fill_weight}")
        elif fill_weight is not None:
            raise ValueError("temporal_preview: fill_weight is the weight of a filled pixel: it needs sparse")
        unknown = sorted(set(temporal_kw) - {"max_history", "sigma_normal", "sigma_plane"} - ({"min_history"} if variance_guided else set()))
        if unknown:
            raise TypeError(f"temporal_preview: unknown parameters {unknown}")
        self._dev, self.samples, self.denoise, self.feature_samples = dev, int(samples), bool(denoise), int(feature_samples)
        self.temporal_kw, self.filter_kw = dict(temporal_kw), dict(filter_kw or {})
        self.scale_sigma_color = scale_sigma_color is None or bool(scale_sigma_color)
        self.acc = dev.progressive(params)
        w, h = dev.resolution
        self._buffers = [torch.empty((4 if self.variance_guided else 3, h, w, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
        self._features = flt.GUIDES if denoise or self.sparse else ("normal", "position", "depth")
        if self.sparse:
            from . import infill
            self._infill_workspace = torch.empty((infill.workspace_bytes(w, h),), dtype=torch.uint8, device="cuda")
        if self.variance_guided:
            from . import varfilter
            self._workspace = torch.empty((varfilter.workspace_bytes(w, h),), dtype=torch.uint8, device="cuda")
            self._variance = torch.empty((h, w), dtype=torch.float32, device="cuda")
            self._sigma_color = None
        else:
            self._workspace = torch.empty((flt.atrous_workspace_bytes(w, h),), dtype=torch.uint8, device="cuda") if denoise else None
            self._sigma_color = float(self.filter_kw.pop("sigma_color", None) or flt.atrous_params().sigma_color) if denoise else None
        self._max_history = float(temporal_params(max_history=temporal_kw.get("max_history")).max_history)
        self.antilag, self.last_scale = None, None
        if antilag is not False and antilag is not None:
            from . import antilag as lag
            self.antilag = {} if antilag is True else dict(antilag)
            lag._params(self.antilag.get("radius"), ((k, v) for k, v in self.antilag.items() if k != "radius"))      # (refuses an unknown name now)
            self._antilag_workspace = torch.empty((lag.workspace_bytes(w, h),), dtype=torch.uint8, device="cuda")
            self._scale = torch.empty((h, w), dtype=torch.float32, device="cuda")
        self._tables, self.last_motion_code = None, None
        if motion is not None:
            from . import motion as mo
            from .host import HostScene
            if not isinstance(motion, HostScene):
                raise ValueError(f"temporal_preview: motion must be the HostScene the scene was uploaded from, not {type(motion).__name__}")
            v = motion.view.contents
            if (int(v.num_vertices), int(v.num_spheres)) != (dev.num_vertices, dev.num_spheres):
                raise ValueError(f"temporal_preview: motion's host scene has {v.num_vertices} vertices and {v.num_spheres} spheres, the "
                                 f"resident scene {dev.num_vertices} and {dev.num_spheres}")
            self._tables = mo.SceneTables.from_host(motion)
            self._centre_rays = None       # (the camera's bytes, its pixel-centre rays)
        self._guides = GuideCache(dev)
        self.reset()

    def reset(self):
        """Drops the history: the next frame() starts over, as the first one did."""
        self._frozen = None        # the History of the last frame before the last change, or None
        self.history = None        # the History of the last frame(): unfiltered radiance, lengths, guides
        self._write = 0            # which buffer the frames since the last change write
        self._generation = None
        self._guides.held = None
        self._k = 0
        self._frames = 0           # frames accumulated since the reset: the nominal history length of the next output
        self.phase = None          # with ``sparse``: the lattice phase of the last frame()
        self._positions = None     # with ``motion``: the scene's Positions at the last frame(), at the frozen history's frame,
        self._frozen_positions = None
        self._previous = None      # and Q, the previous-world position frame of the frames since the last change, or None

    def frame(self, out=None, stream=None):
        """The preview of the scene as it now stands: ``samples`` more samples, accumulated; [H, W, 3] float32 CUDA
        tensor (``out`` when given)."""
        from . import filter as flt
        dev, acc = self._dev, self.acc
        froze = False
        if self._generation != dev.generation:
            acc.reset(stream=stream)
            if self.history is not None:           # the last frame's history freezes; the other buffer is written from now on
                self._frozen, self._write, froze = self.history, 1 - self._write, True
                self._frozen_positions = self._positions
            self._generation, self._k = dev.generation, 0
        g = self._guides.get(acc.params, self.feature_samples, self._features, stream=stream)
        if self._tables is not None:
            self._motion(g, froze, stream)
        position = g["position"] if self._previous is None else self._previous
        if self.sparse:
            mean = self._render_sparse(g, stream)
        else:
            mean = acc.render(self.samples, stream=stream)
        if froze and self.antilag is not None:     # once per freeze: the frozen history is never written otherwise
            from . import antilag as lag
            self.last_scale = lag.rescale(mean, g["normal"], g["position"], g["depth"], self._frozen, world_to_pixel(dev.camera),
                                          out_scale=self._scale, workspace=self._antilag_workspace, stream=stream, **self.antilag)[1]
        self._k += 1
        target = mean if out is None else out
        if self.variance_guided:
            return self._frame_variance_guided(mean, g, position, target, stream)
        if self.sparse:
            from . import wtemporal
            self.history = wtemporal.accumulate(mean, g["normal"], position, g["depth"], self._weight, history=self._frozen,
                                                world_to_pixel=world_to_pixel(dev.camera), out=target, out_code=False,
                                                next_history=self._buffers[self._write], stream=stream, **self.temporal_kw)[0]
        else:
            self.history = accumulate(mean, g["normal"], position, g["depth"], history=self._frozen,
                                      world_to_pixel=world_to_pixel(dev.camera), out=target, next_history=self._buffers[self._write],
                                      stream=stream, current_weight=self._k, **self.temporal_kw)
        self._current_world(g, stream)
        self._frames += 1
        if self.denoise:
            n = min(float(self._frames), self._max_history) if self.scale_sigma_color else 1.0
            sigma_color = self._sigma_color / math.sqrt(n)
            flt.atrous(target, g["normal"], g["position"], g["depth"], albedo=g["albedo"], out=target, workspace=self._workspace,
                       stream=stream, sigma_color=sigma_color, **self.filter_kw)
        return target

    def _motion(self, g, froze, stream):
        """frame() with ``motion``: notes the scene's positions at this frame and, on a frame that froze a history under
        other positions, computes Q (``self._previous``) and ``last_motion_code``; on a change without one, drops Q."""
        from . import motion as mo
        dev, first = self._dev, self._tables.positions
        now = mo.Positions(first.vertices if dev.vertices_given is None else dev.vertices_given,
                           first.spheres if dev.spheres_given is None else dev.spheres_given)
        if self._k == 0:                   # the scene had changed: Q belongs to the frames before
            self._previous = None
            old = self._frozen_positions
            moved = [froze and old is not None and o is not n for o, n in zip(old or now, now)]
            if any(moved):
                import torch
                h, w = self.acc.pixel_shape
                key = bytes(dev.camera)
                if self._centre_rays is None or self._centre_rays[0] != key:
                    with torch.cuda.stream(stream):
                        samples = torch.from_numpy(mo.centre_samples(h, w)).to("cuda")
                    self._centre_rays = (key, dev.camera_rays(samples, stream=stream))
                rays = self._centre_rays[1]
                hits = torch.empty((h * w, 4), dtype=torch.float32, device="cuda")      # VimgRayHit records, as they are
                dev.trace_rays(rays, out=hits, stream=stream)
                self._previous, self.last_motion_code = mo.previous_position(
                    g["position"], hits, rays, self._tables, mo.Positions(*(o if m else None for o, m in zip(old, moved))),
                    mo.Positions(*(n if m else None for n, m in zip(now, moved))), stream=stream)
        self._positions = now

    def _current_world(self, g, stream):
        """After an accumulate call that was given Q: plane G1 of the history it wrote gets the CURRENT positions."""
        if self._previous is not None:
            import torch
            with torch.cuda.stream(stream):
                self.history.tensor[2, :, :, :3].copy_(g["position"])

    def _render_sparse(self, g, stream):
        """The sparse increment of frame(): one masked render launch on the lattice of this frame's phase, the fill,
        and the weight frame for wtemporal.accumulate (``self._weight``).  Returns the filled picture."""
        import torch
        from . import infill, wtemporal
        acc = self.acc
        h, w = acc.pixel_shape
        self.phase = self._frames % (self.sparse * self.sparse)
        with torch.cuda.stream(stream):          # (the mask is filled where the increment reads it)
            lattice = infill.lattice_mask(h, w, self.sparse, self.phase)
        noisy = acc.render(self.samples, stream=stream, mask=lattice)
        state = acc.state(stream)
        filled, code = infill.reconstruct(noisy, g["normal"], g["position"], g["depth"], state["count"], albedo=g["albedo"],
                                          radius=self.sparse, out=noisy, workspace=self._infill_workspace, stream=stream)
        with torch.cuda.stream(stream):
            self._weight = wtemporal.sparse_weights(state["count"], code, state["batches"], fill_weight=self.fill_weight)
        return filled

    def _frame_variance_guided(self, mean, g, position, target, stream):
        """The rest of frame() with ``variance_guided``: moments.accumulate in place of accumulate, handing the variance
        of the accumulated colour to varfilter.atrous.  The accumulator knows a variance once this camera position has
        had two increments; until then the moments alone say what a pixel's noise is."""
        from . import moments, varfilter
        known = self.acc.variance(stream) if self._k >= 2 else None
        self.history = moments.accumulate(mean, g["normal"], position, g["depth"], variance=known, history=self._frozen,
                                          world_to_pixel=world_to_pixel(self._dev.camera), out=target, out_variance=self._variance,
                                          next_history=self._buffers[self._write], stream=stream, current_weight=self._k,
                                          **self.temporal_kw)
        self._current_world(g, stream)
        self._frames += 1
        varfilter.atrous(target, g["normal"], g["position"], g["depth"], albedo=g["albedo"], variance=self._variance, out=target,
                         workspace=self._workspace, stream=stream, **self.filter_kw)
        return target

    def close(self):
        self.acc.close()


__all__ = ["accumulate", "temporal_params", "history_bytes", "world_to_pixel", "History", "TemporalPreview", "FRAMES"]
