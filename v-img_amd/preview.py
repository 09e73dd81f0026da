"""The previews of a resident scene, composed from the frame libraries: ``denoise``, the filter choice of
every preview, and TemporalPreview, whose frame() is one straight line over parts chosen once - an increment, an
accumulation, a filter, and the options despeckle, anti-lag, motion, exposure, demand and rectify.  A part owns its buffers and its state and
imports the libraries it needs and no others; a new mode is a new part and one line of TemporalPreview.__init__.  There
is no CPU fallback."""
import math

from .filter import GUIDES
from .hip import GuideCache
from .temporal import accumulate, temporal_params, world_to_pixel


def denoise(color, g, variance_guided=False, variance=None, **kw):
    """The a-trous filter on ``color`` guided by the feature frames ``g`` (render_features' dict of GUIDES): the fixed one
    (vimg_amd.filter.atrous), or with ``variance_guided`` the variance-guided one (vimg_amd.varfilter.atrous) on the
    per-pixel ``variance`` of ``color`` - None: every pixel's is estimated from its surroundings.  ``kw``: ``out``,
    ``workspace``, ``stream`` and the parameters of the filter chosen, all optional.  Returns the filtered [H, W, 3] image
    (``out`` when given)."""
    if variance_guided:
        from . import varfilter
        return varfilter.atrous(color, g["normal"], g["position"], g["depth"], albedo=g["albedo"], variance=variance, **kw)[0]
    from . import filter as flt
    return flt.atrous(color, g["normal"], g["position"], g["depth"], albedo=g["albedo"], **kw)


def despeckle_kw(given, what):
    """The ``despeckle`` argument of a preview (``what`` names it in a refusal): None or False - no clamp, None is
    returned; True - the library's defaults, {}; a dict - despeckle.params' keywords, checked here."""
    if given is None or given is False:
        return None
    if given is not True and not isinstance(given, dict):
        raise ValueError(f"{what}: despeckle must be None, a bool or a dict of vimg_amd.despeckle's parameters, not {type(given).__name__}")
    from . import despeckle
    kw = {} if given is True else dict(given)
    despeckle.params(**kw)           # (refuses an unknown name now)
    return kw


def clamp_fireflies(color, g, kw, **call):
    """``color`` with its fireflies clamped IN PLACE (vimg_amd.despeckle.clamp, include/vimg_despeckle.h) by the feature
    frames ``g``, before any filter sees it; ``kw``: despeckle_kw's answer, None: nothing is done.  ``call``: ``workspace``,
    ``stream``.  ``color`` must be the caller's own frame, never a buffer of the accumulator."""
    if kw is not None:
        from . import despeckle
        despeckle.clamp(color, g["normal"], g["position"], g["depth"], albedo=g["albedo"], out=color, out_code=False, **call, **kw)
    return color


def exposure_kw(given, what):
    """The ``exposure`` argument of a preview (``what`` names it in a refusal): None or False - the frame stays linear,
    None is returned; True - the library's defaults, {}; a dict - exposure.params' keywords, checked here."""
    if given is None or given is False:
        return None
    if given is not True and not isinstance(given, dict):
        raise ValueError(f"{what}: exposure must be None, a bool or a dict of vimg_amd.exposure's parameters, not {type(given).__name__}")
    from . import exposure
    kw = {} if given is True else dict(given)
    exposure.params(**kw)            # (refuses an unknown name now)
    return kw


def expose(frame, kw, state=None, stream=None):
    """``frame`` scaled IN PLACE by the exposure it is metered to (vimg_amd.exposure.adapt, include/vimg_exposure.h): the
    last stage of a preview, on its output alone.  ``kw``: exposure_kw's answer, None: nothing is done.  ``state``: the
    exposure state to carry on, None: a fresh one.  Every pixel is metered, misses too: they are part of the picture."""
    if kw is not None:
        from . import exposure
        exposure.adapt(frame, state=state, out=frame, stream=stream, **kw)
    return frame


def demand_kw(given, what):
    """The ``demand`` argument of a preview (``what`` names it in a refusal): None or False - the lattice alone, None is
    returned; True - the library's defaults, {}; a dict - it carries ``min_history``, checked here."""
    if given is None or given is False:
        return None
    if given is not True and not isinstance(given, dict):
        raise ValueError(f"{what}: demand must be None, a bool or a dict with min_history, not {type(given).__name__}")
    from . import demand
    kw = {} if given is True else dict(given)
    if set(kw) - {"min_history"}:
        raise TypeError(f"demand: unknown parameters {sorted(set(kw) - {'min_history'})}; expected some of ('min_history',)")
    demand.params(**kw)
    return kw


def _empty(dtype, *shape):
    import torch
    return torch.empty(shape, dtype=getattr(torch, dtype), device="cuda")


def _absent(*args):
    """An option that was not taken: does nothing, holds nothing."""


def _of(part, name):
    """A read-only attribute of TemporalPreview that one of its parts holds; None when the part holds no such thing."""
    return property(lambda self: getattr(getattr(self, part), name, None))


# ---- the increment: (acc, samples, guides, frames since reset(), stream) -> (the picture, its weight frame, its lattice phase;
# None where it has none) ----------------------------------------------------------------------------------------------------
_full_increment = lambda acc, samples, g, frames, stream: (acc.render(samples, stream=stream), None, None)


class _SparseIncrement:
    """``sparse`` (a stride 2..4): a frame samples ONE pixel in sparse^2 and the history supplies the
    rest.  A frame() is then: the lattice infill.lattice_mask(H, W, sparse, phase) with phase = (frames since reset())
    mod sparse^2 - a camera change does not restart it, so a moving camera still visits every cell - one
    acc.render(samples, mask=lattice), infill.reconstruct with acc.counts(), the cached guides, the albedo and
    radius = sparse, wtemporal.sparse_weights (a pixel with samples weighs its increments, a filled one
    ``fill_weight``, default wtemporal.FILL_WEIGHT, a fallback or a hole 0) and wtemporal.accumulate
    (include/vimg_wtemporal.h) in place of accumulate: a sampled pixel blends as ever, a filled pixel takes its
    reprojected history where it has one, and the fill is used only where the history has nothing.  After sparse^2
    frames of a standing camera the accumulator is bit for bit a Progressive after one render(samples).  ``history``
    stays a History; ``variance_guided`` is refused with it (the moments history is not weighted per pixel)."""

    def __init__(self, dev, stride, fill_weight):
        from . import infill, wtemporal
        infill.lattice_cell(stride, 0)           # (refuses a stride outside 2..4)
        self.stride = int(stride)
        self.fill_weight = wtemporal.FILL_WEIGHT if fill_weight is None else float(fill_weight)
        if not self.fill_weight >= 0.0:
            raise ValueError(f"temporal_preview: fill_weight must be >= 0, not {fill_weight}")
        self._workspace = _empty("uint8", infill.workspace_bytes(*dev.resolution))

    def __call__(self, acc, samples, g, frames, stream):
        """One masked render launch on the lattice of this frame's phase, the fill, and the weight frame for
        wtemporal.accumulate.  Returns the filled picture, that frame and the phase."""
        import torch
        from . import infill, wtemporal
        phase = frames % (self.stride * self.stride)
        noisy = acc.render(samples, stream=stream, mask=self._lattice(acc, samples, g, phase, stream))
        state = acc.state(stream)
        filled, code = infill.reconstruct(noisy, g["normal"], g["position"], g["depth"], state["count"], albedo=g["albedo"], radius=self.stride,
                                          out=noisy, workspace=self._workspace, stream=stream)
        with torch.cuda.stream(stream):
            weight = wtemporal.sparse_weights(state["count"], code, state["batches"], fill_weight=self.fill_weight)
        return filled, weight, phase

    def _lattice(self, acc, samples, g, phase, stream):
        import torch
        from . import infill
        with torch.cuda.stream(stream):          # (the mask is filled where the increment reads it)
            return infill.lattice_mask(*acc.pixel_shape, self.stride, phase)


class _DemandIncrement(_SparseIncrement):
    """``demand`` (True: the library's defaults; a dict: ``min_history``), with ``sparse``: the frame
    that renders first after a change - a scene change, reset(), the first frame - samples, beside its lattice, every live
    pixel whose lookup in the frozen history finds less than min_history (vimg_amd.demand, include/vimg_demand.h): the
    mask is demand.mask of the cached guides against the frozen history, with the position frame the accumulate call will
    get (with ``motion``: Q), at this frame's lattice phase and with ``temporal_kw``'s sigmas, so the lengths it reads are
    the accumulate call's own.  A pixel the camera has uncovered has a sample on the frame it appears on instead of up to
    sparse^2 frames later, and the first frame after reset() is a full one.  On standing frame k >= 1 (k: frames since
    the change) the mask is lattice(phase) & (count <= samples (k // sparse^2)), in torch on the stream: a pixel that was
    sampled on demand skips its lattice turn in the first cycle, every masked launch still sees one count, and after
    sparse^2 frames of a standing camera the accumulator is, as without ``demand``, bit for bit a Progressive after one
    render(samples).  The rest of the frame is _SparseIncrement's.  ``last_demand`` is (mask, length, counts) of the last
    library call: [H, W] uint8, [H, W] float32 and the four device words demand.read() names (None before the first).
    ``antilag`` cuts the history AFTER the increment is rendered, so demand sees the uncut lengths: a pixel antilag cuts
    is demanded one frame later, on the next change."""

    def __init__(self, dev, stride, fill_weight, kw, sigmas):
        from . import demand
        super().__init__(dev, stride, fill_weight)
        w, h = dev.resolution
        self.demand, self._sigmas = kw, sigmas
        self._mask, self._length, self._counts = _empty("uint8", h, w), _empty("float32", h, w), demand.new_counts()
        self.reset()

    def reset(self):
        self.last = None           # last_demand
        self._asked = (None, None, 0)

    def ask(self, frozen, position, k):
        """What frame() knows and the increment's signature does not carry: the frozen history, the position frame of
        this frame's accumulate call and the frames since the change."""
        self._asked = (frozen, position, k)

    def _lattice(self, acc, samples, g, phase, stream):
        import torch
        from . import demand, infill
        frozen, position, k = self._asked
        if k == 0:
            self.last = demand.mask(g["normal"], position, g["depth"], history=frozen, stride=self.stride, phase=phase,
                                    out=self._mask, out_length=self._length, counts=self._counts, stream=stream,
                                    **self._sigmas, **self.demand)
            return self.last[0]
        count = acc.counts(stream)
        with torch.cuda.stream(stream):
            lattice = infill.lattice_mask(*acc.pixel_shape, self.stride, phase)
            return lattice & (count <= samples * (k // (self.stride * self.stride))).to(torch.uint8)


# ---- the accumulation: (acc, k, the picture, guides, the position frame, the increment's weight frame, the variance frame to
# write, **what every accumulate call takes) -> the History ------------------------------------------------------------------
def _plain_accumulation(acc, k, mean, g, position, weight, variance, **call):
    return accumulate(mean, g["normal"], position, g["depth"], current_weight=k, **call)


def _weighted_accumulation(acc, k, mean, g, position, weight, variance, **call):
    from . import wtemporal
    return wtemporal.accumulate(mean, g["normal"], position, g["depth"], weight, out_code=False, **call)[0]


def _moments_accumulation(acc, k, mean, g, position, weight, variance, **call):
    """``variance_guided`` (with ``denoise``) lifts that limit: the histories carry the moments of luminance
    (vimg_amd.moments, include/vimg_moments.h; ``temporal_kw`` then takes min_history too), a frame is acc.render,
    acc.variance() once this camera position has had two increments (else no variance frame), moments.accumulate and
    varfilter.atrous on the accumulated colour with the variance the moments give - NaN where the history is shorter
    than min_history, which the filter estimates from the pixel's surroundings.  ``filter_kw`` are then
    varfilter.atrous's parameters, ``scale_sigma_color`` is refused, and ``history`` is a moments.History.  The
    accumulated colour, the history lengths and the accumulator are bit for bit what they are without it.

    The accumulator knows a variance once this camera position has had two increments; until then the moments alone
    say what a pixel's noise is.  The history has four planes, and ``variance`` is the frame _variance_filter reads."""
    from . import moments
    known = acc.variance(call["stream"]) if k >= 2 else None
    return moments.accumulate(mean, g["normal"], position, g["depth"], variance=known, out_variance=variance, current_weight=k, **call)


# ---- the filter: (the accumulated picture, guides, frames since reset(), stream) -> the picture, filtered in place --------
_no_filter = lambda target, g, frames, stream: target


def _fixed_filter(dev, kw, scale, max_history):
    """With ``denoise`` the a-trous filter runs on the accumulated colour for
    the output only; the history keeps unfiltered radiance.  The filter's sigma_color (``filter_kw``'s, or the filter
    library's default) is divided by sqrt(n), n = the frames accumulated since the last reset(), at most max_history:
    its colour term measures colour differences against the noise it expects, and the noise of n accumulated frames is
    1 / sqrt(n) of one frame's, so the filter does less as the history does more (the first frame is filtered as
    Progressive.preview filters it).  It is one factor for the picture: pixels that have just started over are filtered
    as lightly as the rest.  ``scale_sigma_color=False`` passes sigma_color as it is."""
    from . import filter as flt
    sigma_color = float(kw.pop("sigma_color", None) or flt.atrous_params().sigma_color)
    workspace = _empty("uint8", flt.atrous_workspace_bytes(*dev.resolution))

    def run(target, g, frames, stream):
        n = min(float(frames), max_history) if scale else 1.0
        return denoise(target, g, out=target, workspace=workspace, stream=stream, sigma_color=sigma_color / math.sqrt(n), **kw)
    return run


def _variance_filter(dev, kw, variance):
    from . import varfilter
    workspace = _empty("uint8", varfilter.workspace_bytes(*dev.resolution))

    def run(target, g, frames, stream):
        return denoise(target, g, variance_guided=True, variance=variance, out=target, workspace=workspace, stream=stream, **kw)
    return run


class _Despeckle:
    """``despeckle`` (True: the library's defaults; a dict: despeckle.clamp's parameters): every frame()'s
    increment - the running mean acc.render returned, a frame of its own, never the accumulator's sums - has its fireflies
    clamped in place (vimg_amd.despeckle, include/vimg_despeckle.h) right after it is rendered, on moving and standing
    frames alike: the anti-lag test, the moments, the history and the filter all see the clamped frame, and the
    accumulator stays bit for bit a Progressive.  It is refused with ``sparse``: a lattice pixel's neighbours carry no
    samples."""

    def __init__(self, dev, kw):
        from . import despeckle
        self.params = kw
        self._workspace = _empty("uint8", despeckle.workspace_bytes(*dev.resolution))

    def __call__(self, mean, g, stream):
        clamp_fireflies(mean, g, self.params, workspace=self._workspace, stream=stream)


# ---- the exposure: (the picture frame() is about to return, stream) -> the picture ------------------------------------------
_linear = lambda frame, stream: frame


class _Exposure:
    """``exposure`` (True: the library's defaults; a dict: exposure.adapt's parameters): the frame that
    frame() returns - after the accumulation and the filter, a buffer of its own - is metered and scaled in place by an
    exposure that lives in ``state``, 1040 bytes of device memory, and moves toward key / metered from frame to frame
    (vimg_amd.exposure, include/vimg_exposure.h): nothing is read back.  It is the last stage and touches the output
    alone: the accumulator, the history and every filter input stay linear and bit for bit what they are without it.
    reset() zeroes the state: the next frame is scaled to its own target."""

    def __init__(self, dev, kw):
        from . import exposure
        self.params, self.state = kw, exposure.new_state()

    def reset(self):
        self.state.zero_()

    def __call__(self, frame, stream):
        return expose(frame, self.params, self.state, stream)


class _Antilag:
    """``antilag`` (True: the library's defaults; a dict: antilag.rescale's parameters): on the frame()
    on which the scene had changed and a history freezes, that frozen history's lengths are rescaled once
    (vimg_amd.antilag, include/vimg_antilag.h) - after this camera's first increment is rendered (with ``sparse``:
    rendered and filled) and before it is accumulated, against that increment and under the current camera's matrix:
    where the new picture disagrees with the history by more than its noise the lengths are cut, to 0 where it clearly
    does, and accumulate's taps there find a short history or none; everywhere else they find what they found before.
    ``last_scale`` is the [H, W] scale frame of the last such call, in the frozen history's pixel coordinates (None
    before the first).  Standing frames make no call and the accumulator stays bit for bit a Progressive.  With
    ``variance_guided`` only plane A's lengths are rescaled, NOT the moments of plane M: a scaled length below
    min_history makes the variance NaN there, which the filter estimates from the pixel's surroundings."""

    def __init__(self, dev, given):
        from . import antilag as lag
        self._lag, self._dev, self.params = lag, dev, {} if given is True else dict(given)
        lag._params(self.params.get("radius"), ((k, v) for k, v in self.params.items() if k != "radius"))      # (refuses an unknown name now)
        w, h = dev.resolution
        self._workspace, self._scale = _empty("uint8", lag.workspace_bytes(w, h)), _empty("float32", h, w)
        self.last_scale = None

    def __call__(self, mean, g, frozen, stream):
        """Once per freeze: the frozen history is never written otherwise."""
        self.last_scale = self._lag.rescale(mean, g["normal"], g["position"], g["depth"], frozen, world_to_pixel(self._dev.camera),
                                            out_scale=self._scale, workspace=self._workspace, stream=stream, **self.params)[1]


class _Motion:
    """``motion`` (the HostScene the DeviceScene was uploaded from, whose positions must be the resident ones at this
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
    object's old shadow on static surfaces still is."""

    def __init__(self, dev, host):
        from . import motion as mo
        from .host import HostScene
        if not isinstance(host, HostScene):
            raise ValueError(f"temporal_preview: motion must be the HostScene the scene was uploaded from, not {type(host).__name__}")
        v = host.view.contents
        if (int(v.num_vertices), int(v.num_spheres)) != (dev.num_vertices, dev.num_spheres):
            raise ValueError(f"temporal_preview: motion's host scene has {v.num_vertices} vertices and {v.num_spheres} spheres, the "
                             f"resident scene {dev.num_vertices} and {dev.num_spheres}")
        self._dev, self._tables = dev, mo.SceneTables.from_host(host)
        self._camera = self._rays = self.last_code = None       # a camera's bytes and its pixel-centre rays; last_motion_code
        self.reset()

    def reset(self):
        self._positions = None     # the scene's Positions at the last frame()
        self.previous = None       # Q, the previous-world position frame of the frames since the last change, or None

    def __call__(self, g, froze, stream):
        """Notes the scene's positions at this frame and, on a frame that froze a history under other positions, computes
        Q (``previous``) and ``last_motion_code``; on a freeze without one, drops Q.  Returns Q or None."""
        from . import motion as mo
        dev = self._dev
        now = mo.Positions(*(first if given is None else given
                             for first, given in zip(self._tables.positions, (dev.vertices_given, dev.spheres_given))))
        if froze:                          # Q belonged to the frames before; the frozen history's frame is the last one
            old, self.previous = self._positions, None
            moved = [o is not n for o, n in zip(old, now)]
            if any(moved):
                import torch
                w, h = dev.resolution
                if self._camera != bytes(dev.camera):
                    with torch.cuda.stream(stream):
                        samples = torch.from_numpy(mo.centre_samples(h, w)).to("cuda")
                    self._camera, self._rays = bytes(dev.camera), dev.camera_rays(samples, stream=stream)
                hits = _empty("float32", h * w, 4)      # VimgRayHit records, as they are
                dev.trace_rays(self._rays, out=hits, stream=stream)
                self.previous, self.last_code = mo.previous_position(
                    g["position"], hits, self._rays, self._tables, mo.Positions(*(o if m else None for o, m in zip(old, moved))),
                    mo.Positions(*(n if m else None for n, m in zip(now, moved))), stream=stream)
        self._positions = now
        return self.previous


FAST_HISTORY = 2.0      # _Rectify's default fast_history, by the sweep of DESIGN.md 4.33


def rectify_kw(given, what):
    """The ``rectify`` argument of a preview (``what`` names it in a refusal): None or False - no clamp, None is
    returned; True - the defaults, (FAST_HISTORY, {}); a dict - ``fast_history`` and rectify.params' keywords, checked
    here.  Returns (fast_history, the library's keywords)."""
    if given is None or given is False:
        return None
    if given is not True and not isinstance(given, dict):
        raise ValueError(f"{what}: rectify must be None, a bool or a dict of fast_history and vimg_amd.rectify's parameters, "
                         f"not {type(given).__name__}")
    from . import rectify
    kw = {} if given is True else dict(given)
    fast_history = kw.pop("fast_history", None)
    fast_history = FAST_HISTORY if fast_history is None else float(fast_history)
    if not 1.0 <= fast_history < math.inf:
        raise ValueError(f"{what}: rectify's fast_history must be >= 1 and finite, not {fast_history:g}")
    rectify.params(**kw)             # (refuses an unknown name now)
    return fast_history, kw


class _Rectify:
    """``rectify`` (True: the defaults; a dict: ``fast_history`` and rectify.clamp's parameters): beside
    the history of up to max_history frames a second one of ``fast_history`` frames (default FAST_HISTORY) is kept - the
    same temporal.accumulate call on the same colour, guides, position frame, current_weight and matrix, with
    max_history = fast_history, on two buffers of this part's own that freeze and swap exactly as the slow ones do -
    and right after the accumulation (with ``motion``: after plane G1 has its current positions back, which the fast
    history's G1 gets as well) the slow history's colour is clamped IN PLACE to the fast one's statistics around each
    pixel (vimg_amd.rectify, include/vimg_rectify.h), with the albedo frame for demodulation; the clamped colour is
    what the filter and the exposure then see and what frame() returns.  The slow accumulate call is then given no
    picture to write - the increment must reach the fast call as it was rendered - and the clamp writes the picture.  The fast history is always a temporal.History,
    also with ``variance_guided``, whose plane M stays what it is.  Stale radiance - an edit that ``antilag`` does not
    see, a moved object's shading, view-dependent shading - is then bounded within about fast_history frames.
    ``last_rectify_code`` is the [H, W] uint8 code frame of the last call.  The accumulator stays bit for bit a
    Progressive.  It is refused with ``sparse``: a filled pixel's weight would have to enter the fast history as well."""

    def __init__(self, dev, fast_history, kw):
        self.params, self.fast_history = kw, fast_history
        w, h = dev.resolution
        self._buffers = [_empty("float32", 3, h, w, 4) for _ in range(2)]
        self._code = _empty("uint8", h, w)
        self.reset()

    def reset(self):
        self._frozen = self.fast = None     # the fast History frozen at the last change, and the last frame()'s
        self._write = 0
        self.last_code = None               # last_rectify_code

    def __call__(self, froze, k, mean, g, position, moved, slow, target, matrix, sigmas, stream):
        from . import rectify
        if froze:
            self._frozen, self._write = self.fast, 1 - self._write
        self.fast = accumulate(mean, g["normal"], position, g["depth"], history=self._frozen, world_to_pixel=matrix,
                               next_history=self._buffers[self._write], stream=stream, current_weight=k,
                               max_history=self.fast_history, **sigmas)
        if moved:
            import torch
            with torch.cuda.stream(stream):
                self.fast.tensor[2, :, :, :3].copy_(g["position"])
        self.last_code = rectify.clamp(slow, self.fast, albedo=g["albedo"], out=target, code=self._code, stream=stream, **self.params)[2]


class TemporalPreview:
    """The preview of a resident scene whose camera moves (DeviceScene.temporal_preview): one Progressive, two history
    buffers and the a-trous workspace.  ``frame()`` returns the [H, W, 3] preview of the scene as it now stands.

    When the scene changed since the last frame (DeviceScene.generation: set_camera, update_*, rebuild_bvh) the
    accumulator is reset, the guides are rendered again, ``samples`` samples are rendered and blended with the last
    frame's history, reprojected by the last camera's matrix, at current_weight 1.  When nothing changed the
    accumulator goes on - it stays bit for bit what a Progressive alone would hold - and the running mean of its k
    increments is blended, at current_weight k, with the history frozen at the last change: the picture converges to
    the plain progressive image without a pop.

    The modes are parts of this module, chosen once here, and each tells its own contract: ``denoise`` and
    ``scale_sigma_color`` in _fixed_filter, ``variance_guided`` in _moments_accumulation, ``sparse`` and ``fill_weight``
    in _SparseIncrement, ``demand`` in _DemandIncrement, ``despeckle`` in _Despeckle, ``antilag`` in _Antilag, ``motion`` in _Motion, ``exposure`` in
    _Exposure, ``rectify`` in _Rectify.

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
    sparse, fill_weight = _of("_increment", "stride"), _of("_increment", "fill_weight")
    antilag, last_scale = _of("_cut", "params"), _of("_cut", "last_scale")
    despeckle = _of("_clamp", "params")
    last_motion_code, _previous = _of("_motion", "last_code"), _of("_motion", "previous")
    exposure, exposure_state = _of("_expose", "params"), _of("_expose", "state")
    demand, last_demand = _of("_increment", "demand"), _of("_increment", "last")
    rectify, fast_history, last_rectify_code = _of("_rectify", "params"), _of("_rectify", "fast_history"), _of("_rectify", "last_code")

    def __init__(self, dev, params, samples=4, denoise=True, feature_samples=4, filter_kw=None, scale_sigma_color=None,
                 variance_guided=False, sparse=None, fill_weight=None, antilag=False, motion=None, despeckle=None, exposure=None,
                 demand=None, rectify=None, **temporal_kw):
        if params.tile_world != 1:
            raise ValueError("temporal_preview: reprojection reads whole frames, not shards (tile_world must be 1)")
        if int(samples) < 1 or int(feature_samples) < 1:
            raise ValueError("temporal_preview: samples and feature_samples must be at least 1")
        self.variance_guided = bool(variance_guided)
        if self.variance_guided and not denoise:
            raise ValueError("temporal_preview: variance_guided chooses the filter, so it needs denoise=True")
        if self.variance_guided and scale_sigma_color is not None:
            raise ValueError("temporal_preview: scale_sigma_color belongs to the fixed filter; the variance-guided filter has no sigma_color")
        if sparse is not None and self.variance_guided:
            raise ValueError("temporal_preview: sparse does not go with variance_guided: the moments history has no per-pixel weights")
        if sparse is None and fill_weight is not None:
            raise ValueError("temporal_preview: fill_weight is the weight of a filled pixel: it needs sparse")
        clamp = despeckle_kw(despeckle, "temporal_preview")
        if clamp is not None and sparse is not None:
            raise ValueError("temporal_preview: despeckle does not go with sparse: a lattice pixel's neighbours carry no samples")
        exposed = exposure_kw(exposure, "temporal_preview")
        demanded = demand_kw(demand, "temporal_preview")
        if demanded is not None and sparse is None:
            raise ValueError("temporal_preview: demand chooses the pixels a sparse frame samples: it needs sparse")
        rectified = rectify_kw(rectify, "temporal_preview")
        if rectified is not None and sparse is not None:
            raise ValueError("temporal_preview: rectify does not go with sparse: a filled pixel's weight would have to enter the fast history too")
        sigmas = {k: temporal_kw[k] for k in ("sigma_normal", "sigma_plane") if k in temporal_kw}
        self._sigmas = sigmas
        self._increment = (_full_increment if sparse is None else _SparseIncrement(dev, sparse, fill_weight) if demanded is None else
                           _DemandIncrement(dev, sparse, fill_weight, demanded, sigmas))
        self._ask = getattr(self._increment, "ask", _absent)
        unknown = sorted(set(temporal_kw) - {"max_history", "sigma_normal", "sigma_plane"} - ({"min_history"} if variance_guided else set()))
        if unknown:
            raise TypeError(f"temporal_preview: unknown parameters {unknown}")
        self._dev, self.samples, self.denoise, self.feature_samples = dev, int(samples), bool(denoise), int(feature_samples)
        self.temporal_kw, self.filter_kw = dict(temporal_kw), dict(filter_kw or {})
        self.scale_sigma_color = scale_sigma_color is None or bool(scale_sigma_color)
        self.acc = dev.progressive(params)
        self._accumulate = _moments_accumulation if self.variance_guided else _plain_accumulation if sparse is None else _weighted_accumulation
        w, h = dev.resolution
        self._buffers = [_empty("float32", 4 if self.variance_guided else 3, h, w, 4) for _ in range(2)]
        self._variance = _empty("float32", h, w) if self.variance_guided else None
        self._features = GUIDES if denoise or sparse is not None or clamp is not None or rectified is not None else ("normal", "position", "depth")
        max_history = float(temporal_params(max_history=temporal_kw.get("max_history")).max_history)
        self._filter = (_no_filter if not denoise else _variance_filter(dev, self.filter_kw, self._variance) if self.variance_guided else
                        _fixed_filter(dev, self.filter_kw, self.scale_sigma_color, max_history))
        self._clamp = _absent if clamp is None else _Despeckle(dev, clamp)
        self._cut = _absent if antilag is False or antilag is None else _Antilag(dev, antilag)
        self._motion = _absent if motion is None else _Motion(dev, motion)
        self._expose = _linear if exposed is None else _Exposure(dev, exposed)
        self._rectify = _absent if rectified is None else _Rectify(dev, *rectified)
        self._resets = [part.reset for part in (self._increment, self._cut, self._motion, self._expose, self._rectify) if hasattr(part, "reset")]
        self._guides = GuideCache(dev)
        self.reset()

    def reset(self):
        """Drops the history: the next frame() starts over, as the first one did."""
        self._frozen = None        # the History of the last frame before the last change, or None
        self.history = None        # the History of the last frame(): unfiltered radiance, lengths, guides
        self._write = 0            # which buffer the frames since the last change write
        self._generation = self._guides.held = None
        self._k = 0
        self._frames = 0           # frames accumulated since the reset: the nominal history length of the next output
        self.phase = None          # with ``sparse``: the lattice phase of the last frame()
        for reset in self._resets:
            reset()

    def frame(self, out=None, stream=None):
        """The preview of the scene as it now stands: ``samples`` more samples, accumulated; [H, W, 3] float32 CUDA
        tensor (``out`` when given)."""
        dev, acc, froze = self._dev, self.acc, False
        if self._generation != dev.generation:
            acc.reset(stream=stream)
            if self.history is not None:           # the last frame's history freezes; the other buffer is written from now on
                self._frozen, self._write, froze = self.history, 1 - self._write, True
            self._generation, self._k = dev.generation, 0
        g = self._guides.get(acc.params, self.feature_samples, self._features, stream=stream)
        previous = self._motion(g, froze, stream)          # Q, or None
        self._ask(self._frozen, g["position"] if previous is None else previous, self._k)
        mean, weight, self.phase = self._increment(acc, self.samples, g, self._frames, stream)
        self._clamp(mean, g, stream)
        if froze:
            self._cut(mean, g, self._frozen, stream)
        self._k += 1
        target = mean if out is None else out
        position, matrix, rectified = g["position"] if previous is None else previous, world_to_pixel(dev.camera), self._rectify is not _absent
        # with ``rectify`` the accumulate call writes no picture - the increment stays what it is for the fast history - and
        # the clamp writes ``target`` from the history it has clamped
        self.history = self._accumulate(acc, self._k, mean, g, position, weight, self._variance,
                                        history=self._frozen, world_to_pixel=matrix, out=None if rectified else target,
                                        next_history=self._buffers[self._write], stream=stream, **self.temporal_kw)
        if previous is not None:       # the accumulate call was given Q: plane G1 of the history it wrote gets the CURRENT positions
            import torch
            with torch.cuda.stream(stream):
                self.history.tensor[2, :, :, :3].copy_(g["position"])
        self._rectify(froze, self._k, mean, g, position, previous is not None, self.history, target, matrix, self._sigmas, stream)
        self._frames += 1
        return self._expose(self._filter(target, g, self._frames, stream), stream)

    def close(self):
        self.acc.close()
