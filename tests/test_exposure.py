"""The auto-exposure on the GPU (libvimg_exposure.so, include/vimg_exposure.h): vimg_exposure_adapt
against the numpy restatement of its contract (tests/exposure_ref.py) BIT FOR BIT, the state's 1040 bytes and the scaled
frame both, at the sizes where the meter's grid and its tail can go wrong and with every value that is not a luminance
planted; a sequence on one state; a caller's stream; and ``exposure=`` on DeviceScene.temporal_preview and
render_denoised: the last stage, on the output alone, and nothing at all when it is None."""
import numpy as np
import pytest

import exposure_ref as R
import scenes
from test_despeckle import orbit_camera

pytestmark = pytest.mark.gpu
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F
    diff = _bits(got) != _bits(want)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4].tolist(), got[diff][:4], want[diff][:4])


def _state_bytes(state):
    return state.cpu().numpy().view(np.uint8)


def _same_state(got, want):
    got = _state_bytes(got)
    assert got.shape == (R.STATE_BYTES,)
    assert np.array_equal(got, want), (R.read(got), R.read(want), np.flatnonzero(got != want)[:8].tolist())


def _ibits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(scope="module")
def gpu():
    from vimg_amd import exposure, hip
    hip.init(0)
    return exposure


# 1 x 1; 7 x 5, less than a wave; 65 x 4, a ragged last wave; 130 x 67, 35 workgroups with ragged rows and columns;
# 512 x 300 = 153600 pixels, more than twice the 65536 lanes of the capped grid: the grid-stride loop wraps twice, the
# third pass ragged
SIZES = [(1, 1), (7, 5), (65, 4), (130, 67), (512, 300)]


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_every_size_is_the_restatement_bit_for_bit(gpu, size):
    """With and without a depth frame (misses, a negative and a NaN depth in it), with NaN, +-inf, 0, negative, denormal and
    edge-valued pixels planted (as far as the frame has room), out of place, in place and meter-only, on a fresh state
    and, for the rates' branch, on the state the first call left - every parameter explicit."""
    import torch
    from vimg_amd import abi
    w, h = size
    assert (w * h > abi.EXPOSURE_MAX_WORKGROUPS * 256) == (size == SIZES[-1])
    kw = dict(low_permille=300, high_permille=900, key=0.2, min_exposure=1 / 1024, max_exposure=48.0, rate_brighten=0.3, rate_darken=0.6)
    for with_depth in (False, True):
        color, depth = R.planted(h, w, seed=int(with_depth), depth=with_depth)
        d_color, d_depth = torch.from_numpy(color).cuda(), None if depth is None else torch.from_numpy(depth).cuda()
        want, want_state = R.adapt(color, depth, **kw)
        if w * h > 40:
            assert R.read(want_state)["frames"] == 1 and 0 < R.read(want_state)["counted"] < w * h
        # out of place, into a buffer the call fills whole
        out, state = torch.full_like(d_color, -3.0), gpu.new_state()
        res, st = gpu.adapt(d_color, d_depth, state=state, out=out, **kw)
        assert res is out and st is state
        _same(out.cpu().numpy(), want)
        _same_state(state, want_state)
        assert np.array_equal(_bits(d_color.cpu().numpy()), _bits(color))          # the frame was only read
        # in place
        buf, state = d_color.clone(), gpu.new_state()
        res, _ = gpu.adapt(buf, d_depth, state=state, out=buf, **kw)
        assert res is buf
        _same(buf.cpu().numpy(), want)
        _same_state(state, want_state)
        # meter only
        state = gpu.new_state()
        res, _ = gpu.adapt(d_color, d_depth, state=state, **kw)
        assert res is None
        _same_state(state, want_state)
        # a second call on that state, of the frame at a quarter and then at four times the radiance: both rates
        for scale in (0.25, 4.0):
            with np.errstate(over="ignore", invalid="ignore"):
                scaled = (color * F(scale)).astype(F)
            want2, want_state2 = R.adapt(scaled, depth, state=want_state, **kw)
            st2 = state.clone()
            got2, _ = gpu.adapt(torch.from_numpy(scaled).cuda(), d_depth, state=st2, out=True, **kw)
            _same(got2.cpu().numpy(), want2)
            _same_state(st2, want_state2)


def test_a_sequence_on_one_state(gpu):
    """Six frames on one state at the library's defaults, the radiance quartered after the third and an all-black frame
    between the second and the third: every call's state and output are the restatement's, ``frames`` counts the six,
    the histogram is zero after each call, the black frame leaves E where it was, and E moves toward E* by the stated
    rates - brightening a quarter of the way per call after the radiance falls."""
    import torch
    rng = np.random.default_rng(3)
    base = (F(2) ** rng.uniform(-4, 3, (67, 130, 1)).astype(F) * rng.uniform(0.5, 1.5, (67, 130, 3)).astype(F)).astype(F)
    frames = [base * F(1 + 0.01 * i) for i in range(3)] + [base * F(0.25 * (1 + 0.01 * i)) for i in range(3)]
    frames.insert(2, np.zeros_like(base))
    state, want_state = gpu.new_state(), R.new_state()
    assert gpu.read(state) == dict(exposure=1.0, frames=0, metered=0.0, counted=0)
    seen = []
    for n, color in enumerate(frames):
        color = np.ascontiguousarray(color, F)
        before = R.read(want_state)
        want, want_state = R.adapt(color, state=want_state)
        got, st = gpu.adapt(torch.from_numpy(color).cuda(), state=state, out=True)
        assert st is state
        _same(got.cpu().numpy(), want)
        _same_state(state, want_state)
        now = gpu.read(state)
        assert now == R.read(want_state) and not _state_bytes(state)[:1024].any()
        if n == 2:
            assert now == dict(before, counted=0)
            _same(got.cpu().numpy(), color * F(before["exposure"]))
            continue
        target = float(R.target(color))
        if before["frames"] == 0:
            assert now["exposure"] == target
        else:
            rate = F(0.5) if F(target) < F(before["exposure"]) else F(0.25)
            assert now["exposure"] == float(F(before["exposure"]) + (F(target) - F(before["exposure"])) * rate)
        seen.append((before["exposure"], target, now["exposure"]))
    assert gpu.read(state)["frames"] == 6 and gpu.read(state)["counted"] == 67 * 130
    # after the radiance is quartered the target is about four times the exposure, and each call covers a quarter of the way
    was, target, now = seen[3]
    assert 3.5 < target / was < 4.5 and now == pytest.approx(was + 0.25 * (target - was), rel=1e-6)
    assert seen[3][2] < seen[4][2] < seen[5][2] < seen[5][1]
    # ... and a frame a little brighter than the last (1 % each) darkens at the other rate
    assert seen[1][1] < seen[1][0] and seen[1][2] == pytest.approx(seen[1][0] + 0.5 * (seen[1][1] - seen[1][0]), rel=1e-6)


def test_a_callers_stream_numpy_frames_and_what_is_refused(gpu):
    """The same bits on the default stream, inside ``with torch.cuda.stream(side)`` and with ``stream=side`` while the
    default stream is current (tests/test_stream_rule.py's three ways): the call has no synchronisation of its own to
    lean on, its three launches are ordered by the stream alone."""
    import torch
    from vimg_amd import hip
    color, depth = R.planted(67, 130, seed=5, depth=True)
    want, want_state = R.adapt(color, depth)
    side = torch.cuda.Stream()
    assert torch.cuda.current_stream().cuda_stream != side.cuda_stream
    for way in ("default stream", "with torch.cuda.stream(side)", "stream=side"):
        d_color, d_depth, state = torch.from_numpy(color).cuda(), torch.from_numpy(depth).cuda(), gpu.new_state()
        torch.cuda.synchronize()
        if way == "with torch.cuda.stream(side)":
            with torch.cuda.stream(side):
                got, _ = gpu.adapt(d_color, d_depth, state=state, out=True)
        else:
            got, _ = gpu.adapt(d_color, d_depth, state=state, out=True, stream=side if way == "stream=side" else None)
        side.synchronize()
        torch.cuda.current_stream().synchronize()
        _same(got.cpu().numpy(), want)
        _same_state(state, want_state)
    # numpy in, numpy out; the state stays on the device, and without one the call makes its own
    got, state = gpu.adapt(color, depth, out=True)
    assert isinstance(got, np.ndarray) and isinstance(state, torch.Tensor) and state.is_cuda
    _same(got, want)
    _same_state(state, want_state)
    # what the binding and the library refuse
    d_color = torch.from_numpy(color).cuda()
    with pytest.raises(ValueError, match="exposure depth"):
        gpu.adapt(d_color, torch.from_numpy(depth[:, :5].copy()).cuda())
    with pytest.raises(ValueError, match="exposure: state must be a contiguous CUDA tensor of 1040 bytes"):
        gpu.adapt(d_color, state=torch.zeros(259, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="exposure: out must be"):
        gpu.adapt(d_color, out=torch.empty(67, 130, 4, device="cuda"))
    with pytest.raises(hip.HipError, match="the permilles must be 0 <= low < high <= 1000, not 950 and 950"):
        gpu.adapt(d_color, low_permille=950)
    with pytest.raises(hip.HipError, match="the output overlaps the depth frame"):
        d_depth = torch.from_numpy(depth).cuda()
        gpu.adapt(d_color, d_depth, out=d_depth)
    with pytest.raises(hip.HipError, match="the state must be 16-byte aligned"):
        gpu.adapt(d_color, state=torch.zeros(262, dtype=torch.int32, device="cuda")[2:])


# ---- rendered frames ------------------------------------------------------------------------------------------------
RES = 32


def test_temporal_preview_with_exposure_scales_the_output_alone_and_none_changes_nothing(gpu):
    """cornell_box_spheres 32 x 32, mis at 4 spp, three frame()s with set_camera between them, at the preview's defaults
    (filtered).  ``exposure=None`` gives the bits of a preview built without the argument; with ``exposure=True`` each
    returned frame is that linear frame times exposure.read(state)["exposure"] in float32, bit for bit, and the
    accumulator and the history are bitwise the plain preview's."""
    import torch
    from vimg_amd import hip
    s = scenes.json_scene("cornell_box_spheres.json", res=(RES, RES))
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    plain, off, on = dev.temporal_preview(p, samples=4), dev.temporal_preview(p, samples=4, exposure=None), dev.temporal_preview(p, samples=4, exposure=True)
    assert plain.exposure is None and plain.exposure_state is None and off.exposure_state is None and on.exposure == {}
    assert gpu.read(on.exposure_state) == dict(exposure=1.0, frames=0, metered=0.0, counted=0)
    exposures = []
    for cam in (0, 1, 2):
        dev.set_camera(*orbit_camera(cam))
        linear, same, exposed = (x.frame().clone() for x in (plain, off, on))
        assert torch.equal(_ibits(same), _ibits(linear))
        assert torch.equal(_ibits(off.history.tensor), _ibits(plain.history.tensor))
        now = gpu.read(on.exposure_state)
        assert now["frames"] == cam + 1 and 0 < now["counted"] <= RES * RES
        assert torch.equal(_ibits(exposed), _ibits(linear * torch.tensor(now["exposure"], dtype=torch.float32, device="cuda")))
        assert not torch.equal(_ibits(exposed), _ibits(linear))
        # exposure is the last stage, on the output only: what carries on to the next frame is linear
        assert torch.equal(_ibits(on.history.tensor), _ibits(plain.history.tensor))
        a, b = on.acc.state(), plain.acc.state()
        assert all(torch.equal(_ibits(a[k]), _ibits(b[k])) for k in ("sum", "count", "batches", "m2"))
        # ... and it is the restatement's, carried from frame to frame
        want_state = R.adapt(linear.cpu().numpy(), state=want_state if exposures else None)[1]
        _same_state(on.exposure_state, want_state)
        exposures.append(now["exposure"])
    assert len(set(exposures)) == 3
    # reset() zeroes the state
    state = on.exposure_state
    on.reset()
    assert on.exposure_state is state and not _state_bytes(state).any()
    # a dict: the parameters; anything else is refused
    keyed = dev.temporal_preview(p, samples=4, exposure=dict(key=0.36))
    assert keyed.exposure == dict(key=0.36)
    plain.reset()
    linear, exposed = plain.frame().clone(), keyed.frame().clone()
    _same(exposed.cpu().numpy(), R.adapt(linear.cpu().numpy(), key=0.36)[0])
    with pytest.raises(ValueError, match="temporal_preview: exposure must be"):
        dev.temporal_preview(p, exposure=2)
    with pytest.raises(TypeError, match="exposure: unknown parameters"):
        dev.temporal_preview(p, exposure=dict(max_history=4))
    for x in (plain, off, on, keyed):
        x.close()
    dev.close()


def test_render_denoised_with_exposure_is_the_plain_call_scaled_to_its_own_target(gpu):
    import torch
    from vimg_amd import hip
    s = scenes.json_scene("cornell_box_spheres.json", res=(RES, RES))
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    plain = dev.render_denoised(p)
    assert torch.equal(_ibits(dev.render_denoised(p, exposure=None)), _ibits(plain))
    assert torch.equal(_ibits(dev.render_denoised(p, exposure=False)), _ibits(plain))
    _same(dev.render_denoised(p, exposure=True).cpu().numpy(), R.adapt(plain.cpu().numpy())[0])
    out = torch.empty_like(plain)
    assert dev.render_denoised(p, out=out, exposure=dict(key=0.5, high_permille=1000)) is out
    _same(out.cpu().numpy(), R.adapt(plain.cpu().numpy(), key=0.5, high_permille=1000)[0])
    with pytest.raises(ValueError, match="render_denoised: exposure must be"):
        dev.render_denoised(p, exposure="yes")
    dev.close()
