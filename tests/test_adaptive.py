"""Adaptive sampling (vimg_hip_progressive_render_masked, _state, _error, _select; Progressive.render(mask=...),
.counts, .error, .state, .render_adaptive): after any sequence of masked and unmasked increments a pixel whose
count is N carries exactly the bits of one render at N samples - on every integrator, every scheduler
configuration, whole frames and shards, with and without statistics - and the per-pixel error is the float32
statistic include/vimg_hip.h states."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import scenes
from test_adaptive_abi import SEQUENCES, check_against_model, restatement_over, same_floats, stat_error, stat_update
from test_gpu_parity import SCHEDULES

pytestmark = pytest.mark.gpu

STATS_FIELDS = ("paths", "closest_rays", "shadow_rays", "internal_visits", "leaf_visits", "prim_tests",
                "sphere_tests", "nan_samples")
INTEGRATORS = ("s_normal", "g_normal", "material", "mis")
RES = (70, 44)          # ragged in both directions: tiles with slots off the image
# Above 2^20 items the list builder's scan (adapt_scan_kernel, 1024 workgroups of 1024 items per pass) takes a second
# pass and carries a total into it.  BIG: ragged in both directions, 138 x 128 tiles, 1 130 496 items, 1104 list
# workgroups; with 128 tile rows the items from 2^20 on are exactly the pixels with x >= 1024.  BIG_SHARD: every
# second tile of 225 x 150, 1 080 000 items, 1055 list workgroups.
BIG, BIG_SHARD = (1099, 1021), (1800, 1200)


def _dev(s, **opts):
    from vimg_amd import hip
    return hip.DeviceScene(s, **opts)


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _bits(img):
    return np.ascontiguousarray(_np(img)).view(np.uint32)


def _params(s, integrator, **kw):
    depth = {"material": 6}.get(integrator)
    return s.default_params(integrator=integrator, **({"depth": depth} if depth else {}), **kw)


def _shard_valid(res, world, rank):
    """Which slots of the shard's compact buffer are pixels (ragged tiles have slots off the image), and their
    (x, y)."""
    w, h = res
    tx_n, ty_n = (w + 7) // 8, (h + 7) // 8
    tiles = np.arange(rank, tx_n * ty_n, world)
    item = np.arange(tiles.size * 64)
    tile, within = tiles[item >> 6], item & 63
    x, y = (tile // ty_n) * 8 + (within & 7), (tile % ty_n) * 8 + (within >> 3)
    return (x < w) & (y < h), x, y


class _Refs:
    """One render per count N on a lane-bound device, in the accumulator's layout (every scheduler gives these
    bits: tests/test_gpu_parity.py)."""

    def __init__(self, s, integrator, world, rank):
        self.s, self.integrator, self.world, self.rank = s, integrator, world, rank
        self.dev = _dev(s, scheduler="lane")
        self.cache = {}

    def at(self, n):
        if n not in self.cache:
            p = _params(self.s, self.integrator, samples=int(n), tile_world=self.world, tile_rank=self.rank)
            self.cache[n] = _np(self.dev.render(p, stats=False)).copy()
        return self.cache[n]


def _check_contract(img, counts, refs, valid, what):
    """Every pixel of `img` is the reference render's at that pixel's own count; none is left out."""
    img, counts = _np(img), _np(counts)
    checked = np.zeros(counts.shape, dtype=bool)
    for n in np.unique(counts[valid]):
        at = valid & (counts == n)
        want = refs.at(n)[at] if n else np.zeros((int(at.sum()), 3), dtype=np.float32)
        assert np.array_equal(_bits(img[at]), _bits(want)), (what, "count", int(n))
        checked |= at
    assert np.array_equal(checked, valid), what
    assert (counts[~valid] == 0).all(), what


def _masks(shape, seed):
    """The calls of the sequence: overlapping random masks, one of zeros, one of ones."""
    rng = np.random.default_rng(seed)
    a = (rng.random(shape) < 0.6).astype(np.uint8)
    b = (rng.random(shape) < 0.5).astype(np.uint8)
    c = (rng.random(shape) < 0.3).astype(np.uint8)
    return [(a, 2), (np.zeros(shape, np.uint8), 3), (b, 1), (np.ones(shape, np.uint8), 2), (c, 1)]


def _run_sequence(d, s, integrator, world, rank, stats, refs, what, oracle_pixels=0, res=RES, calls=None,
                  check_after=(2, 4), then=None):
    """One sequence of masked calls on a fresh accumulator, every pixel checked against the library's own one-shot
    render at its count.  The oracle's trace_pixel is asked for a handful of pixels of whole frames only (shards,
    and the schedules other than lane and cu, are held to that one-shot render, which tests/test_gpu_parity.py
    holds to the oracle).  `calls(shape, valid)` gives another sequence of (mask or None, n) than _masks', checked
    against the one-shot renders after the calls of `check_after`; `then(acc, valid)` runs on the accumulator the
    sequence leaves."""
    import torch
    p = _params(s, integrator, tile_world=world, tile_rank=rank)
    acc = d.progressive(p)
    shape = acc.pixel_shape
    if world == 1:
        valid = np.ones(shape, dtype=bool)
    else:
        valid = _shard_valid(res, world, rank)[0]
    expect = np.zeros(shape, dtype=np.int64)
    n_old, k_old, m2_old = np.zeros(shape, np.uint32), np.zeros(shape, np.uint32), np.zeros(shape, np.float32)
    s_old = np.zeros(shape + (3,), np.float32)
    paths = 0
    for i, (mask, n) in enumerate(_masks(shape, 1234 + world) if calls is None else calls(shape, valid)):
        # numpy masks are copied up, CUDA tensors are used where they are
        m = mask if i % 2 == 0 or mask is None else torch.from_numpy(mask).cuda()
        launches = acc.launches
        r = acc.render(n, mask=m, stats=stats)
        img = r[0] if stats else r
        sel = ((mask != 0) & valid) if mask is not None else valid
        classes = np.unique(expect[sel]).size
        assert acc.launches - launches == classes, (what, i)     # one launch per distinct count among the selected
        expect[sel] += n
        if stats:
            paths += r[1].paths
            assert r[1].paths == int(sel.sum()) * n, (what, i)
        st = acc.state()
        counts = _np(st["count"]).astype(np.int64)
        assert np.array_equal(counts, expect), (what, i)
        assert np.array_equal(_np(acc.counts()), _np(st["count"])), (what, i)
        # 4. the statistic: state() through the numpy restatement gives K, M2 and error() bit for bit
        s_new = _np(st["sum"])
        n_new, k_new, m2_new = stat_update(n_old, k_old, m2_old, s_old, s_new, n, sel)
        assert np.array_equal(n_new, counts), (what, i)
        assert np.array_equal(_np(st["batches"]).astype(np.uint32), k_new), (what, i)
        assert same_floats(_np(st["m2"]), m2_new), (what, i)
        err = _np(acc.error())
        want_err = np.where(valid, stat_error(n_new, k_new, m2_new, s_new), np.float32(0))
        assert same_floats(err, want_err), (what, i)
        assert np.array_equal(s_new[~sel], s_old[~sel]), (what, i)       # unselected pixels keep their sums
        n_old, k_old, m2_old, s_old = n_new, k_new, m2_new, s_new
        if i == 2 and calls is None:
            assert np.unique(counts[valid]).size >= 4 and (counts[valid] == 0).any(), (what, "four counts with 0")
        if i in check_after:
            _check_contract(img, counts, refs, valid, (what, i))
    assert np.unique(expect[valid]).size >= 4
    if stats:
        assert paths == int(expect[valid].sum()), what             # 3. the paths of the calls add up to sum_p N_p
    if oracle_pixels and world == 1:
        w, h = res
        rng = np.random.default_rng(99)
        img = _np(img)
        for x, y in [(0, 0), (w - 1, h - 1), (w // 2, h // 2)] + [(int(rng.integers(w)), int(rng.integers(h)))
                                                               for _ in range(oracle_pixels)]:
            n = int(expect[h - 1 - y, x])
            ref = O.trace_pixel(s, _params(s, integrator, samples=n), x, y)
            print(f"oracle pixel ({x}, {y}) at N = {n}: gpu {img[h - 1 - y, x]} oracle {ref}")
            assert np.array_equal(_bits(img[h - 1 - y, x]), _bits(ref)), (what, x, y, n)
    if then:
        then(acc, valid)
    acc.close()


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_every_pixel_is_the_render_at_its_own_count(integrator):
    """1, 3, 4.  A seeded sequence of five (mask, n) calls - overlapping masks, all zeros, all ones - on every
    configuration of SCHEDULES; whole frame and a shard of two, with and without statistics (alternating over the
    configurations so that each schedule sees both and each (layout, statistics) pair is seen by many)."""
    s = scenes.json_scene("disney_spheres.json", res=RES)
    refs = {1: _Refs(s, integrator, 1, 0), 2: _Refs(s, integrator, 2, 1)}
    for i, (name, opts) in enumerate(SCHEDULES.items()):
        d = _dev(s, **opts)
        for world, rank, stats in ((1, 0, i % 2 == 0), (2, 1, i % 2 == 1)):
            _run_sequence(d, s, integrator, world, rank, stats, refs[world], (integrator, name, world, stats),
                          oracle_pixels=3 if name in ("lane", "cu") else 0)
        d.close()


@pytest.mark.parametrize("sched", ["cu", "lane"])
def test_statistics_and_plain_launches_on_both_layouts(sched):
    """The (layout, statistics) pairs the alternation above does not give the two main schedules."""
    s = scenes.json_scene("cornell_box_spheres.json", res=RES)
    d = _dev(s, scheduler=sched)
    for world, rank in ((1, 0), (2, 0)):
        refs = _Refs(s, "mis", world, rank)
        for stats in (False, True):
            _run_sequence(d, s, "mis", world, rank, stats, refs, (sched, world, stats))


def test_unmasked_paths():
    """2.  A mask of ones is the unmasked increment, bit for bit in image and counters; a call without a mask after
    masked ones continues every pixel from its own count."""
    s = scenes.json_scene("disney_spheres.json", res=RES)
    d = _dev(s)
    p = _params(s, "mis")
    a, b = d.progressive(p), d.progressive(p)
    ones = np.ones(a.pixel_shape, np.uint8)
    for n in (3, 2):
        ia, sa = a.render(n, stats=True)
        ib, sb = b.render(n, mask=ones, stats=True)
        assert np.array_equal(_bits(ia), _bits(ib))
        assert {k: getattr(sa, k) for k in STATS_FIELDS} == {k: getattr(sb, k) for k in STATS_FIELDS}
        assert a.samples == b.samples and a.launches == b.launches
        for k, v in a.state().items():
            assert same_floats(_np(v), _np(b.state()[k])) if v.dtype.is_floating_point else np.array_equal(_np(v), _np(b.state()[k]))
    refs = _Refs(s, "mis", 1, 0)
    rng = np.random.default_rng(5)
    m1, m2 = (rng.random(ones.shape) < 0.5).astype(np.uint8), (rng.random(ones.shape) < 0.5).astype(np.uint8)
    a.render(1, mask=m1, out=False)
    a.render(2, mask=m2, out=False)
    expect = 5 + m1.astype(np.int64) + 2 * m2
    before = a.launches
    img = a.render(3)                          # no mask: everyone, each from its own count
    assert a.launches - before == np.unique(expect).size == 4
    expect += 3
    assert np.array_equal(_np(a.counts()), expect) and a.samples == expect.max()
    _check_contract(img, expect, refs, np.ones(ones.shape, bool), "unmasked after masked")


def test_a_pixel_of_constant_background_has_error_zero():
    """4.  One small sphere under a constant background: the top rows of the frame see only the background (the
    sphere, radius 0.5 at distance 5, covers +-6 of the +-30 degrees of the frame's height), so every sample of
    those pixels is the background colour and their error is exactly 0 after two increments, +inf before.
    (Increments of 2 and 2 and a colour of binary fractions: the sums are then exact and the batch mean and the
    means are the same float, scaling by 2 and 4 being exact - for other lengths Y(3 c) / 3 and Y(2 c) / 2 may
    differ in the last bit, and the error is then some 1e-8 instead of 0.)"""
    import vimg_amd
    bg = (0.25, 0.5, 0.75)
    s = vimg_amd.HostScene()
    s.set_camera((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), (0, 1, 0), 60.0, (48, 32))
    s.set_render_defaults("mis", 4, 8)
    s.add_sphere((0.0, 0.0, 0.0), 0.5, s.add_material("lambertian", tex=s.add_texture_const((0.6, 0.6, 0.6))))
    s.set_background_const(bg, add_to_lights=True)
    s.build_bvh(vimg_amd.abi.BVH_SWEEP)
    acc = _dev(s).progressive(s.default_params())
    acc.render(2, out=False)
    assert np.isinf(_np(acc.error())).all()
    img = _np(acc.render(2))
    st = acc.state()
    err = _np(acc.error())
    sky = slice(0, 8)
    assert (img[sky] == np.asarray(bg, np.float32)).all()
    assert (_np(st["batches"]) == 2).all() and (_np(st["count"]) == 4).all()
    assert (err[sky] == 0).all() and (_np(st["m2"])[sky] == 0).all()
    assert (err[12:20, 20:28] > 0).any()                     # the lit sphere is noisy
    assert same_floats(err, stat_error(_np(st["count"]), _np(st["batches"]), _np(st["m2"]), _np(st["sum"])))


def _adaptive_runs(d, p, refs, target, step, cap, what):
    """render_adaptive twice on fresh accumulators of `d`: what test_render_adaptive states, checked on each run;
    the first run's (image, counts)."""
    runs = []
    for _ in range(2):
        acc = d.progressive(p)
        steps = []
        img = acc.render_adaptive(target, step, cap, progress=lambda n, active: steps.append((n, active)))
        counts, err = _np(acc.counts()), _np(acc.error())
        assert len(steps) <= cap // step and steps[-1][0] == counts.max()
        assert [n for n, _ in steps] == [step * (i + 1) for i in range(len(steps))]
        assert acc.launches == len(steps)                       # one count class, one launch, per step
        active = [a for _, a in steps][2:]
        assert active == sorted(active, reverse=True)           # a pixel that dropped out stays out
        assert ((err <= target) | (counts == cap)).all()
        assert (counts % step == 0).all() and counts.min() >= 2 * step and counts.max() <= cap
        _check_contract(img, counts, refs, np.ones(counts.shape, bool), what)
        assert acc.select(target, cap)[1] == 0
        runs.append((_np(img).copy(), counts.copy()))
        acc.close()
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0])) and np.array_equal(runs[0][1], runs[1][1])
    assert np.unique(runs[0][1]).size > 1, "the target separates no pixels: the test shows nothing"
    return runs[0]


def test_render_adaptive():
    """5.  The driver terminates; every pixel ends at err <= target or count == max_samples; counts are multiples
    of step; the image is every pixel's render at its own count; two runs agree; one launch per step."""
    s = scenes.json_scene("disney_spheres.json", res=RES)
    d = _dev(s)
    p = _params(s, "mis")
    refs = _Refs(s, "mis", 1, 0)
    target, step, cap = 0.08, 4, 40
    runs = [_adaptive_runs(d, p, refs, target, step, cap, "render_adaptive")]
    # a shard runs the same loop on its own pixels
    acc = d.progressive(_params(s, "mis", tile_world=2, tile_rank=1))
    img = acc.render_adaptive(target, step, cap)
    valid, x, y = _shard_valid(RES, 2, 1)
    counts = _np(acc.counts())
    assert np.array_equal(counts[valid], runs[0][1][RES[1] - 1 - y[valid], x[valid]])
    assert np.array_equal(_bits(_np(img)[valid]), _bits(runs[0][0][RES[1] - 1 - y[valid], x[valid]]))
    with pytest.raises(ValueError):
        acc.render_adaptive(target, 4, 42)
    with pytest.raises(ValueError):
        acc.render_adaptive(target, 4, 40, min_samples=4)


_big = {}


def _big_frame():
    """The scene at BIG, its one-shot references and one device per scheduler, made once for the tests that share them
    (and never changed by them)."""
    if not _big:
        s = scenes.json_scene("disney_spheres.json", res=BIG)
        _big.update(s=s, refs=_Refs(s, "mis", 1, 0), cu=_dev(s, scheduler="cu"))
        _big["lane"] = _big["refs"].dev
    return _big


def _big_calls(shape, valid):
    """The calls that put the scan's second pass and its carry under _run_sequence's assertions.  The counts: after
    the third call 2 and 6 left of x = 1024, 1 and 5 right of it; the fifth call's n = 1 lifts list workgroup 1024
    (right) to 2 and 6, so those two classes of the last call have thousands of members before item 2^20 and 1024
    after it, while 1 and 5 lie wholly in the second pass; the two single items and the last pixel make two more
    classes of one member (3 or 7 left, 4 or 8 right).  Six distinct counts at the end.  (Left of x = 1024 only the
    first and third call and one item of the fifth change anything, so no choice of n gives every class members on
    both sides.)"""
    w, h = BIG
    ok, x, y = _shard_valid(BIG, 1, 0)
    assert ok.size == 1104 * 1024 and np.array_equal(x[ok] >= 1024, np.flatnonzero(ok) >= 1 << 20)
    at = lambda items: (h - 1 - y[items], x[items])          # an item's place in the image
    right = np.ascontiguousarray(np.broadcast_to(np.arange(w) >= 1024, shape))
    rng = np.random.default_rng(77)
    first = (rng.random(shape) < 0.6).astype(np.uint8)
    last = np.flatnonzero(ok)[-1]
    assert (x[last], y[last]) == (w - 1, h - 1)
    one = np.zeros(shape, np.uint8)
    one[at(last)] = 1
    # list workgroup 1024 whole; beside it one item each of 1023 and 1025: valid ones, the left one at count 2 or 6
    count3 = np.where(right, 1, 2) + 4 * first.astype(np.int64)
    group = np.zeros(shape, np.uint8)
    items = np.arange(1024 * 1024, 1025 * 1024)
    assert ok[items].all()
    group[at(items)] = 1
    for wg in (1023, 1025):
        items = np.arange(wg * 1024, (wg + 1) * 1024)
        group[at(items[ok[items]][:1])] = 1
    assert group.sum() == 1026 and set(np.unique(count3[group != 0])) <= {1, 2, 5, 6}
    return [(first, 4), (right.astype(np.uint8), 1), ((~right).astype(np.uint8), 2), (one, 3), (group, 1),
            (np.zeros(shape, np.uint8), 3), (None, 2)]


def _check_select(acc, valid):
    """vimg_hip_progressive_select pixel by pixel: ((err > target) & (N < max_samples)) | (K < 2) from error(),
    counts() and state(), 0 on a shard's off-image slots, and the returned number of ones."""
    err, counts = _np(acc.error()), _np(acc.counts())
    k = _np(acc.state()["batches"])
    finite = err[valid & np.isfinite(err)]
    assert finite.size
    for target in (0.0, float(np.median(finite)), float("inf")):
        for max_samples in (int(counts[valid].min()), int(counts[valid].max()) + 1):
            mask, active = acc.select(target, max_samples)
            want = (((err > np.float32(target)) & (counts < max_samples)) | (k < 2)) & valid
            assert np.array_equal(_np(mask), want.astype(np.uint8)), (target, max_samples)
            assert active == int(want.sum()), (target, max_samples)


@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("sched", ["cu", "lane"])
def test_a_frame_above_2_20_items(sched, stats):
    """The list of a class longer than one scan pass (BIG: 1104 list workgroups, 80 of them in the second pass):
    _big_calls' seven calls - a random mask, only the second pass, only the first, the last valid item alone, list
    workgroup 1024 with one item of each neighbour, nothing, everyone - under everything _run_sequence asserts after
    each call, the one-shot renders after the third and the last, the oracle for four pixels ((1098, 1020) among
    them), and select() pixel by pixel on the accumulator they leave."""
    b = _big_frame()
    _run_sequence(b[sched], b["s"], "mis", 1, 0, stats, b["refs"], (sched, stats), oracle_pixels=1, res=BIG,
                  calls=_big_calls, check_after=(2, 6), then=_check_select)


def test_render_adaptive_above_2_20_items():
    """test_render_adaptive's statements at BIG: every masked step builds a list through both scan passes."""
    b = _big_frame()
    _, counts = _adaptive_runs(b["cu"], _params(b["s"], "mis"), b["refs"], 0.08, 4, 24, "render_adaptive at BIG")
    assert counts[:, 1024:].max() > 8 and counts[:, :1024].max() > 8       # masked steps had members in both passes


def test_a_shard_above_2_20_items():
    """A shard whose own items pass 2^20 (BIG_SHARD, rank 1 of 2: 1055 list workgroups): _masks' five calls on cu.
    225 x 150 tiles cover the frame exactly, so this shard has no off-image slots; what they hold (count 0, error
    0, select mask 0) is asserted on the ragged shard of test_select_on_a_ragged_shard."""
    s = scenes.json_scene("disney_spheres.json", res=BIG_SHARD)
    d = _dev(s, scheduler="cu")
    assert _shard_valid(BIG_SHARD, 2, 1)[0].sum() == 1080000
    _run_sequence(d, s, "mis", 2, 1, True, _Refs(s, "mis", 2, 1), "shard above 2^20", res=BIG_SHARD, then=_check_select)


def test_select_on_a_ragged_shard():
    """select() pixel by pixel where a shard has slots off the image: those are 0 in the mask, the error and the
    counts, and are not counted."""
    s = scenes.json_scene("disney_spheres.json", res=RES)
    valid = _shard_valid(RES, 2, 1)[0]
    assert not valid.all()

    def then(acc, v):
        assert not _np(acc.error())[~v].any() and not _np(acc.counts())[~v].any()
        _check_select(acc, v)

    _run_sequence(_dev(s), s, "mis", 2, 1, False, _Refs(s, "mis", 2, 1), "select on a shard", then=then)


def test_twelve_classes_in_one_call():
    """Four striped masks with n = 1, 2, 4, 8 write the bits of x % 12 into the counts; the unmasked call that
    follows is twelve launches, one per class, and every pixel is the render at its own count."""
    s = scenes.json_scene("disney_spheres.json", res=RES)
    acc = _dev(s).progressive(_params(s, "mis"))
    want = np.broadcast_to(np.arange(RES[0]) % 12, acc.pixel_shape).astype(np.int64)
    for bit in range(4):
        acc.render(1 << bit, mask=((want >> bit) & 1).astype(np.uint8), out=False)
    assert np.array_equal(_np(acc.counts()), want) and np.unique(want).size == 12
    before = acc.launches                      # (1 + 2 + 4 + 4: the classes among the pixels each stripe selected)
    img = acc.render(1)
    assert acc.launches - before == 12
    assert np.array_equal(_np(acc.counts()), want + 1) and acc.samples == 12
    _check_contract(img, want + 1, _Refs(s, "mis", 1, 0), np.ones(want.shape, bool), "twelve classes")


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_the_statistic_of_a_long_run_against_float64(name):
    """A real accumulator through the 8 to 256 increments of SEQUENCES (up to 512 samples): the sums after every
    increment give the float64 model of tests/test_adaptive_abi.py, which holds the final M2 and error() by its derived
    bound; they are also the numpy restatement's bit for bit, and the image is the one-shot render at N."""
    ns = SEQUENCES[name]
    s = scenes.json_scene("cornell_box_spheres.json", res=(64, 64))
    d = _dev(s)
    acc = d.progressive(_params(s, "mis"))
    sums = [np.zeros(acc.pixel_shape + (3,), np.float32)]
    for i, n in enumerate(ns):
        img = acc.render(n, out=None if i == len(ns) - 1 else False)
        sums.append(_np(acc.state()["sum"]))
    st = acc.state()
    assert (_np(st["count"]) == sum(ns)).all() and (_np(st["batches"]) == len(ns)).all() and acc.launches == len(ns)
    m2, err = _np(st["m2"]), _np(acc.error())
    check_against_model(("device", name), np.stack(sums), ns, m2, err)
    _, _, m2_np, err_np = restatement_over(sums, ns)
    assert same_floats(m2, m2_np) and same_floats(err, err_np)
    want = d.render(_params(s, "mis", samples=sum(ns)), stats=False)
    assert np.array_equal(_bits(img), _bits(want))


def test_lifecycle_and_errors():
    """6.  reset clears counts and statistics; a geometry update makes the next masked call fail until reset; a
    call refused for its arguments leaves state() as it was."""
    import torch
    from vimg_amd import abi, hip
    lib = abi.hip_lib()
    s = scenes.json_scene("cornell_box_spheres.json", res=(48, 40))
    d, other = _dev(s), _dev(s)
    p = _params(s, "mis")
    acc = d.progressive(p)
    rng = np.random.default_rng(3)
    mask = (rng.random(acc.pixel_shape) < 0.5).astype(np.uint8)
    acc.render(2, mask=mask, out=False)
    acc.render(3, out=False)
    first = _np(acc.render(1, mask=mask)).copy()

    def snapshot():
        return {k: _np(v).copy() for k, v in acc.state().items()}, acc.samples, acc.launches

    def unchanged(snap):
        now = snapshot()
        return all(_bits(now[0][k]).tobytes() == _bits(snap[0][k]).tobytes() for k in snap[0]) and now[1:] == snap[1:]

    snap = snapshot()
    dmask = torch.from_numpy(mask).cuda()
    out = torch.zeros(acc.pixel_shape + (3,), dtype=torch.float32, device="cuda")
    args = (C.c_void_p(dmask.data_ptr()), C.c_void_p(out.data_ptr()), None, None)
    # samples == 0, another scene's accumulator, NULL handles: VIMG_E_INVALID, nothing advanced
    with pytest.raises(hip.HipError, match=r"\[-1\]"):
        acc.render(0, mask=mask)
    assert lib.vimg_hip_progressive_render_masked(other._h, acc._h, 1, *args) == -1
    assert b"another scene" in lib.vimg_hip_last_error()
    assert lib.vimg_hip_progressive_render_masked(d._h, None, 1, *args) == -1
    assert lib.vimg_hip_progressive_render_masked(None, acc._h, 1, *args) == -1
    # a selected pixel's count would pass UINT32_MAX (masked: judged on the selected pixels; unmasked: on all)
    with pytest.raises(hip.HipError, match=r"\[-1\].*2\^32"):
        acc.render(0xFFFFFFFF - 2, mask=mask)
    with pytest.raises(hip.HipError, match=r"\[-1\].*2\^32"):
        acc.render(0xFFFFFFFF - 2)
    with pytest.raises(hip.HipError, match=r"\[-1\]"):
        acc.select(float("nan"), 8)
    with pytest.raises(ValueError):
        acc.render(1, mask=mask[:-1])
    with pytest.raises(ValueError):
        acc.render(1, mask=mask.astype(np.float32))
    assert unchanged(snap) and not out.any()
    # the scene changes: refused until reset
    verts = torch.from_numpy(np.ascontiguousarray(
        np.ctypeslib.as_array(s.view.contents.vertices, shape=(d.num_vertices, 3)).copy())).cuda()
    d.update_geometry(vertices=verts)           # (the same positions: a new generation all the same)
    with pytest.raises(hip.HipError, match=r"\[-1\].*reset"):
        acc.render(1, mask=mask)
    with pytest.raises(hip.HipError, match=r"\[-1\].*reset"):
        acc.render(1)
    assert unchanged(snap)
    acc.reset()
    st = acc.state()
    assert acc.samples == 0 and acc.launches == 0 and not any(_np(v).any() for v in st.values())
    assert np.isinf(_np(acc.error())).all()
    assert not _np(acc.render(1, mask=np.zeros_like(mask))).any()       # count 0: written 0 0 0
    acc.render(2, mask=mask, out=False)
    acc.render(3, out=False)
    again = _np(acc.render(1, mask=mask))
    assert np.array_equal(_bits(again), _bits(first))                    # the same sequence, the same bits
    acc.close()
    with pytest.raises(hip.HipError, match="after close"):
        acc.counts()


def test_cli_adaptive(tmp_path):
    import vimg_amd
    exe = os.path.join(vimg_amd.abi.PKG_DIR, "bin", "vimg-amd")
    scene = os.path.join(scenes.SCENES, "cornell_box_spheres.json")
    a, b = str(tmp_path / "a.png"), str(tmp_path / "b.png")
    outs = []
    for o in (a, b):
        r = subprocess.run([exe, "-f", scene, "-s", "24", "-p", "4", "-e", "0.05", "-c", "1", "-b", "1", "-o", o],
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "samples 4 / 24, active pixels" in r.stdout and "samples 8 / 24, active pixels" in r.stdout, r.stdout
        outs.append([l.split(" (")[0] for l in r.stdout.splitlines() if "active pixels" in l])     # (without the times)
    assert outs[0] == outs[1] and open(a, "rb").read() == open(b, "rb").read()
