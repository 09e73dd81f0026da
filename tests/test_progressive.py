"""Progressive rendering (vimg_hip_progressive_*, DeviceScene.progressive): a frame's samples added a few at
a time give, after every increment, exactly the bits of one render at the running total - on every scheduler
configuration of the product library, with and without statistics, on every feature, for shards, and for
accumulators that share a scene."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import scenes
from test_gpu_parity import FEATURE_CASES, SCHEDULES, _compare_images, scheduler_scene

pytestmark = pytest.mark.gpu

STATS_FIELDS = ("paths", "closest_rays", "shadow_rays", "internal_visits", "leaf_visits", "prim_tests",
                "sphere_tests", "nan_samples")


def _dev(s, **opts):
    from vimg_amd import hip
    return hip.DeviceScene(s, **opts)


def _params(p, **kw):
    from vimg_amd import abi
    q = abi.RenderParams.from_buffer_copy(p)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _bits(img):
    a = img.cpu().numpy() if hasattr(img, "cpu") else np.asarray(img)
    return np.ascontiguousarray(a).view(np.uint32)


def _one_shot(d, p, total, stats=False):
    return d.render(_params(p, samples=total), stats=stats)


def _check_increments(d, p, incs, refs, what, stats=False):
    """Renders `incs` on a fresh accumulator of `d`; after each prefix the image must be refs[total]."""
    acc = d.progressive(p)
    total, summed = 0, {k: 0 for k in STATS_FIELDS}
    for n in incs:
        r = acc.render(n, stats=stats)
        img = r[0] if stats else r
        total += n
        assert acc.samples == total
        assert np.array_equal(_bits(img), _bits(refs[total])), (what, incs, total)
        if stats:
            for k in STATS_FIELDS:
                summed[k] += getattr(r[1], k)
    acc.close()
    return summed


@pytest.mark.parametrize("scene_name", ["disney_spheres.json", "glass_in_box.json", "feature"])
def test_increments_give_the_one_shot_bits_on_every_schedule(scene_name):
    """Every configuration of SCHEDULES (lane, the CU scheduler by policy, 5 / 2 / 3 segments, few and tiny
    pools, early and late rays ...): increments [1, 3, 4] (plain builds) and [5, 2, 1] (statistics builds),
    whose boundaries miss the segment lengths, equal the one-shot render at every prefix; the summed
    statistics equal the one-shot render's."""
    s, p = scheduler_scene(scene_name)
    lane = _dev(s, scheduler="lane")
    refs = {t: _one_shot(lane, p, t) for t in (1, 4, 5, 7, 8)}
    _, ref_st = _one_shot(lane, p, 8, stats=True)
    for name, opts in SCHEDULES.items():
        d = _dev(s, **opts)
        assert np.array_equal(_bits(_one_shot(d, p, 8)), _bits(refs[8])), (scene_name, name)
        _check_increments(d, p, [1, 3, 4], refs, (scene_name, name, "plain"))
        summed = _check_increments(d, p, [5, 2, 1], refs, (scene_name, name, "statistics"), stats=True)
        assert summed == {k: getattr(ref_st, k) for k in STATS_FIELDS}, (scene_name, name)
        d.close()


@pytest.mark.parametrize("case", list(FEATURE_CASES))
def test_increments_on_every_feature(case):
    """Image textures, env map and lens (the TEX builds), trees in global memory and stacks deeper than their
    LDS rows (the DEEP builds), all four integrators: increments -> the one-shot bits."""
    s, kw = FEATURE_CASES[case]()
    p = s.default_params(**kw)
    n = p.samples
    incs = [1, 2, n - 3]
    for opts in (dict(scheduler="cu"), dict(scheduler="cu", pool_slots=8, pool_segments=3),
                 dict(scheduler="cu", lds_stack=1), dict(scheduler="cu", lds_budget_kb=1, lds_leaf=0),
                 dict(scheduler="cu", cu_flex=33, pool_segments=2), dict(scheduler="lane")):
        d = _dev(s, **opts)
        refs = {t: _one_shot(d, p, t) for t in (1, 3, n)}
        _check_increments(d, p, incs, refs, (case, opts))
        d.close()


def test_progressive_render_against_the_oracle():
    s = scenes.json_scene("disney_spheres.json", res=(96, 48))
    p = s.default_params(samples=8)
    acc = _dev(s).progressive(p)
    acc.render(3)
    img = acc.render(5).cpu().numpy()
    cpu, _, _ = O.render(s, p)
    _compare_images(img, cpu, "disney_spheres, 3 + 5 samples")


def test_statistics_of_the_increments_add_up():
    s = scenes.feature_scene(res=(72, 48), envmap=True, lens=True)
    p = s.default_params(samples=7, depth=7)
    d = _dev(s)
    _, one = d.render(p)
    acc = d.progressive(p)
    summed = {k: 0 for k in STATS_FIELDS}
    for n in (2, 4, 1):
        _, st = acc.render(n, stats=True)
        assert st.paths == 72 * 48 * n
        for k in STATS_FIELDS:
            summed[k] += getattr(st, k)
    assert summed == {k: getattr(one, k) for k in STATS_FIELDS}


@pytest.mark.parametrize("world", [2, 3])
def test_one_accumulator_per_shard(world):
    import torch
    from vimg_amd import dist as vdist
    s = scenes.json_scene("disney_spheres.json", res=(123, 61))
    for opts in (dict(scheduler="cu"), dict(scheduler="lane")):
        d = _dev(s, **opts)
        full = d.render(s.default_params(samples=6), stats=False)
        stride = vdist.shard_stride_pixels(123, 61, world)
        gathered = torch.zeros((world, stride, 3), dtype=torch.float32, device="cuda")
        accs = [d.progressive(s.default_params(tile_rank=r, tile_world=world)) for r in range(world)]
        for n in (2, 1, 3):            # ranks advanced in turn on one scene
            for r, acc in enumerate(accs):
                out = acc.render(n)
                assert out.shape == (d.shard_pixels(acc.params), 3)
                gathered[r, :out.shape[0]] = out
        img = d.assemble_shards(gathered, world, stride)
        assert torch.equal(img, full), (world, opts)
        for acc in accs:
            acc.close()


def test_accumulators_are_independent_and_reset_repeats():
    s = scenes.json_scene("cornell_box_spheres.json", res=(80, 80))
    d = _dev(s, scheduler="cu", pool_segments=3)
    pm = s.default_params(samples=1)
    pn = s.default_params(samples=1, integrator="material", depth=16)
    want_m = {t: _one_shot(d, pm, t) for t in (2, 5, 9)}
    want_n = {t: _one_shot(d, pn, t) for t in (3, 4, 9)}
    a, b = d.progressive(pm), d.progressive(pn)
    for (ka, kb) in ((2, 3), (3, 1), (4, 5)):     # alternately, different integrators
        ta, tb = a.samples + ka, b.samples + kb
        assert np.array_equal(_bits(a.render(ka)), _bits(want_m[ta]))
        # a plain render between two increments does not disturb the accumulators
        _one_shot(d, pm, 6)
        assert np.array_equal(_bits(b.render(kb)), _bits(want_n[tb]))
    a.reset()
    assert a.samples == 0
    for k, t in ((2, 2), (3, 5), (4, 9)):
        assert np.array_equal(_bits(a.render(k)), _bits(want_m[t]))


def test_errors_and_advance_only():
    from vimg_amd import abi, hip
    lib = abi.hip_lib()
    s = scenes.json_scene("disney_spheres.json", res=(40, 24))
    d, other = _dev(s), _dev(s)
    p = s.default_params(samples=4)
    want = {t: _one_shot(d, p, t) for t in (1, 3, 5)}
    acc = d.progressive(p)
    with pytest.raises(hip.HipError, match=r"\[-1\]"):
        acc.render(0)
    assert acc.render(1, out=False) is None      # NULL output: advances, writes nothing
    assert acc.samples == 1
    # the running total must stay a 32-bit sample count: refused on the host, nothing launched
    with pytest.raises(hip.HipError, match=r"\[-1\]"):
        acc.render(0xFFFFFFFF)
    assert acc.samples == 1
    assert np.array_equal(_bits(acc.render(2)), _bits(want[3]))
    # another scene's handle
    out = want[1].clone()
    assert lib.vimg_hip_progressive_render(other._h, acc._h, 1, C.c_void_p(out.data_ptr()), None, None) == -1
    assert b"another scene" in lib.vimg_hip_last_error()
    assert acc.samples == 3
    # NULL arguments
    h = C.c_void_p()
    assert lib.vimg_hip_progressive_create(None, C.byref(p), C.byref(h)) == -1 and not h
    assert lib.vimg_hip_progressive_create(d._h, None, C.byref(h)) == -1 and not h
    assert lib.vimg_hip_progressive_create(d._h, C.byref(p), None) == -1
    assert lib.vimg_hip_progressive_render(d._h, None, 1, None, None, None) == -1
    assert lib.vimg_hip_progressive_render(None, acc._h, 1, None, None, None) == -1
    assert lib.vimg_hip_progressive_reset(None) == -1
    assert lib.vimg_hip_progressive_samples(None) == 0
    assert lib.vimg_hip_progressive_free(None) == 0
    assert np.array_equal(_bits(acc.render(2)), _bits(want[5]))
    # bad parameters are refused at creation
    with pytest.raises(hip.HipError, match=r"\[-1\]"):
        d.progressive(s.default_params(tile_rank=2, tile_world=2))
    acc.close()
    with pytest.raises(hip.HipError, match="after close"):
        acc.render(1)
    acc.close()                                   # twice is harmless


def test_cli_progressive_png_is_the_plain_runs(tmp_path):
    import vimg_amd
    exe = os.path.join(vimg_amd.abi.PKG_DIR, "bin", "vimg-amd")
    scene = os.path.join(scenes.SCENES, "cornell_box_spheres.json")
    plain, prog = str(tmp_path / "plain.png"), str(tmp_path / "prog.png")
    r = subprocess.run([exe, "-f", scene, "-s", "6", "-c", "1", "-b", "1", "-o", plain],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, "-f", scene, "-s", "6", "-p", "4", "-c", "1", "-b", "1", "-o", prog],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "samples 4 / 6" in r.stdout and "samples 6 / 6" in r.stdout, r.stdout
    assert open(prog, "rb").read() == open(plain, "rb").read()
