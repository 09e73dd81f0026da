"""Late builds of render_cu_kernel do not queue a shadow ray whose light sample adds exactly (0, 0, 0)
(render_cu_kernel.h: cu_vertex, ELIDE).  The occlusion answer of such a ray decides between
`result + 0` and `result`, and `result` is never -0, so the frame keeps its bits; the reference traced the ray,
so the counts keep counting it.  Early builds (the ray is queued before its contribution is known), the
statistics build (its node and primitive counts are the reference's) and the lane-bound kernel walk every
shadow ray: all five frames must be one frame, on scenes with none, some and only such rays."""
import re

import numpy as np
import pytest

import scenes

PLAIN_NAME, GENERAL_NAME = "render_cu_kernel<false>", "render_cu_kernel<false,general>"
WOULD_ELIDE = re.compile(r"\[vimg walk\] would-elide shadow rays (\d+) of (\d+)")


# ---------------------------------------------------------------------------------------------- CPU
def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def test_adding_a_signed_zero_to_a_sum_that_started_at_plus_zero_changes_no_bit():
    """The lemma the elision rests on, in numpy float32 (round to nearest, as the kernels): r + (+-0) has r's
    bits for every r but -0, and a running sum started at +0 never is -0 - a sum is -0 only if both operands are."""
    f32 = np.float32
    tiny = np.array([1], dtype=np.uint32).view(np.float32)[0]
    with np.errstate(over="ignore"):
        for r in (f32(0.0), tiny, f32(1.0), f32(-1.0), np.finfo(np.float32).max, f32(np.inf)):
            for z in (f32(0.0), f32(-0.0)):
                s = np.add(r, z, dtype=np.float32)
                assert _bits(s) == _bits(r), (r, z)
        # (the one value the lemma excludes: -0 + +0 is +0)
        assert _bits(np.add(f32(-0.0), f32(0.0), dtype=np.float32)) != _bits(f32(-0.0))
        rng = np.random.default_rng(11)
        minus_zero = _bits(f32(-0.0))
        for trial in range(64):
            n = 200
            vals = rng.standard_normal(n).astype(np.float32) * f32(10.0) ** rng.integers(-30, 30, n).astype(np.float32)
            kind = rng.integers(0, 4, n)
            vals[kind == 0] = f32(0.0)
            vals[kind == 1] = f32(-0.0)
            if trial % 2:   # exact cancellations too: each value followed by its negative
                vals[1::2] = -vals[0::2]
            acc = f32(0.0)
            for v in vals:
                acc = np.add(acc, v, dtype=np.float32)
                assert _bits(acc) != minus_zero
                for z in (f32(0.0), f32(-0.0)):
                    assert _bits(np.add(acc, z, dtype=np.float32)) == _bits(acc)


def light_behind_scene(res=(48, 48)):
    """A Lambertian floor and one Lambertian sphere under a one-sided light quad that faces UP, away from all
    geometry: every light sample sees the emitter from behind (light_col == 0), so every shadow ray's
    contribution is exactly zero.  The camera looks down from above the light and sees its front."""
    import vimg_amd
    from vimg_amd import abi
    s = vimg_amd.HostScene()
    s.set_camera((0.0, 6.0, 5.0), (0.0, 0.6, 0.0), (0, 1, 0), 40.0, res)
    s.set_render_defaults("mis", 8, 8)
    t_floor = s.add_texture_const((0.7, 0.7, 0.7))
    t_ball = s.add_texture_const((0.8, 0.3, 0.2))
    m_floor = s.add_material("lambertian", tex=t_floor)
    m_ball = s.add_material("lambertian", tex=t_ball)
    m_light = s.add_material("diffuse_light", emit=(10.0, 9.0, 8.0))

    def quad(scale, rot_x_deg, trans):   # the unit quad faces +z; column-major transform
        a = np.deg2rad(rot_x_deg)
        r = np.array([[1, 0, 0, 0], [0, np.cos(a), -np.sin(a), 0], [0, np.sin(a), np.cos(a), 0], [0, 0, 0, 1]], dtype=np.float32)
        t = np.eye(4, dtype=np.float32)
        t[:3, 3] = trans
        return (t @ r @ np.diag([scale[0], scale[1], 1, 1]).astype(np.float32)).T.reshape(16)

    s.add_quad(quad((4, 4), -90, (0, 0, 0)), m_floor)          # floor, normal +y
    s.add_quad(quad((0.7, 0.7), -90, (0.0, 2.5, 0.0)), m_light)   # light, normal +y: its back to floor and sphere
    s.add_sphere((0.9, 0.5, 0.6), 0.5, m_ball)
    s.build_bvh(abi.BVH_SWEEP)
    return s


CASES = {
    "disney": (lambda: scenes.json_scene("disney_spheres.json", res=(96, 48)), 16),
    "cornell": (lambda: scenes.json_scene("cornell_box_spheres.json", res=(64, 64)), 8),
    "glass": (lambda: scenes.json_scene("glass_in_box.json", res=(48, 48)), 8),
    "light_behind": (light_behind_scene, 8),
}


@pytest.fixture(scope="module")
def oracle_frames():
    """The CPU restatement's frame and counts, once per scene."""
    import oracle_lib as O
    out = {}
    for name, (make, spp) in CASES.items():
        s = make()
        p = s.default_params(samples=spp)
        img, st, _ = O.render(s, p)
        out[name] = (s, p, img, st)
    return out


def test_the_built_scene_has_shadow_rays_and_light_only_from_the_emitters_front(oracle_frames):
    """What the GPU test of `light_behind` relies on, on the CPU: the reference traces shadow rays there, and the
    frame is black except where the camera sees the emitter's front (no light sample ever adds anything)."""
    s, p, img, st = oracle_frames["light_behind"]
    assert st.shadow_rays > 0 and st.nan_samples == 0
    lit = img.max(axis=-1) > 0
    assert 0 < lit.sum() < lit.size // 8
    # every lit pixel shows the emitter itself: its colour's ratios, and nothing dimmer than partial coverage
    ys, xs = np.nonzero(lit)
    assert np.allclose(img[lit] / img[lit][:, :1], np.array([10.0, 9.0, 8.0], dtype=np.float32) / 10.0, rtol=1e-5)
    assert ys.max() - ys.min() < img.shape[0] // 2 and xs.max() - xs.min() < img.shape[1] // 2   # one compact patch


# ---------------------------------------------------------------------------------------------- GPU
def _frame(d, p):
    import torch
    img = d.render(p, stats=False)
    torch.cuda.synchronize()
    d.check()
    return img


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_five_builds_render_one_frame_and_the_counts_stay_the_references(case, oracle_frames, monkeypatch, capfd):
    """Late PLAIN (cu_flex = 1: k_cu_plain*.hip), late general (the same under VIMG_HIP_PLAIN=0: k_cu.hip), early
    (cu_flex = 1 | 32), statistics (render(stats=True): k_cu_diag.hip, which elides nothing) and lane-bound frames
    are torch.equal; rays, shadow_rays and nan_samples of the statistics launch are the oracle's; and the
    statistics build's count of the rays a late build would not have queued (printed under VIMG_HIP_DIAG) is
    10 - 25 % of the shadow rays on disney_spheres (17.6 % at 450 x 200, 16 spp on the CPU), all of them on
    the scene whose light faces away, and at most the shadow rays elsewhere.  Measured on an MI355X: 32 522 of
    182 151 (17.85 %) on disney_spheres, 30 509 of 113 958 on cornell, 27 596 of 87 873 on glass_in_box (its walls
    take light samples; only the dielectric's vertices take none), 15 442 of 15 442 on the built scene."""
    import torch
    from test_plain_build import _dev
    s, p, cpu_img, cpu_st = oracle_frames[case]
    late, general = _dev(s, cu_flex=1), _dev(s, general=True, cu_flex=1)
    early, lane = _dev(s, cu_flex=1 | 32), _dev(s, scheduler="lane")
    # every scene here is untextured with its tree in LDS: the late and the early device run a PLAIN build (with the
    # fourth ring on glass_in_box, whose dielectric is a material of class 3), the override the general one
    assert late.kernel_for(p) == PLAIN_NAME and early.kernel_for(p) == PLAIN_NAME
    assert late.plain_fold_for(p) != 0 and early.plain_fold_for(p) != 0
    assert general.kernel_for(p) == GENERAL_NAME and general.plain_fold_for(p) == 0
    a = _frame(late, p)
    assert bool(torch.isfinite(a).all()) and float(a.max()) > 0
    for name, d in (("general", general), ("early", early), ("lane", lane)):
        assert torch.equal(a.view(torch.int32), _frame(d, p).view(torch.int32)), name
    monkeypatch.setenv("VIMG_HIP_DIAG", "1")
    capfd.readouterr()
    img, st = late.render(p)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    monkeypatch.delenv("VIMG_HIP_DIAG")
    assert torch.equal(a.view(torch.int32), img.view(torch.int32)), "statistics"
    assert (st.rays, st.shadow_rays, st.nan_samples) == (cpu_st.rays, cpu_st.shadow_rays, cpu_st.nan_samples)
    m = WOULD_ELIDE.search(err)
    assert m, err
    would, of = int(m.group(1)), int(m.group(2))
    print(f"{case}: would-elide {would} of {of} shadow rays ({100.0 * would / max(of, 1):.2f} %)")
    assert of == st.shadow_rays and would <= st.shadow_rays
    if case == "disney":
        assert 0.10 * st.shadow_rays <= would <= 0.25 * st.shadow_rays
    elif case == "light_behind":
        assert st.shadow_rays > 0 and would == st.shadow_rays
        lit = cpu_img.max(axis=-1) > 0
        assert bool((a.cpu().numpy()[~lit] == 0).all())
    # (glass_in_box, cornell: the relation above is all that is asserted of the count)
    for d in (late, general, early, lane):
        d.close()
