"""The leaf records of a PLAIN launch once more per major axis of a ray (plain_build.h: PF_LEAF_PERM,
render_cu_kernel.h: stage_leaf_perm, render_kernels.h: tri_vertex): a lane reads the copy made for its ray's kz, whose
triangles' vertices are already permuted, and the watertight test permutes nothing.  permute(p - o, kz) and
permute(p, kz) - permute(o, kz) are the same subtractions of the same operands, so every frame must be, bit for bit,
the general build's (VIMG_HIP_PLAIN=0) and the CPU oracle's: for rays of every major axis, on leaves that mix
triangles and spheres, on both PLAIN builds, after the scene was edited, on shards and progressive increments.  A
scene without triangles stages no copy."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import scenes
from test_lds_tables import GENERAL_NAME, PLAIN_NAME, _bits, _dev, _filled_scene, _frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "v-img_amd", "csrc")
RES, SPP = (64, 48), 4
SCENE_FILES = ["cornell_box_spheres.json", "disney_spheres.json", "empty_box.json"]
AXES = {"own": None, "+x": (1, 0, 0), "-x": (-1, 0, 0), "+y": (0, 1, 0), "-y": (0, -1, 0), "+z": (0, 0, 1), "-z": (0, 0, -1)}


def _scene(name, axis=None, res=RES):
    """The scene with its own camera, or with one inside its triangles' bounds that looks along `axis`."""
    s = scenes.json_scene(name, res=res)
    if axis is not None:
        v, _, _ = s.geometry()
        lo, hi = v.min(0), v.max(0)
        mid, ext = 0.5 * (lo + hi), hi - lo
        d = np.asarray(axis, dtype=np.float64)
        eye = mid - 0.45 * ext * d
        up = (0, 0, 1) if axis[1] else (0, 1, 0)
        s.set_camera(tuple(eye), tuple(eye + d), up, 70.0, res)
    return s


def _plain_general_oracle(s, p, **opts):
    """The frame of the default upload (which must run the PLAIN kernel), of the general build and of the oracle."""
    plain, general = _dev(s, **opts), _dev(s, general=True, **opts)
    assert plain.kernel_for(p) == PLAIN_NAME and general.kernel_for(p) == GENERAL_NAME
    a, b = _frame(plain, p), _frame(general, p)
    plain.close(), general.close()
    cpu, _, _ = O.render(s, p)
    return a, b, cpu


# ---------------------------------------------------------------------------------------------- CPU
PROGRAM = r"""
#include <cstdio>
#include "plain_build.h"
int main() {
  using namespace vimg;
  int bad = 0;
  auto expect = [&](const char* what, bool got, bool want) { if (got != want) { std::printf("wrong: %s\n", what); ++bad; } };
  static_assert(PF_LEAF_PERM != 0u && (PF_LEAF_PERM & (PF_LEAF_PERM - 1u)) == 0u, "one bit");
  static_assert((PF_LEAF_PERM & (PF_INTEGRATOR | PF_CLASSES | PF_LEAF_LDS | PF_SINGLE | PF_ITEMS | PF_FLEX | PF_TABLES)) == 0u, "a bit of its own");
  expect("copies staged serve", plain_leaf_perm_serves(1u, PF_LEAF_PERM), true);
  expect("copies missing do not serve", plain_leaf_perm_serves(0u, PF_LEAF_PERM), false);
  expect("bit unfolded does not ask (missing)", plain_leaf_perm_serves(0u, 127u), true);
  expect("bit unfolded does not ask (staged)", plain_leaf_perm_serves(1u, 127u), true);
  expect("nothing folded does not ask", plain_leaf_perm_serves(0u, 0u), true);
  expect("every bit folded asks", plain_leaf_perm_serves(0u, ~0u), false);
  expect("the default mask", plain_leaf_perm_serves(0u), (PLAIN_FOLD & PF_LEAF_PERM) == 0u);
  expect("the default mask, staged", plain_leaf_perm_serves(1u), true);
  // the other predicates do not read the bit
  expect("tables ignore the bit", plain_tables_serve(0u, PF_LEAF_PERM), true);
  std::printf("bad %d\n", bad);
  return bad;
}
"""


def test_the_predicate_of_the_permuted_copies(tmp_path):
    """plain_leaf_perm_serves (plain_build.h, compiled on its own): copies staged serve, copies missing do not, and a
    build that does not fold the bit does not ask."""
    src, exe = tmp_path / "perm.cpp", tmp_path / "perm"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++20", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "bad 0", r.stdout


# ---------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("axis", list(AXES))
@pytest.mark.parametrize("name", SCENE_FILES)
def test_every_major_axis_on_mixed_leaves(name, axis):
    """The scene's own camera and cameras that look along +-x, +-y, +-z from inside the box: primary rays of each kz on
    triangles, secondary rays of every direction (the scenes' own depth).  The early-ray PLAIN build (every pixel of
    a frame this small owns a slot) against the general build and the oracle."""
    s = _scene(name, AXES[axis])
    p = s.default_params(samples=SPP)
    assert p.depth >= 3
    a, b, cpu = _plain_general_oracle(s, p)
    exact = (_bits(a) == _bits(cpu)).all(axis=-1).mean()
    print(f"{name} {axis}: {exact * 100:.3f} % of the pixels are the oracle's bits, max |diff| {np.abs(a - cpu).max():.3e}")
    assert np.isfinite(a).all() and a.max() > 0
    assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(_bits(a), _bits(cpu))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box_spheres.json", "empty_box.json"])
def test_the_late_ray_build_at_test_size(name):
    """cu_flex = 1 by name keeps the policy from queueing rays early: k_cu_plain.hip against k_cu.hip, and the oracle."""
    s = _scene(name, AXES["+x"])
    p = s.default_params(samples=SPP)
    a, b, cpu = _plain_general_oracle(s, p, cu_flex=1)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(cpu))


@pytest.mark.gpu
def test_the_late_ray_build_on_the_flagship_launch():
    """disney_spheres at its own 1800 x 800 has more than three pools' worth of pixels per compute unit: the policy
    itself picks the late-ray build the benchmark times.  2 spp, compared on the GPU against the general build."""
    import torch
    s = scenes.json_scene("disney_spheres.json")
    p = s.default_params(samples=2)
    plain, general = _dev(s), _dev(s, general=True)
    assert plain.kernel_for(p) == PLAIN_NAME and general.kernel_for(p) == GENERAL_NAME
    a, b = plain.render(p, stats=False), general.render(p, stats=False)
    torch.cuda.synchronize()
    plain.check(), general.check()
    assert bool(torch.isfinite(a).all()) and float(a.max()) > 0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    plain.close(), general.close()


@pytest.mark.gpu
def test_a_scene_of_spheres_alone_runs_plain_on_the_oracles_bits():
    """No triangle, no copy: the three "copies" are the leaf table itself.  (The binding exposes nothing of a launch's
    LDS bytes; that the layout is the parent's is what the boundary search of test_lds_tables.py, which runs on
    sphere-only scenes, keeps checking.)"""
    s = _filled_scene(12, 2, RES)
    v, _, _ = s.geometry()
    assert len(v) == 0
    p = s.default_params(samples=SPP)
    a, b, cpu = _plain_general_oracle(s, p)
    assert a.max() > 0 and np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(cpu))


def _quad_scene(res):
    """42 quads (a floor, a light above it, forty slabs tilted every way) and a sphere: 85 leaf primitives, the most
    that leaves in LDS allow (85 x 48 bytes <= 4 KB)."""
    import vimg_amd
    s = vimg_amd.HostScene()
    s.set_camera((0.0, 3.0, 9.0), (0.0, 0.8, 0.0), (0, 1, 0), 40.0, res)
    s.set_render_defaults("mis", SPP, 8)
    t = [s.add_texture_const(c) for c in ((0.7, 0.6, 0.5), (0.3, 0.5, 0.8))]
    m_light = s.add_material("diffuse_light", emit=(14.0, 13.0, 11.0))
    mats = [s.add_material("lambertian", tex=t[0]), s.add_material("principled", tex=t[1], metallic=0.3, roughness=0.4)]

    def xf(scale, rx, ry, trans):
        a, b = np.deg2rad(rx), np.deg2rad(ry)
        r1 = np.array([[1, 0, 0, 0], [0, np.cos(a), -np.sin(a), 0], [0, np.sin(a), np.cos(a), 0], [0, 0, 0, 1]], dtype=np.float32)
        r2 = np.array([[np.cos(b), 0, np.sin(b), 0], [0, 1, 0, 0], [-np.sin(b), 0, np.cos(b), 0], [0, 0, 0, 1]], dtype=np.float32)
        m = np.eye(4, dtype=np.float32)
        m[:3, 3] = trans
        return (m @ r2 @ r1 @ np.diag([scale[0], scale[1], scale[2], 1]).astype(np.float32)).T.reshape(16)   # column-major

    s.add_quad(xf((6, 6, 1), -90, 0, (0, 0, 0)), mats[0])
    s.add_quad(xf((1.0, 0.8, 1), 90, 0, (0.0, 5.0, 0.5)), m_light)
    for i in range(40):
        s.add_quad(xf((0.35, 0.35, 1), 37 * i, 53 * i, ((i % 8 - 3.5) * 0.9, 0.5 + 0.7 * (i // 8 % 2), (i // 16) * 0.9 - 1.0)), mats[i % 2])
    s.add_sphere((0.0, 1.0, 2.0), 0.5, mats[1])
    s.build_bvh()
    return s


@pytest.mark.gpu
def test_copies_that_do_not_fit_send_the_launch_to_the_general_build():
    """85 leaf primitives: two copies of 4 080 bytes behind the tables.  The room is made scarce by sixteen walking
    waves and pool_slots by name (which lifts the policy's cap of 1 280) on a frame with more pixels per compute unit
    than slots fit, so the pool binds; the boundary is found through kernel_for alone, as in test_lds_tables.py:
    PLAIN beside the largest pool that fits, the general build beside eight slots more, the oracle's bits from both.
    (The frame has to be this large for the pool to bind at all: the policy never gives a launch more slots than it
    has pixels per compute unit.)"""
    res = (704, 432)
    s = _quad_scene(res)
    assert s.view.contents.bvh.max_depth + 2 <= 32       # (every stack row in LDS: not the DEEP build)
    p = s.default_params(samples=SPP)

    def plain(slots):
        d = _dev(s, cu_walkers=16, pool_slots=slots)
        name = d.kernel_for(p)
        d.close()
        assert name in (PLAIN_NAME, GENERAL_NAME)
        return name == PLAIN_NAME

    lo, hi = 1, 256            # pool slots in eights: 8 fit beside the copies, 2 048 do not fit the LDS at all
    assert plain(8 * lo) and not plain(8 * hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plain(8 * mid) else (lo, mid)
    slots = 8 * lo
    print(f"85 leaf primitives: the copies fit beside {slots} slots and not beside {slots + 8}")
    assert slots > 64
    cpu, _, _ = O.render(s, p)
    for n, want in ((slots, PLAIN_NAME), (slots + 8, GENERAL_NAME)):
        d = _dev(s, cu_walkers=16, pool_slots=n)
        assert d.kernel_for(p) == want
        gpu = _frame(d, p)
        d.close()
        assert np.array_equal(_bits(gpu), _bits(cpu)), (n, want)


@pytest.mark.gpu
def test_a_resident_scene_after_its_triangles_moved():
    """update_geometry moves the triangles and refits the tree on the GPU; the next launch stages its copies from the
    leaf records as they stand then: the frame of a fresh upload of the host scene edited and refit the same way."""
    from test_scene_update_host import apply_host, deformed
    make = lambda: _scene("cornell_box_spheres.json", AXES["-z"])     # noqa: E731
    s = make()
    p = s.default_params(samples=SPP)
    d = _dev(s)
    before = _frame(d, p)
    v, n, sp = deformed(s, seed=5, scale=0.03)
    d.update_geometry(vertices=v, normals=n, spheres=sp if len(sp) else None)
    h = apply_host(make(), v, n, sp)
    assert d.kernel_for(p) == PLAIN_NAME
    moved = _frame(d, p)
    fresh, general = _dev(h), _dev(h, general=True)
    assert fresh.kernel_for(p) == PLAIN_NAME and general.kernel_for(p) == GENERAL_NAME
    assert not np.array_equal(_bits(moved), _bits(before))
    assert np.array_equal(_bits(moved), _bits(_frame(fresh, p)))
    assert np.array_equal(_bits(moved), _bits(_frame(general, p)))
    cpu, _, _ = O.render(h, p)
    assert np.array_equal(_bits(moved), _bits(cpu))
    for x in (d, fresh, general):
        x.close()


@pytest.mark.gpu
def test_a_shard_and_a_progressive_pair_equal_the_single_launch():
    """tile_world = 2: both shards together are the whole frame's pixels; 2 + 2 samples in two launches are the frame
    at 4."""
    import torch
    s = _scene("cornell_box_spheres.json", AXES["+y"])
    d = _dev(s)
    p = s.default_params(samples=SPP)
    assert d.kernel_for(p) == PLAIN_NAME
    whole = _frame(d, p)
    general = _dev(s, general=True)
    shards = [s.default_params(samples=SPP, tile_world=2, tile_rank=rank) for rank in (0, 1)]
    stride = max(d.shard_pixels(ps) for ps in shards)
    gathered = torch.zeros((2, stride, 3), dtype=torch.float32, device="cuda")
    for rank, ps in enumerate(shards):
        assert d.kernel_for(ps) == PLAIN_NAME
        shard = d.render(ps, stats=False)
        torch.cuda.synchronize()
        d.check()
        assert shard.ndim == 2 and np.array_equal(_bits(shard.cpu().numpy()), _bits(_frame(general, ps)))
        gathered[rank, :shard.shape[0]] = shard
    assert np.array_equal(_bits(d.assemble_shards(gathered, 2, stride).cpu().numpy()), _bits(whole))
    acc = d.progressive(s.default_params(samples=1))
    acc.render(2)
    img = acc.render(2)
    torch.cuda.synchronize()
    d.check()
    assert np.array_equal(_bits(img.cpu().numpy()), _bits(whole))
    acc.close(), d.close(), general.close()
