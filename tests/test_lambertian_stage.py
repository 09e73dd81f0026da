"""The Lambertian vertex stage of render_cu_kernel (render_cu_kernel.h: cu_vertex<..., VIMG_MAT_LAMBERTIAN, ...>).

Its batches evaluate both directions of a vertex in line, from registers, instead of in the generic body's two-pass
loop over the slot's record; where rays are queued late they sample the light before the BSDF, from the generator
as it stands, instead of after it from a saved state.  None of that may move a bit: the smallest frames on which the
stage can go wrong - boxes whose every wall is Lambertian, a camera that
looks at a wall's back (no scatter, the shadow ray still traced), depths at which the vertex stage ends the paths -
under every build that holds the stage, against each other and against the CPU oracle."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import scenes
import vimg_amd
from test_gpu_parity import _compare_images
from test_plain_build import GENERAL_NAME, PLAIN_NAME, _dev

pytestmark = pytest.mark.gpu

# the red wall of both boxes is the plane x = 0 facing +x: from x = -800 every primary hit is on its back
BEHIND_THE_RED_WALL = {"from": [-800, 278, 278], "at": [278, 278, 278], "up": [0, 1, 0]}

# (scene, resolution, samples, depth or None for the file's, camera transform or None for the file's)
FRAMES = [(name, res, spp, None, None)
          for name in ("cornell_box_spheres.json", "empty_box.json") for res in ((16, 8), (24, 16)) for spp in (4, 16)]
FRAMES += [("empty_box.json", (24, 16), 4, None, BEHIND_THE_RED_WALL),
           ("cornell_box_spheres.json", (24, 16), 4, None, BEHIND_THE_RED_WALL),
           ("cornell_box_spheres.json", (24, 16), 16, 1, None),
           ("cornell_box_spheres.json", (24, 16), 16, 2, None),
           ("empty_box.json", (16, 8), 16, 2, None)]


def _id(f):
    name, res, spp, depth, cam = f
    return (f"{name.split('.')[0]}-{res[0]}x{res[1]}-{spp}spp" + (f"-depth{depth}" if depth else "") + ("-behind" if cam else ""))


def _scene(name, res, cam):
    with open(os.path.join(scenes.SCENES, name)) as f:
        d = json.load(f)
    d["camera"]["resolution"] = [int(res[0]), int(res[1])]
    if cam is not None:
        d["camera"]["transform"] = cam
    return vimg_amd.HostScene.from_json_text(json.dumps(d))


# the builds that hold the stage: the PLAIN build and the general build with rays queued late (the builds whole
# frames are timed on; an explicit cu_flex = 1 keeps the policy from queueing early at these sizes), the early build
# (cu_flex bit 5), the lane-bound kernel (no stage: the same device functions, lane by lane).  The statistics
# build is every one of these scenes' launch with statistics.
BUILDS = {"plain": dict(cu_flex=1), "general": dict(general=True, cu_flex=1), "early": dict(cu_flex=33),
          "lane": dict(scheduler="lane")}


def _counts(st):
    return (st.paths, st.rays, st.closest_rays, st.shadow_rays, st.nan_samples)


@pytest.mark.parametrize("frame", FRAMES, ids=[_id(f) for f in FRAMES])
def test_every_build_renders_the_oracles_bits(frame):
    import torch
    name, res, spp, depth, cam = frame
    s = _scene(name, res, cam)
    p = s.default_params(samples=spp) if depth is None else s.default_params(samples=spp, depth=depth)
    cpu, cst, _ = O.render(s, p)
    assert np.isfinite(cpu).all() and cst.paths == res[0] * res[1] * spp
    if cam is not None:
        # nothing scatters behind the wall: a path is its camera ray and at most one shadow ray
        assert cst.closest_rays == cst.paths and 0 < cst.shadow_rays <= cst.paths
    elif depth is None:
        assert cpu.max() > 0 and cst.closest_rays > 2 * cst.paths
    images = {}
    for build, opts in BUILDS.items():
        d = _dev(s, **opts)
        if build in ("plain", "general"):
            assert d.kernel_for(p) == (PLAIN_NAME if build == "plain" else GENERAL_NAME)
        if build == "lane":
            assert "render_kernel" in d.kernel_for(p)
        img = d.render(p, stats=False)   # (no statistics: the build itself)
        torch.cuda.synchronize()
        d.check()
        images[build] = img.cpu().numpy()
        if build == "plain":
            simg, sst = d.render(p)      # ... and the statistics build, with the counts
            images["stats"] = simg.cpu().numpy()
            assert _counts(sst) == _counts(cst), (build, _counts(sst), _counts(cst))
        d.close()
    for build, img in images.items():
        _compare_images(img, cpu, f"{_id(frame)} {build}")
        assert np.array_equal(img.view(np.uint32), images["plain"].view(np.uint32)), build
        assert np.array_equal(img.view(np.uint32), cpu.view(np.uint32)), build
