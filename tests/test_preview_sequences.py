"""TemporalPreview's modes in combination, on one sequence that stands, moves the camera, moves geometry, edits a
texture, rebuilds the tree and resets: every frame of every configuration is bit for bit what
tests/golden/preview_sequences.json holds (tests/golden/make_preview_sequences.py wrote it, through ``walk`` below, before
the preview was split into parts - vimg_amd.preview).  Only the preview's public surface is used."""
import hashlib
import json
import os

import numpy as np
import pytest

from test_motion import moved_vertices, panel_scene
from test_temporal import orbit_camera

RES = 48          # 48 columns leave a partial wave, 48 rows are three row tiles of the anti-lag kernel
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preview_sequences.json")
RECOLOUR = (0.95, 0.85, 0.05)          # the panel's (0.2, 0.3, 0.7), made a bright yellow
ITEMS = ("picture", "history", "sum", "count", "batches", "m2", "last_scale", "last_motion_code", "phase")
MOVED_TRIANGLE = 1


def configurations():
    """{name: temporal_preview's keywords}; ``motion=True`` stands for the host scene."""
    base = {f"{'denoise' if d else 'raw'}-{name}": dict(denoise=d, **kw) for d in (False, True)
            for name, kw in (("plain", {}), ("sparse2", dict(sparse=2)), ("sparse3", dict(sparse=3)))}
    base["variance_guided"] = dict(variance_guided=True)
    return {name + "+antilag" * lag + "+motion" * mo: dict(kw, antilag=lag, motion=mo or None)
            for name, kw in base.items() for lag in (False, True) for mo in (False, True)}


CONFIGS = configurations()
STREAMED = ("denoise-plain+antilag+motion", "denoise-sparse2")          # run once more on a stream of the caller's


def _digest(t):
    return None if t is None else hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def recolour(dev, s):
    """update_materials with the panel's constant texture - the last one - set to RECOLOUR."""
    tex = s.textures()
    tex[len(tex) - 1].col_a[:] = RECOLOUR
    dev.update_materials(textures=tex)


def walk(s, config, streamed=False):
    """The sequence on a fresh DeviceScene of ``s`` = panel_scene(RES): per frame the ITEMS (digests, and the phase as
    it is), and the three counts that say the sequence exercised what it is for."""
    import torch
    from vimg_amd import hip
    dev = hip.DeviceScene(s)
    kw = dict(CONFIGS[config])
    if kw["motion"]:
        kw["motion"] = s
    pre = dev.temporal_preview(s.default_params(integrator="mis", samples=4), samples=4, feature_samples=4, **kw)
    stream = torch.cuda.Stream() if streamed else None
    mine = torch.empty((RES, RES, 3), dtype=torch.float32, device="cuda")
    steps = [lambda: None,
             lambda: None,
             lambda: dev.set_camera(*orbit_camera(1)),
             lambda: None,
             lambda: dev.update_geometry(moved_vertices(s, 1)),
             lambda: (dev.update_geometry(moved_vertices(s, 2)), dev.set_camera(*orbit_camera(2))),
             lambda: None,
             lambda: recolour(dev, s),
             lambda: dev.rebuild_bvh(),
             lambda: pre.reset(),
             lambda: None]
    frames, counts = [], dict(history_length=0.0, moved=0, cut=0)
    for i, edit in enumerate(steps):
        edit()
        out = mine if i == len(steps) - 1 else None
        picture = pre.frame(out=out, stream=stream)
        if streamed:
            stream.synchronize()
        assert out is None or picture is out
        state = pre.acc.state(stream)
        if streamed:
            stream.synchronize()
        frames.append([_digest(picture), _digest(pre.history.tensor)] + [_digest(state[k]) for k in ("sum", "count", "batches", "m2")]
                      + [_digest(pre.last_scale), _digest(pre.last_motion_code), pre.phase])
        counts["history_length"] = max(counts["history_length"], float(pre.history.length.max()))
        if i in (4, 5) and pre.last_motion_code is not None:          # the frames after update_geometry
            counts["moved"] += int((pre.last_motion_code == MOVED_TRIANGLE).sum())
        if i == 7 and pre.last_scale is not None:                     # the frame after the recolour
            counts["cut"] = int((pre.last_scale < 1).sum())
    pre.close()
    dev.close()
    return dict(counts=counts, frames=frames)


@pytest.fixture(scope="module")
def setting():
    from vimg_amd import hip
    hip.init(0)
    with open(RECORD) as f:
        return panel_scene(res=RES), json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(CONFIGS) + [c + "@stream" for c in STREAMED])
def test_every_frame_of_the_sequence_is_the_recorded_one(setting, config):
    """The eleven frames of one configuration against the record, item by item; ``@stream``: the same record, with
    frame(stream=...) on a stream of the caller's.  The record's counts say that it is not hollow: history was carried,
    every ``motion`` configuration saw moved pixels, every ``antilag`` configuration cut after the recolour."""
    s, record = setting
    name, _, streamed = config.partition("@")
    want = record["configurations"][name]
    assert record["items"] == list(ITEMS) and record["res"] == RES and len(want["frames"]) == 11
    assert want["counts"]["history_length"] >= 2
    assert want["counts"]["moved"] > 0 or not CONFIGS[name]["motion"]
    assert want["counts"]["cut"] > 0 or not CONFIGS[name]["antilag"]
    got = walk(s, name, streamed=bool(streamed))
    for i, (g, w) in enumerate(zip(got["frames"], want["frames"])):
        for item, a, b in zip(ITEMS, g, w):
            assert a == b, f"{config}: frame {i + 1}: {item} is {a}, recorded {b}"
    assert got["counts"] == want["counts"], config


def test_the_record_names_every_configuration():
    with open(RECORD) as f:
        record = json.load(f)
    assert sorted(record["configurations"]) == sorted(CONFIGS) and len(CONFIGS) == 28
    assert set(record["streamed"]) == set(STREAMED) <= set(CONFIGS)
    assert os.path.getsize(RECORD) < 64 * 1024
    assert np.all([len(f) == len(ITEMS) for c in record["configurations"].values() for f in c["frames"]])
