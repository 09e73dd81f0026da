"""The binding's stream rule (vimg_amd.hip._Launch): a call gives the same bits on the default stream,
inside ``with torch.cuda.stream(side)`` and with ``stream=side`` while the default stream is current - for every
call that allocates its result or copies a numpy argument up.  Equality of results only: nothing here tries to
make a race show itself.  36 x 20 is ragged against the 8 x 8 tiles in both directions, the smallest frame on which
a shard slab and a whole frame differ in shape and the edge tiles are exercised."""
from types import SimpleNamespace

import numpy as np
import pytest

import scenes
from test_scene_update_host import deformed

pytestmark = pytest.mark.gpu

RES = (36, 20)


@pytest.fixture(scope="module")
def ctx():
    import torch
    from vimg_amd import hip
    s = scenes.json_scene("disney_spheres.json", res=RES)
    c = SimpleNamespace(hip=hip, s=s, dev=hip.DeviceScene(s), side=torch.cuda.Stream(),
                        p=s.default_params(samples=4, depth=3),
                        p_shard=s.default_params(samples=4, depth=3, tile_world=2, tile_rank=1))
    c.frame = c.dev.render(c.p, stats=False)
    yy, xx = np.mgrid[0:RES[1], 0:RES[0]]
    c.mask = (xx + yy) % 3 != 0
    c.acc = c.dev.progressive(c.p)          # an accumulator with unequal counts for the read-outs
    c.acc.render(2)
    c.acc.render(2, mask=c.mask)
    torch.cuda.synchronize()
    yield c
    c.acc.close()
    c.dev.close()


@pytest.fixture(scope="module")
def moved():
    """A second upload for the updates, its positions as uploaded and moved (numpy and CUDA tables)."""
    import torch
    from vimg_amd import hip
    s = scenes.json_scene("disney_spheres.json", res=RES)
    m = SimpleNamespace(dev=hip.DeviceScene(s), v0=s.geometry()[0], v=deformed(s, seed=5)[0], results={})
    assert m.v.shape[0] > 0 and not np.array_equal(m.v, m.v0)
    m.v_cuda = torch.from_numpy(m.v).to("cuda")
    torch.cuda.synchronize()
    yield m
    m.dev.close()


def _host(r):
    """The result of a call as numpy arrays (a tensor, a float, or a tuple / dict of them)."""
    if isinstance(r, dict):
        return {k: _host(v) for k, v in r.items()}
    if isinstance(r, tuple):
        return tuple(_host(v) for v in r)
    return r.cpu().numpy() if hasattr(r, "cpu") else r


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def _three_ways(side, call, before=lambda: None):
    """call(stream) on the default stream, inside the side stream's context, and with stream=side; `before` runs on
    the default stream ahead of each and is waited for.  Returns the first result after checking the other two."""
    import torch
    assert torch.cuda.current_stream().cuda_stream != side.cuda_stream
    got = []
    for way in ("default stream", "with torch.cuda.stream(side)", "stream=side"):
        before()
        torch.cuda.synchronize()
        if way == "with torch.cuda.stream(side)":
            with torch.cuda.stream(side):
                r = call(None)
        else:
            r = call(side if way == "stream=side" else None)
        side.synchronize()
        torch.cuda.current_stream().synchronize()
        got.append(_host(r))
        assert _same(got[0], got[-1]), way
    return got[0]


def _fresh_increment(c, **kw):
    def call(stream):
        acc = c.dev.progressive(c.p)
        try:
            return _host(acc.render(4, stream=stream, **kw))   # (read before the accumulator goes)
        finally:
            acc.close()
    return call


CALLS = {
    "render": lambda c: lambda st: c.dev.render(c.p, stats=False, stream=st),
    "render shard": lambda c: lambda st: c.dev.render(c.p_shard, stats=False, stream=st),
    "render_heatmap": lambda c: lambda st: c.dev.render_heatmap(c.p, stream=st),
    "post_rgb8": lambda c: lambda st: c.hip.post_rgb8(c.frame, stream=st),
    "Progressive.render": lambda c: _fresh_increment(c),
    "Progressive.render numpy mask": lambda c: _fresh_increment(c, mask=c.mask),
    "Progressive.state": lambda c: lambda st: c.acc.state(stream=st),
    "Progressive.counts": lambda c: lambda st: c.acc.counts(stream=st),
    "Progressive.error": lambda c: lambda st: c.acc.error(stream=st),
    "Progressive.select": lambda c: lambda st: c.acc.select(0.05, 64, stream=st),
    "bvh_cost": lambda c: lambda st: c.dev.bvh_cost(stream=st),
}


@pytest.mark.parametrize("name", list(CALLS))
def test_same_bits_on_every_stream(name, ctx):
    r = _three_ways(ctx.side, CALLS[name](ctx))
    if name == "render":
        assert r.shape == (RES[1], RES[0], 3) and _same(r, _host(ctx.frame))
    if name == "render shard":
        assert r.shape == (ctx.dev.shard_pixels(ctx.p_shard), 3)
    if name == "Progressive.render numpy mask":
        assert (r[~ctx.mask] == 0).all() and r[ctx.mask].any()
    if name == "Progressive.select":
        assert r[1] == int((r[0] != 0).sum()) > 0


def test_counts_are_the_state_launch(ctx):
    state, counts = ctx.acc.state(), ctx.acc.counts()
    assert counts.dtype == state["count"].dtype and _same(_host(counts), _host(state["count"]))
    assert set(np.unique(_host(counts))) == {2, 4}
    assert list(state) == ["sum", "count", "batches", "m2"]


@pytest.mark.parametrize("table", ["numpy", "cuda"])
def test_update_geometry_then_render_on_every_stream(table, ctx, moved):
    v = moved.v if table == "numpy" else moved.v_cuda

    def call(stream):
        moved.dev.update_geometry(vertices=v, stream=stream)
        return moved.dev.render(ctx.p, stats=False, stream=stream)
    r = _three_ways(ctx.side, call, before=lambda: moved.dev.update_geometry(vertices=moved.v0))
    assert not _same(r, _host(ctx.frame))        # the update was seen
    moved.results[table] = r


def test_update_geometry_is_update_materials_with_positions_only(ctx, moved):
    for table in ("numpy", "cuda"):
        if table not in moved.results:
            moved.dev.update_geometry(vertices=moved.v0)
            moved.dev.update_geometry(vertices=moved.v if table == "numpy" else moved.v_cuda)
            moved.results[table] = _host(moved.dev.render(ctx.p, stats=False))
    moved.dev.update_geometry(vertices=moved.v0)
    moved.dev.update_materials(vertices=moved.v)
    r = _host(moved.dev.render(ctx.p, stats=False))
    assert _same(r, moved.results["numpy"]) and _same(r, moved.results["cuda"])
