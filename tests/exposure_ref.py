"""numpy restatement of the contract of include/vimg_exposure.h (libvimg_exposure.so), written from the header and not
from the kernels: uint32 / uint64 integer arithmetic and float32 + - * /, one rounding each, in the order written.  The
state is the 1040 bytes the library keeps in device memory, as a numpy uint8 array; ``adapt`` returns the new state's
bytes and the scaled frame, which the GPU tests compare BIT FOR BIT."""
import numpy as np

F = np.float32
BINS, FIRST, STATE_BYTES = 256, 888, 1040
DEFAULTS = dict(low_permille=500, high_permille=950, key=0.18, min_exposure=1 / 64, max_exposure=64.0, rate_brighten=0.25,
                rate_darken=0.5)
STATE = np.dtype([("hist", np.uint32, BINS), ("exposure", F), ("frames", np.uint32), ("metered", F), ("counted", np.uint32)])
assert STATE.itemsize == STATE_BYTES


def new_state():
    return np.zeros(STATE_BYTES, np.uint8)


def fields(state):
    """The state's bytes as one record: hist, exposure, frames, metered, counted."""
    return np.ascontiguousarray(state).view(STATE)[0]


def read(state):
    s = fields(state)
    return {"exposure": float(s["exposure"]) if s["frames"] else 1.0, "frames": int(s["frames"]), "metered": float(s["metered"]),
            "counted": int(s["counted"])}


def luminance(c):
    c = np.asarray(c, F)
    return (c[..., 0] * F(0.212671) + c[..., 1] * F(0.715160)) + c[..., 2] * F(0.072169)


def bin_of(L):
    """The bin of each luminance, and whether it is counted at all (without a depth frame)."""
    L = np.asarray(L, F)
    with np.errstate(invalid="ignore"):
        counted = (L > 0) & (L < np.inf)
    k = (np.ascontiguousarray(L).view(np.uint32) >> np.uint32(20)).astype(np.int64) - FIRST
    return np.clip(k, 0, BINS - 1), counted


def edge(b):
    """Where bin b starts; edge(256) = 2^16 is where bin 255 ends."""
    return np.array((int(b) + FIRST) << 20, np.uint32).view(F)[()]


def meter(color, depth=None):
    """hist[256] (uint32) of the frame."""
    k, counted = bin_of(luminance(color))
    if depth is not None:
        with np.errstate(invalid="ignore"):
            counted = counted & (np.asarray(depth, F)[..., 0] > 0)
    return np.bincount(k[counted].ravel(), minlength=BINS).astype(np.uint32)


def window(hist, low_permille, high_permille):
    """(T, lo, hi, S) as Python integers (exact; every value fits a uint64)."""
    counts = [int(c) for c in hist]
    T = sum(counts)
    lo, hi = T * int(low_permille) // 1000, T * int(high_permille) // 1000
    S, first = 0, 0
    for b, c in enumerate(counts):
        end = first + c
        S += b * max(0, min(end, hi) - max(first, lo))
        first = end
    assert S < 2 ** 64
    return T, lo, hi, S


def metered_of(S, ranks):
    m = F(np.uint64(S)) / F(np.uint64(ranks))
    i = int(np.floor(m))
    f = m - F(i)
    e0, e1 = edge(i), edge(i + 1)
    return F(e0 + f * (e1 - e0))


def target_of(metered, key, min_exposure, max_exposure):
    E = F(key) / F(metered)
    if E < F(min_exposure):
        E = F(min_exposure)
    if E > F(max_exposure):
        E = F(max_exposure)
    return F(E)


def resolve(state, hist, **params):
    """The new state's bytes after a call that metered ``hist`` (added to what the state's own histogram holds)."""
    p = dict(DEFAULTS, **params)
    new = np.array(state, np.uint8, copy=True)
    s = new.view(STATE)[0]
    T, lo, hi, S = window(s["hist"].astype(np.uint64) + np.asarray(hist, np.uint64), p["low_permille"], p["high_permille"])
    s["hist"] = 0
    s["counted"] = np.uint32(T)
    if T == 0 or hi == lo:
        return new
    metered = metered_of(S, hi - lo)
    target = target_of(metered, p["key"], p["min_exposure"], p["max_exposure"])
    if s["frames"] == 0:
        E = target
    else:
        was = F(s["exposure"])
        rate = F(p["rate_darken"]) if target < was else F(p["rate_brighten"])
        E = F(was + F(F(target - was) * rate))
    s["exposure"], s["metered"], s["frames"] = E, metered, s["frames"] + np.uint32(1)
    return new


def adapt(color, depth=None, state=None, apply=True, **params):
    """(the scaled frame or None, the new state's bytes)."""
    color = np.asarray(color, F)
    new = resolve(new_state() if state is None else state, meter(color, depth), **params)
    if not apply:
        return None, new
    s = new.view(STATE)[0]
    E = F(s["exposure"]) if s["frames"] else F(1)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return (color * E).astype(F), new


def target(color, depth=None, **params):
    """E* of a frame on its own, or None when nothing is metered."""
    p = dict(DEFAULTS, **params)
    T, lo, hi, S = window(meter(color, depth), p["low_permille"], p["high_permille"])
    if T == 0 or hi == lo:
        return None
    return target_of(metered_of(S, hi - lo), p["key"], p["min_exposure"], p["max_exposure"])


def planted(h, w, seed=0, depth=False):
    """A log-uniform random [h, w, 3] frame over 2^-18 .. 2^18 (so both end bins take overflow) with the odd values
    planted where the frame has room for them: NaN, +inf, -inf, 0, a negative, a denormal, and pixels whose luminance sits
    on and just below bin edges.  With ``depth``: a [h, w, 3] depth frame too, with misses (0), a negative and a NaN."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    color = (F(2) ** rng.uniform(-18, 18, (h, w, 1)).astype(F) * rng.uniform(0.5, 1.5, (h, w, 3)).astype(F)).astype(F)
    flat = color.reshape(-1, 3)
    odd = [(np.nan, 1, 1), (np.inf, 0, 0), (1, -np.inf, 1), (0, 0, 0), (-1, -2, -3), (1e-42, 1e-42, 1e-42), (3e38, 3e38, 3e38),
           (-1, 0.5, 0)]
    for b in (0, 1, 100, 255, 256):
        for nudge in (0, -1):
            g = np.array(((b + FIRST) << 20) + nudge, np.uint32).view(F)[()] / F(0.715160)
            odd.append((0, g, 0))
    n = flat.shape[0]
    if n > len(odd):
        where = rng.choice(n, len(odd), replace=False)
        flat[where] = np.array(odd, F)
    elif n > 1:
        flat[-1] = (np.nan, 1, 1)
    z = None
    if depth:
        z = np.repeat(rng.uniform(1, 100, (h, w, 1)).astype(F), 3, axis=2)
        z[rng.uniform(size=(h, w)) < 0.3] = 0
        zf = z.reshape(-1, 3)
        if n > 4:
            zf[1], zf[2] = -5, np.nan
    return color, z
