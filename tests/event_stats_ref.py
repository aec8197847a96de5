"""The loader's side of EventStream stated in numpy alone, from the definitions: per-pixel counts, the
accumulation picture, the hot-pixel mask and the stream without masked pixels.  Not a test: tests/test_event_stats_ref.py
holds `render` equal to the reference's own render_ev_accumulation (tests/golden/ref_event_accumulation.npz) and the CPU
route of EventStream equal to these; tests/test_gpu_event_stats.py holds the device route equal to these."""
import math

import numpy as np


def polarity(p):
    """+1 where p > 0, -1 otherwise (0/1 files and -1/+1 files alike)."""
    return np.where(np.asarray(p) > 0, 1, -1).astype(np.int64)


def pixel_counts(x, y, p, H, W):
    """int32 [H, W, 2]: events of polarity -1 and of polarity +1 per sensor pixel."""
    c = np.zeros((H, W, 2), np.int32)
    np.add.at(c, (np.asarray(y, np.int64), np.asarray(x, np.int64), (polarity(p) > 0).astype(np.int64)), 1)
    return c


def render(x, y, pol, H, W):
    """The accumulation picture of coordinates of any dtype: white, then every event with x >= 0, y >= 0, x < W, y < H
    gives the cell (int(y), int(x)) its polarity (0 counts as -1), a later event over an earlier one; -1 is (255, 0, 0), +1
    (0, 0, 255).  uint8 [H, W, 3]."""
    x, y = np.asarray(x), np.asarray(y)
    pol = polarity(pol)
    ok = (x >= 0) & (y >= 0) & (x < W) & (y < H)                           # (False for NaN)
    last = np.zeros(H * W, np.int64)
    cells = y[ok].astype(np.int64) * W + x[ok].astype(np.int64)            # truncated (the values are not negative)
    for c, v in zip(cells.tolist(), pol[ok].tolist()):                     # stream order: the last event at a cell stays
        last[c] = v
    last = last.reshape(H, W)
    img = np.full((H, W, 3), 255, np.uint8)
    img[last == -1] = (255, 0, 0)
    img[last == 1] = (0, 0, 255)
    return img


def accumulation_image(x, y, p, H, W, rectify_map=None):
    """EventStream.accumulation_image: sensor cells, or with a map the cells of (xr, yr) = rectify_map[y, x] in float32."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    if rectify_map is None:
        return render(x, y, p, H, W)
    r = np.asarray(rectify_map, np.float32)[y, x]
    return render(r[:, 0], r[:, 1], p, H, W)


def moments(counts):
    """(n, S, Q) of c = counts.sum(-1) as Python integers: pixels with c > 0, sum c, sum c * c."""
    c = np.asarray(counts, np.int64).sum(-1).reshape(-1)
    return int((c > 0).sum()), int(c.sum()), int((c * c).sum())


def threshold(n, S, Q, n_sigma=None, max_count=None):
    if max_count is not None:
        return int(max_count)
    mu = S / n
    sigma = math.sqrt(max(Q / n - mu * mu, 0.0))
    return int(math.floor(mu + n_sigma * sigma))


def hot_pixels(x, y, p, H, W, n_sigma=None, max_count=None):
    """-> (bool [H, W], the report EventStream.hot_pixels leaves)."""
    counts = pixel_counts(x, y, p, H, W)
    c = counts.astype(np.int64).sum(-1)
    n, S, Q = moments(counts)
    T = threshold(n, S, Q, n_sigma, max_count)
    mask = c > T
    return mask, {"active": n, "events": S, "threshold": T, "hot": int(mask.sum()), "hot_events": int(c[mask].sum())}


def without_pixels(x, y, t, p, mask):
    """The four columns without the events at masked sensor pixels, order kept."""
    keep = ~np.asarray(mask, bool)[np.asarray(y, np.int64), np.asarray(x, np.int64)]
    return tuple(np.asarray(v)[keep] for v in (x, y, t, p))


def random_stream(seed, E, H, W, hot=0, hot_share=0.0):
    """A seeded stream: uniform pixels, `hot` pixels holding `hot_share` of the events, ascending microsecond stamps,
    -1 / +1 polarities.  -> dict of x, y (uint16), t (int64), p (int8)."""
    g = np.random.default_rng(seed)
    x = g.integers(0, W, E)
    y = g.integers(0, H, E)
    if hot:
        at = g.random(E) < hot_share
        which = g.integers(0, hot, E)
        hx, hy = g.integers(0, W, hot), g.integers(0, H, hot)
        x, y = np.where(at, hx[which], x), np.where(at, hy[which], y)
    t = np.sort(g.integers(1_000_000, 1_000_000 + max(50_000, E // 20), E)).astype(np.int64)
    p = g.choice(np.array([-1, 1], np.int8), E)
    return {"x": x.astype(np.uint16), "y": y.astype(np.uint16), "t": t, "p": p}


def random_map(seed, H, W):
    """A rectify map [H, W, 2] float32 (x', y') with every kind of target: inside (fractional), negative, in [W - 1, W)
    and [H - 1, H), at and beyond W / H, and NaN."""
    g = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    m = np.stack([xx + g.uniform(-1.5, 1.5, (H, W)), yy + g.uniform(-1.5, 1.5, (H, W))], -1).astype(np.float32)
    kind = g.integers(0, 12, (H, W))
    m[kind == 0, 0] = -0.25
    m[kind == 1, 1] = -3.0
    m[kind == 2, 0] = np.float32(W) - np.float32(0.5)
    m[kind == 3, 1] = np.nextafter(np.float32(H), np.float32(0))
    m[kind == 4, 0] = W
    m[kind == 5, 1] = H + 7.5
    m[kind == 6, 0] = np.nan
    m[kind == 7, 1] = np.nan
    m.reshape(-1, 2)[:8] = [[-0.25, 1], [1, -3.0], [W - 0.5, 0], [0, H - 0.25], [W, 0], [0, H + 7.5], [np.nan, 1], [1, np.nan]]
    return m
