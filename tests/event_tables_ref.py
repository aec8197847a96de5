"""A plain statement of what csrc/event_tables.hip computes, in numpy alone (no torch, nothing of enerf_amd), and the event
streams the device tests feed it (tests/test_gpu_event_tables_edges.py; tests/test_event_tables_ref.py pins this file to
the loop oracle and to enerf_amd.event_dataset.tables_statement before a GPU sees a case).

Semantics (enerf_amd/event_dataset.py, DESIGN.md 4.20, oracle/event_collate.py): the pixel key is the SENSOR pixel
y * W + x; pixels with fewer than two events in the window are dropped; pixels are ordered by the stream position of their
first event and a pixel's events by stream position; time is float32(float64(t + t_offset) * ns_per_unit); polarity is +1
where p > 0 and -1 otherwise; a no-event candidate of chunk j is a pixel without an event e with
edges[j] <= (float64(t + t_offset) * ns_per_unit) * 1e-3 < edges[j + 1], the two products rounded one after the other."""
import numpy as np


# ---- the reference ----------------------------------------------------------------------------------------------------
def tables(x, y, t, p, first, last, H, W, rect=None, ns_per_unit=1000.0, t_offset=0):
    """-> dict: events [N, 4] fp32, num_at_xy / first_at_xy int64 [P], no_successor bool [N], num_successor int64 [N],
    pol_cumsum float64 [N + 1], and order int64 [N] (the window position of every row).  rect [H, W, 2] or None (the
    integer coordinates).  Every event of the window must lie on the sensor."""
    xs, ys = np.asarray(x[first:last]).astype(np.int64), np.asarray(y[first:last]).astype(np.int64)
    if xs.size and (xs.max() >= W or ys.max() >= H or xs.min() < 0 or ys.min() < 0):
        raise ValueError("event_tables_ref.tables: an event outside the sensor")
    E = xs.size
    pix = ys * W + xs
    by_pixel = np.argsort(pix, kind="stable")                       # grouped by pixel, stream order inside a pixel
    sp = pix[by_pixel]
    starts = np.flatnonzero(np.concatenate([[True], sp[1:] != sp[:-1]])) if E else np.zeros(0, np.int64)
    counts = np.diff(np.concatenate([starts, [E]]))
    kept = counts > 1
    starts, counts = starts[kept], counts[kept]
    rank = np.argsort(by_pixel[starts], kind="stable")              # a group's first entry is the pixel's first event
    starts, num = starts[rank], counts[rank].astype(np.int64)
    first_at = np.cumsum(num) - num
    N, P = int(num.sum()), int(num.size)
    order = by_pixel[np.repeat(starts - first_at, num) + np.arange(N)]
    tt = np.asarray(t[first:last]).astype(np.int64)[order]
    t_ns = ((tt + int(t_offset)).astype(np.float64) * float(ns_per_unit)).astype(np.float32)
    pol = np.where(np.asarray(p[first:last])[order] > 0, 1, -1).astype(np.int64)
    if rect is None:
        cx, cy = xs[order].astype(np.float32), ys[order].astype(np.float32)
    else:
        r32 = np.asarray(rect).astype(np.float32)
        cx, cy = r32[ys[order], xs[order], 0], r32[ys[order], xs[order], 1]
    events = np.stack([cx, cy, t_ns, pol.astype(np.float32)], axis=1).astype(np.float32).reshape(N, 4)
    num_successor = np.repeat(first_at + num, num) - np.arange(N) - 1
    pol_cumsum = np.concatenate([[0], np.cumsum(pol)]).astype(np.float64)
    return {"events": events, "num_at_xy": num, "first_at_xy": first_at, "no_successor": num_successor == 0,
            "num_successor": num_successor, "pol_cumsum": pol_cumsum, "order": order, "N": N, "P": P}


def no_event_candidates(x, y, t, first, last, H, W, edges_us, ns_per_unit=1000.0, t_offset=0):
    """-> list over the chunks: the ascending linear indices (int64) of the pixels without an event in the chunk."""
    pix = np.asarray(y[first:last]).astype(np.int64) * W + np.asarray(x[first:last]).astype(np.int64)
    t_ns = (np.asarray(t[first:last]).astype(np.int64) + int(t_offset)).astype(np.float64) * float(ns_per_unit)
    t_us = t_ns * 1e-3
    out = []
    for j in range(len(edges_us) - 1):
        m = (t_us >= edges_us[j]) & (t_us < edges_us[j + 1])
        hit = np.zeros(H * W, bool)
        hit[pix[m]] = True
        out.append(np.flatnonzero(~hit).astype(np.int64))
    return out


def edges(start_us, end_us, chunk_len_ms):
    """The chunk edges as provider.py:1299-1313 and :1348 accumulate them (float64, `ts_iter += dt_us`)."""
    dur_ms = end_us / 1e3 - start_us / 1e3
    n = int(dur_ms / chunk_len_ms) + 1
    dt_us = 1e3 * dur_ms / n
    e = [float(start_us)]
    for _ in range(n):
        e.append(e[-1] + dt_us)
    return e


# ---- the cases --------------------------------------------------------------------------------------------------------
KEYS = ("events", "num_at_xy", "first_at_xy", "no_successor", "num_successor", "pol_cumsum")
SCAN_TILE = 2048                                                    # values per workgroup of a scan (kScanTile)
SCAN_TOP = 256 * SCAN_TILE                                          # values one round of k_scan_top covers


def frac_map(H, W):
    """x' = 0.7 x + 0.25, y' = 0.7 y + 0.125: fractional, compressing, injective."""
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    return np.stack([0.7 * xs + 0.25, 0.7 * ys + 0.125], axis=2)


def _case(pix, t, p, H, W, rect=True, first=0, last=None, unit_per_ms=1000, t_offset=0, **more):
    pix = np.asarray(pix)
    c = {"x": (pix % W).astype(np.uint16), "y": (pix // W).astype(np.uint16), "t": np.asarray(t).astype(np.int64),
         "p": np.asarray(p).astype(np.int8), "H": H, "W": W, "rect": frac_map(H, W) if rect else None, "first": first,
         "last": len(pix) if last is None else last, "unit_per_ms": unit_per_ms, "t_offset": t_offset}
    c.update(more)
    return c


def reference(c):
    return tables(c["x"], c["y"], c["t"], c["p"], c["first"], c["last"], c["H"], c["W"], c["rect"],
                  1e6 / float(c["unit_per_ms"]), c["t_offset"])


def _stamps(rng, n, t0=1000, lo=0):
    return t0 + np.cumsum(rng.integers(lo, 3, n))


def case_scan_carry():
    """30 x 41 sensor, 2048 * 257 + 3 events, 85 % of them negative: the rank and finish scans span 258 tiles, so
    k_scan_top goes round twice, and the running polarity is below -350 000 where its carry enters."""
    rng = np.random.default_rng(11)
    n = SCAN_TILE * 257 + 3
    pix = rng.integers(0, 30 * 41, n)
    return _case(pix, _stamps(rng, n), rng.random(n) >= 0.85, 30, 41)


def case_big_sensor():
    """1024 x 513 sensor (525 312 pixels: a multiple of 32, more than 524 288), every pixel twice in shuffled order and
    3000 events more, 50 events before the span and 50 after it: P = H * W = pmax - 1 through the H * W branch, more than
    256 tiles in the first scan.  32 chunks: 3, 17 and 31 sparse (200 events), 5 empty; 32 * 16 416 bitmap words."""
    rng = np.random.default_rng(12)
    H, W = 513, 1024
    HW = H * W
    pix = np.concatenate([np.arange(HW), np.arange(HW), rng.integers(0, HW, 3000)])
    pix = pix[rng.permutation(pix.size)]
    n = pix.size
    start_us, end_us, chunk_len_ms = 1_000_000.0, 1_064_007.0, 2.05
    e = edges(start_us, end_us, chunk_len_ms)
    assert len(e) == 33 and e[1] != np.floor(e[1])
    n_out, sparse, empty = 50, (3, 17, 31), 5
    dense = [j for j in range(32) if j not in sparse and j != empty]
    per = np.zeros(32, np.int64)
    per[list(sparse)] = 200
    rest = n - 2 * n_out - 200 * len(sparse)
    per[dense] = rest // len(dense)
    per[dense[0]] += rest - per[dense].sum()
    t = [rng.integers(int(start_us) - 5000, int(start_us), n_out)]
    for j in range(32):
        t.append(rng.integers(int(np.ceil(e[j])), int(np.floor(e[j + 1])), per[j]))
    t.append(rng.integers(int(np.ceil(e[32])) + 1, int(e[32]) + 5000, n_out))
    t = np.sort(np.concatenate(t))
    assert t.size == n
    return _case(pix, t, rng.integers(0, 2, n), H, W, span=(start_us, end_us, chunk_len_ms), sparse=sparse, empty=empty)


def case_exact_fit(odd):
    """2 k events on k = 700 distinct pixels of the 30 x 41 sensor: P = k = E / 2 = pmax - 1; `odd`: one more pixel with a
    single event, E = 2 k + 1."""
    rng = np.random.default_rng(13 + odd)
    k = 700
    chosen = rng.permutation(30 * 41)[:k + 1]
    pix = np.concatenate([chosen[:k], chosen[:k], chosen[k:][:odd]])
    pix = pix[rng.permutation(pix.size)]
    return _case(pix, _stamps(rng, pix.size), rng.integers(0, 2, pix.size), 30, 41)


def case_two_events(offset):
    """Two events on one pixel: N = 2, P = 1.  `offset`: the same two at first = 1 of a stream of five (x and y are
    uint16: the window begins at an odd 2-byte address)."""
    pix = [77, 77] if not offset else [3, 77, 77, 5, 9]
    n = len(pix)
    return _case(pix, 1000 + 7 * np.arange(n), [1, 0, 1, 1, 0][:n], 30, 41, first=offset, last=offset + 2)


def case_no_pair():
    return _case([4, 9, 1229], [1000, 1001, 1002], [1, 0, 1], 30, 41)


SEGMENT_LENGTHS = (1, 2, 32, 33, 4096, 4097)


def case_segment_boundaries():
    """6 x 6 sensor: six pixels with exactly 1, 2, 32, 33, 4096 and 4097 events (the single one is dropped), the other 30
    with 40 .. 600; stream order shuffled."""
    rng = np.random.default_rng(15)
    where = rng.permutation(36)
    counts = np.concatenate([SEGMENT_LENGTHS, rng.integers(40, 601, 30)])
    pix = np.repeat(where, counts)
    pix = pix[rng.permutation(pix.size)]
    return _case(pix, _stamps(rng, pix.size), rng.integers(0, 2, pix.size), 6, 6, pixels=where[:6])


def case_many_long_segments():
    """30 x 41 sensor, 36 to 40 events on every pixel: 1230 segments that a workgroup sorts, more than the 1024 of the grid."""
    rng = np.random.default_rng(16)
    pix = np.repeat(np.arange(30 * 41), rng.integers(36, 41, 30 * 41))
    pix = pix[rng.permutation(pix.size)]
    return _case(pix, _stamps(rng, pix.size), rng.integers(0, 2, pix.size), 30, 41)


TIME_UNITS = ((1_000_000, 0), (1000, 123_456_789), (1_000_000, 123_456_789))


def case_time_units(unit_per_ms, t_offset):
    """5000 events on the 30 x 41 sensor, the window strictly inside the stream, stamps near 5e7 us spaced 1 or 2 us (in
    nanoseconds with 1e6 units per ms): (float) t_ns is 4096 ns apart or more there, so distinct stamps are one fp32 value
    and the order among them is stream order.  Pixel 0 fires once in the window, pixel 1 twice."""
    rng = np.random.default_rng(17)
    n = 5000
    pix = rng.integers(2, 30 * 41, n)
    pix[[50, 1000]] = 0
    pix[[2000, n - 500]] = 1
    t = 50_000_000 + np.cumsum(rng.integers(1, 3, n))
    if unit_per_ms == 1_000_000:
        t = t * 1000 + np.sort(rng.integers(0, 1000, n))
    return _case(pix, t, rng.integers(0, 2, n), 30, 41, first=137, last=4871, unit_per_ms=unit_per_ms, t_offset=t_offset)


def time_units_span(c):
    """A span for case_time_units' window in three chunks with fractional edges: it begins after the window's first events
    and ends before its last."""
    k = c["unit_per_ms"] / 1000
    t_us = (c["t"][c["first"]:c["last"]] + c["t_offset"]) / k
    return float(np.floor(t_us[40])) + 0.5, float(np.floor(t_us[-40])) + 0.25, (t_us[-40] - t_us[40]) / 1e3 / 2.5


SENSORS = ((32, 32), (3, 11), (1, 31), (4, 4))                      # H, W: 1024 pixels, 33 (one in the last word), 31, 16
SPANS = ((1, 1_000_000.0, 1_050_001.0, 100.0), (3, 1_000_000.0, 1_050_001.0, 20.0))      # n_chunks, start, end, chunk_len_ms


def case_edge_events(H, W, span):
    """Events at the integer stamps either side of every edge of the span (on an edge where it is an integer), one before
    the first edge and one after the last, and a few inside the chunks."""
    rng = np.random.default_rng(18 + H * W)
    n_chunks, start_us, end_us, chunk_len_ms = span
    e = edges(start_us, end_us, chunk_len_ms)
    assert len(e) == n_chunks + 1
    t = [int(e[0]) - 3]
    for v in e:
        t += [int(np.floor(v)) - 1, int(np.floor(v)), int(np.ceil(v)), int(np.ceil(v)) + 1]
    t += [int(np.ceil(e[-1])) + 9]
    t += list(rng.integers(int(e[0]) + 5, int(e[-1]) - 5, max(2, H * W // 4)))
    t = np.sort(np.array(t))
    pix = rng.permutation(np.arange(t.size) % (H * W))              # distinct pixels while they last: each event shows
    return _case(pix, t, rng.integers(0, 2, t.size), H, W, span=(start_us, end_us, chunk_len_ms))


def case_full_and_empty_chunks(H, W, span, fill):
    """n_chunks = 3: every pixel fires in chunk 0, none in chunk 1, a few in chunk 2.  n_chunks = 1: every pixel fires in
    the chunk (`fill`), or none does and the events lie before and after the span (the row holds all H * W pixels)."""
    rng = np.random.default_rng(19 + H * W)
    n_chunks, start_us, end_us, chunk_len_ms = span
    e = edges(start_us, end_us, chunk_len_ms)
    HW = H * W
    inside = lambda j, n: rng.integers(int(e[j]) + 10, int(e[j + 1]) - 10, n)            # noqa: E731
    every = np.concatenate([np.arange(HW), rng.integers(0, HW, 5)])
    if n_chunks == 3:
        pix = np.concatenate([every, rng.integers(0, HW, 4)])
        t = np.concatenate([inside(0, every.size), inside(2, 4)])
    elif fill:
        pix, t = every, inside(0, every.size)
    else:
        pix = rng.integers(0, HW, 12)
        t = np.concatenate([rng.integers(int(e[0]) - 500, int(e[0]), 6), rng.integers(int(e[1]) + 1, int(e[1]) + 500, 6)])
    order = np.argsort(t, kind="stable")
    return _case(pix[order], t[order], rng.integers(0, 2, t.size), H, W, span=(start_us, end_us, chunk_len_ms))


def candidates(c):
    """no_event_candidates over the case's window and span -> (list of rows, edges)."""
    e = edges(*c["span"])
    return no_event_candidates(c["x"], c["y"], c["t"], c["first"], c["last"], c["H"], c["W"], e,
                               1e6 / float(c["unit_per_ms"]), c["t_offset"]), e


# ---- segments for the sort aid ----------------------------------------------------------------------------------------
SORT_LENGTHS = (2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1025, 4095, 4096, 4097, 8192, 8193, 12289)
FILLINGS = ("ascending", "descending", "shuffled", "smallest last")
CANARY = 0xffffffff                                                 # never an entry: entries are below it


def _filled(values, filling, rng):
    v = np.sort(values)
    if filling == "descending":
        v = v[::-1]
    elif filling == "shuffled":
        v = v[rng.permutation(v.size)]
    elif filling == "smallest last":
        v = np.concatenate([v[1:], v[:1]])
    return v


def segments(lengths, fillings, seed, gap=3, tail=5):
    """One idx array for the sort aid: segment k has lengths[k] unique uint32 entries drawn from the whole range (0 and
    0xfffffffe among them) in the filling fillings[k], `gap` canary entries lie in front of every segment and `tail`
    behind the last.  -> (idx uint32 [N + tail], N, num uint32 [P], first uint32 [P], want: idx with every segment sorted)."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int64)
    total = int(lengths.sum())
    pool = np.unique(np.concatenate([rng.integers(1, 0xfffffffe, total + 1000, dtype=np.uint64), [0, 0xfffffffe]]))
    assert pool.size >= total
    rest = rng.permutation(pool[1:-1])[:total - 2]
    pool = rng.permutation(np.concatenate([[0, 0xfffffffe], rest])).astype(np.uint32)
    first = np.cumsum(lengths + gap) - lengths
    N = int(first[-1] + lengths[-1])
    idx = np.full(N + tail, CANARY, np.uint32)
    want = idx.copy()
    at = 0
    for k, (n, b) in enumerate(zip(lengths, first)):
        vals = pool[at:at + n]
        at += n
        idx[b:b + n] = _filled(vals, fillings[k], rng)
        want[b:b + n] = np.sort(vals)
    return idx, N, lengths.astype(np.uint32), first.astype(np.uint32), want
