"""csrc/event_tables.hip at its scan, sort and bitmap boundaries, bit for bit against tests/event_tables_ref.py (numpy; pinned
to the loop oracle and to the torch statement by tests/test_event_tables_ref.py).  Nothing here is rounded: every
comparison is array_equal.

  A  the segment sorts alone (enerf_debug_event_segment_sort): every length at which the route or the comparator network
     changes, handed ascending, descending, shuffled and nearly sorted segments; more long segments than workgroups; one
     segment on a grid of one
  B  tables through EventStream: two rounds of the scans' top level (rank, first, free, finish; a running polarity below
     -350 000 across the carry), P = pmax - 1 through H * W and through E / 2, the smallest window, the segment lengths
     1, 2, 32, 33, 4096, 4097 in one stream, 1230 long segments, nanosecond stamps and a stream offset
  C  bitmaps and chunk edges: sensors of 1024, 33, 31 and 16 pixels, one chunk and three with fractional edges, events
     either side of every edge, a chunk in which every pixel fires and one in which none does; enerf_no_event_coords
  D  the entry points called directly on buffers with canaries either side
  E  the same bits on two runs"""
import ctypes

import numpy as np
import pytest
import torch

import event_tables_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                                                                 # canary entries either side of a buffer
CANARY = {torch.float32: -12345.5, torch.float64: -12345.5, torch.int64: 0x5a5a5a5a5a5a5a5a, torch.int32: 0x5a5a5a5a,
          torch.uint8: 0xa5}
UNWRITTEN = {torch.float32: float("nan"), torch.float64: float("nan"), torch.int64: -7, torch.int32: -7, torch.uint8: 0x77}


def _lib():
    from enerf_amd import _lib as L
    return L, L.lib()


def _guarded(shape, dtype):
    """-> (buffer with GUARD canary entries either side, its interior viewed as `shape` and filled with UNWRITTEN)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), CANARY[dtype], dtype=dtype, device=DEV)
    inner = buf[GUARD:GUARD + n]
    inner.fill_(UNWRITTEN[dtype])
    return buf, inner.view(shape)


def _intact(buf):
    c = CANARY[buf.dtype]
    return bool((buf[:GUARD] == c).all()) and bool((buf[-GUARD:] == c).all())


def _stream(c):
    from enerf_amd.event_dataset import EventStream
    return EventStream(*(torch.from_numpy(c[k]).to(DEV) for k in "xytp"), c["H"], c["W"], rectify_map=c["rect"],
                       unit_per_ms=c["unit_per_ms"], t_offset=c["t_offset"])


def _equal(tab, ref):
    """The device tables against the reference; beside a mismatch, where they part."""
    ok = True
    for k in R.KEYS:
        a, b = tab[k].cpu().numpy(), ref[k]
        if a.dtype != b.dtype or a.shape != b.shape:
            print(f"{k}: device {a.dtype} {a.shape}, reference {b.dtype} {b.shape}")
            ok = False
        elif not np.array_equal(a, b):
            bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(1))
            print(f"{k}: {bad.size} rows differ, first at {bad[0]}: device {a[bad[0]]}, reference {b[bad[0]]}")
            ok = False
    return ok


def _tables(c):
    s = _stream(c)
    tab = s.tables(c["first"], c["last"])
    ref = R.reference(c)
    assert _equal(tab, ref)
    assert s.last_report == {"N": ref["N"], "P": ref["P"], "bad": 0}
    return tab, ref


def _batch(c, tables=True):
    """(tables, candidate rows as numpy, the no-event dict) of the case's window and span, every candidate row read back."""
    s = _stream(c)
    seen = []
    keep = lambda j, cand: (seen.append(cand.cpu().numpy()), cand[:1])[1]   # noqa: E731
    if tables:
        tab, nev = s.batch_tables(c["first"], c["last"], *c["span"], keep=keep)
    else:
        tab, nev = None, s.no_event_tables(c["first"], c["last"], *c["span"], keep=keep)
    return tab, seen, nev, s.last_report


def _rows_equal(seen, rows):
    assert len(seen) == len(rows)
    for j, (a, b) in enumerate(zip(seen, rows)):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f"chunk {j}: {a.shape} against {b.shape}"


# ---- A: the segment sorts ---------------------------------------------------------------------------------------------
def _sort(idx, N, num, first):
    """enerf_debug_event_segment_sort on idx (uint32 [>= N]; what lies past N is canary) -> idx afterwards."""
    L, lib = _lib()
    P = len(num)
    as_dev = lambda a: torch.from_numpy(a.view(np.int32).copy()).to(DEV)     # noqa: E731
    d_idx, d_num, d_first = as_dev(idx), as_dev(num), as_dev(first)
    words = (20 * P + 32 + 7) // 8
    ws_buf, ws = _guarded((words,), torch.int64)
    L.check(lib.enerf_debug_event_segment_sort(d_idx.data_ptr(), N, d_num.data_ptr(), d_first.data_ptr(), P, ws.data_ptr(),
                                               L.stream_handle()), "debug_event_segment_sort")
    torch.cuda.synchronize()
    assert _intact(ws_buf)
    assert np.array_equal(ws[:P].cpu().numpy(), num.astype(np.int64))       # the num_at_xy / first_at_xy of _fill
    assert np.array_equal(ws[P:2 * P].cpu().numpy(), first.astype(np.int64))
    assert np.array_equal(d_num.cpu().numpy().view(np.uint32), num) and np.array_equal(d_first.cpu().numpy().view(np.uint32), first)
    return d_idx.cpu().numpy().view(np.uint32)


def _sorted_as_wanted(got, want, num, first, lengths, fillings):
    for k, (n, b) in enumerate(zip(num, first)):
        assert np.array_equal(got[b:b + n], want[b:b + n]), f"segment {k}: {lengths[k]} entries, {fillings[k]}"
    assert np.array_equal(got, want)                                       # canaries between the segments and past N


def test_sort_every_length_in_four_fillings():
    lengths = [n for n in R.SORT_LENGTHS for _ in R.FILLINGS]
    fillings = [f for _ in R.SORT_LENGTHS for f in R.FILLINGS]
    idx, N, num, first, want = R.segments(lengths, fillings, seed=1)
    assert len(num) == 88 and (idx[N:] == R.CANARY).all()
    _sorted_as_wanted(_sort(idx, N, num, first), want, num, first, lengths, fillings)


def test_sort_more_long_segments_than_workgroups():
    """1500 segments, all above 32 entries: 1497 of 33 .. 40 and three of 4097 (sorted in global memory) at ranks 0, 750
    and 1499.  The list of long segments is in the order the atomics arrived in, so where the three stand in it cannot be
    forced; the ranks put them at its head, middle and tail.  Takes k_sort_big's q += gridDim.x loop, the LDS tile's reuse
    and a workgroup that sorts in LDS after it sorted in global memory."""
    rng = np.random.default_rng(2)
    lengths = rng.integers(33, 41, 1500)
    lengths[[0, 750, 1499]] = 4097
    fillings = ["shuffled"] * 1500
    idx, N, num, first, want = R.segments(lengths, fillings, seed=3)
    _sorted_as_wanted(_sort(idx, N, num, first), want, num, first, lengths, fillings)


@pytest.mark.parametrize("filling", R.FILLINGS)
def test_sort_one_segment_on_a_grid_of_one(filling):
    idx, N, num, first, want = R.segments([33], [filling], seed=4)
    _sorted_as_wanted(_sort(idx, N, num, first), want, num, first, [33], [filling])


# ---- B: tables end to end ---------------------------------------------------------------------------------------------
def test_scan_carry_in_the_rank_and_finish_scans():
    c = R.case_scan_carry()
    tab, ref = _tables(c)
    assert ref["N"] == R.SCAN_TILE * 257 + 3 and ref["pol_cumsum"][R.SCAN_TOP] < -350_000


_big = {}


def _big_sensor_run():
    if "case" not in _big:
        c = R.case_big_sensor()
        _big.update(case=c, ref=R.reference(c), rows=R.candidates(c)[0])
    tab, seen, nev, report = _batch(_big["case"])
    out = {k: tab[k].cpu().numpy() for k in R.KEYS}
    del tab, nev
    torch.cuda.empty_cache()                                               # the candidate buffer is 134 MB
    return out, seen, report


def test_scan_carry_in_the_first_and_free_scans_on_a_big_sensor():
    out, seen, report = _big_sensor_run()
    _big["first run"] = (out, seen)
    c, ref = _big["case"], _big["ref"]
    HW = c["H"] * c["W"]
    assert report == {"N": len(c["t"]), "P": HW, "bad": 0}                 # P = H * W = pmax - 1
    assert _equal({k: torch.from_numpy(v) for k, v in out.items()}, ref)
    _rows_equal(seen, _big["rows"])
    assert len(seen) == 32 and len(seen[c["empty"]]) == HW


def test_big_sensor_same_bits_on_two_runs():
    if "first run" not in _big:
        _big["first run"] = _big_sensor_run()[:2]
    out, seen = _big_sensor_run()[:2]
    first_out, first_seen = _big.pop("first run")
    for k in R.KEYS:
        assert np.array_equal(out[k], first_out[k]), k
    _rows_equal(seen, first_seen)


@pytest.mark.parametrize("odd", [0, 1])
def test_exact_fit_through_half_the_events(odd):
    c = R.case_exact_fit(odd)
    tab, ref = _tables(c)
    assert ref["P"] == len(c["t"]) // 2 < c["H"] * c["W"]


@pytest.mark.parametrize("offset", [0, 1])
def test_two_events_on_one_pixel(offset):
    tab, ref = _tables(R.case_two_events(offset))
    assert (ref["N"], ref["P"]) == (2, 1)


def test_window_without_a_pixel_that_fires_twice():
    c = R.case_no_pair()
    s = _stream(c)
    with pytest.raises(ValueError, match="no pixel with two events"):
        s.tables(0, 3)
    assert s.last_report == {"N": 0, "P": 0, "bad": 0}


def test_segment_lengths_either_side_of_each_sort_route():
    c = R.case_segment_boundaries()
    tab, ref = _tables(c)
    assert set(R.SEGMENT_LENGTHS[1:]) <= set(ref["num_at_xy"].tolist()) and ref["P"] == 35


def test_more_long_segments_than_workgroups_and_same_bits_on_two_runs():
    c = R.case_many_long_segments()
    tab, ref = _tables(c)
    assert ref["P"] == 1230 and ref["num_at_xy"].min() > 32
    again = _stream(c).tables(c["first"], c["last"])
    for k in R.KEYS:
        assert torch.equal(tab[k], again[k]), k


@pytest.mark.parametrize("unit", R.TIME_UNITS, ids=["ns", "offset", "ns-offset"])
def test_time_units_and_stream_offset(unit):
    c = R.case_time_units(*unit)
    c["span"] = R.time_units_span(c)
    ref = R.reference(c)
    tab, seen, nev, report = _batch(c)
    assert _equal(tab, ref) and report == {"N": ref["N"], "P": ref["P"], "bad": 0}
    rows, e = R.candidates(c)
    _rows_equal(seen, rows)
    assert nev["N_ev_chunks"] == 3 and nev["start_time_us"] == e[:-1]
    alone = _batch(c, tables=False)[1]
    _rows_equal(alone, rows)


# ---- C: bitmaps and chunk edges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sensor", R.SENSORS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bitmap_words_and_chunk_edges(sensor):
    H, W = sensor
    for span in R.SPANS:
        cases = [R.case_edge_events(H, W, span), R.case_full_and_empty_chunks(H, W, span, True)]
        if span[0] == 1:
            cases.append(R.case_full_and_empty_chunks(H, W, span, False))
        for c in cases:
            rows, e = R.candidates(c)
            _, seen, nev, _ = _batch(c, tables=False)
            _rows_equal(seen, rows)
            assert nev["N_ev_chunks"] == span[0] and nev["start_time_us"] == e[:-1]
        assert len(rows[0]) == (H * W if span[0] == 1 else 0)              # (the last case: none fires / every pixel fires)
        assert span[0] == 1 or len(rows[1]) == H * W


@pytest.mark.parametrize("sensor", R.SENSORS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mapped", [False, True], ids=["identity", "map"])
def test_no_event_coords(sensor, mapped):
    L, lib = _lib()
    H, W = sensor
    HW = H * W
    rect32 = R.frac_map(H, W).astype(np.float32)
    rect = torch.from_numpy(rect32).to(DEV) if mapped else None
    pixels = np.array([HW - 1, -1, 0, HW, HW // 2, 1, HW - 1], np.int64)
    d_pix = torch.from_numpy(pixels).to(DEV)
    buf, xy = _guarded((len(pixels), 2), torch.float32)
    bad_buf, bad = _guarded((1,), torch.int32)
    bad.fill_(7)
    L.check(lib.enerf_no_event_coords(d_pix.data_ptr(), len(pixels), rect.data_ptr() if mapped else None, H, W, xy.data_ptr(),
                                      bad.data_ptr(), L.stream_handle()), "no_event_coords")
    ok = (pixels >= 0) & (pixels < HW)
    q = np.where(ok, pixels, 0)
    want = rect32.reshape(-1, 2)[q] if mapped else np.stack([q % W, q // W], 1).astype(np.float32)
    want[~ok] = np.nan
    assert np.array_equal(xy.cpu().numpy(), want, equal_nan=True) and int(bad) == 7 + 2
    assert _intact(buf) and _intact(bad_buf) and np.array_equal(d_pix.cpu().numpy(), pixels)
    # n = 0: the one dummy pixel, nothing counted
    buf, xy = _guarded((1, 2), torch.float32)
    L.check(lib.enerf_no_event_coords(None, 0, rect.data_ptr() if mapped else None, H, W, xy.data_ptr(), bad.data_ptr(),
                                      L.stream_handle()), "no_event_coords")
    assert xy.cpu().tolist() == [[0.0, 0.0]] and int(bad) == 9 and _intact(buf) and _intact(bad_buf)


# ---- D: the entry points on guarded buffers ----------------------------------------------------------------------------
def _direct(c):
    """enerf_event_tables_count / _fill / enerf_no_event_coords called as the wrapper calls them, every output in a buffer
    with canaries either side -> (tables dict, candidate rows, coords of each chunk's first three candidates)."""
    L, lib = _lib()
    H, W, first, last = c["H"], c["W"], c["first"], c["last"]
    HW = H * W
    ns_per_unit = 1e6 / float(c["unit_per_ms"])
    ins = {k: torch.from_numpy(c[k]).to(DEV) for k in "xytp"}
    ins["p"] = torch.where(ins["p"] > 0, 1, -1).to(torch.int8)
    if c["rect"] is not None:
        ins["rect"] = torch.from_numpy(c["rect"].astype(np.float32)).to(DEV)
    e = R.edges(*c["span"]) if "span" in c else []
    n_chunks = max(len(e) - 1, 0)
    if n_chunks:
        ins["edges"] = torch.tensor(e, dtype=torch.float64, device=DEV)
    before = {k: v.clone() for k, v in ins.items()}
    ptr = lambda k: ins[k].data_ptr() if k in ins else None                # noqa: E731
    nbytes = ctypes.c_uint64(0)
    L.check(lib.enerf_event_tables_workspace(last - first, H, W, n_chunks, ctypes.byref(nbytes)), "workspace")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    bufs = {}

    def out(name, shape, dtype):
        bufs[name], inner = _guarded(shape, dtype)
        return inner

    report = out("report", (4 + n_chunks,), torch.int64)
    cand = out("candidates", (n_chunks, HW), torch.int64) if n_chunks else None
    stream = L.stream_handle()
    L.check(lib.enerf_event_tables_count(ptr("x"), ptr("y"), ptr("t"), first, last, H, W, ns_per_unit, c["t_offset"], 1,
                                         ptr("edges"), n_chunks, ws.data_ptr(), report.data_ptr(),
                                         cand.data_ptr() if n_chunks else None, stream), "count")
    rep = report.tolist()
    N, P = rep[0], rep[1]
    assert rep[2:4] == [0, 0] and N >= 2 and P >= 1
    tab = {"events": out("events", (N, 4), torch.float32), "no_successor": out("no_successor", (N,), torch.uint8),
           "num_successor": out("num_successor", (N,), torch.int64), "pol_cumsum": out("pol_cumsum", (N + 1,), torch.float64),
           "num_at_xy": out("num_at_xy", (P,), torch.int64), "first_at_xy": out("first_at_xy", (P,), torch.int64)}
    L.check(lib.enerf_event_tables_fill(ptr("x"), ptr("y"), ptr("t"), ptr("p"), first, last, H, W, ptr("rect"), ns_per_unit,
                                        c["t_offset"], ws.data_ptr(), n_chunks, N, P, tab["events"].data_ptr(),
                                        tab["no_successor"].data_ptr(), tab["num_successor"].data_ptr(),
                                        tab["pol_cumsum"].data_ptr(), tab["num_at_xy"].data_ptr(),
                                        tab["first_at_xy"].data_ptr(), stream), "fill")
    rows, coords = [], []
    for j in range(n_chunks):
        n = rep[4 + j]
        assert 0 <= n <= HW and bool((cand[j, n:] == UNWRITTEN[torch.int64]).all())   # the rest of the row is not written
        rows.append(cand[j, :n].cpu().numpy())
        sel = cand[j, :3].contiguous()
        xy = out(f"coords {j}", (3, 2), torch.float32)
        L.check(lib.enerf_no_event_coords(sel.data_ptr(), 3, ptr("rect"), H, W, xy.data_ptr(), None, stream), "no_event_coords")
        coords.append(xy)
    torch.cuda.synchronize()
    for name, buf in bufs.items():
        assert _intact(buf), name
    for k, v in ins.items():
        assert torch.equal(v, before[k]), k
    tab["no_successor"] = tab["no_successor"].view(torch.bool)
    return tab, rows, coords


def test_direct_calls_on_guarded_buffers_tables_and_candidates():
    c = R.case_time_units(1000, 123_456_789)
    c["span"] = R.time_units_span(c)
    tab, rows, coords = _direct(c)
    ref = R.reference(c)
    assert _equal(tab, ref)
    want_rows = R.candidates(c)[0]
    _rows_equal(rows, want_rows)
    assert all(len(r) >= 3 for r in rows)
    rect32 = c["rect"].astype(np.float32).reshape(-1, 2)
    for j in range(3):
        assert np.array_equal(coords[j].cpu().numpy(), rect32[want_rows[j][:3]]), j
    wtab, seen, nev, _ = _batch(c)                                         # the wrapper's
    for k in R.KEYS:
        assert torch.equal(tab[k], wtab[k]), k
    _rows_equal(rows, seen)


def test_direct_calls_on_guarded_buffers_segment_boundaries():
    c = R.case_segment_boundaries()
    tab, rows, _ = _direct(c)
    assert _equal(tab, R.reference(c)) and rows == []
    wtab = _stream(c).tables(c["first"], c["last"])
    for k in R.KEYS:
        assert torch.equal(tab[k], wtab[k]), k
