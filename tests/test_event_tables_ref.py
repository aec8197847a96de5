"""tests/event_tables_ref.py (the numpy statement the device tests of csrc/event_tables.hip compare with) pinned without a
GPU: equal, bit for bit, to the loop restatement of the reference (oracle/event_collate.py: group_events, no_event_tables)
on the small cases -- the loops are slow: a few thousand events at the most -- and to the torch statement
(enerf_amd.event_dataset.tables_statement, event_sampler.build_no_event_tables) on every case the device tests run, at
full size.  So each big case has two independent CPU statements agreeing before a GPU sees it."""
import time

import numpy as np
import pytest
import torch

import event_tables_ref as R
from oracle import event_collate as O
from test_event_dataset_host import assert_tables_equal_group, reference_rows, scale_map, small_stream


def _as_torch(ref):
    return {k: torch.from_numpy(np.ascontiguousarray(ref[k])) for k in R.KEYS}


def _oracle_equal(c):
    """The reference of the case against the grouping loop."""
    H, W = c["H"], c["W"]
    eye = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=2).astype(np.float64)
    rows = reference_rows(c["x"], c["y"], c["t"], c["p"], eye if c["rect"] is None else c["rect"],
                          1e6 / float(c["unit_per_ms"]), c["t_offset"])
    g = O.group_events(rows[c["first"]:c["last"]])
    ref = R.reference(c)
    assert_tables_equal_group(_as_torch(ref), g)
    assert ref["N"] == len(g["events"]) and ref["P"] == len(g["xy_numEvs_Idx"])
    return ref, g


def _statement_equal(c):
    """The reference of the case against the torch statement on CPU tensors."""
    from enerf_amd.event_dataset import tables_statement
    ref = R.reference(c)
    st, bad = tables_statement(*(torch.from_numpy(c[k]) for k in "xytp"), c["first"], c["last"], c["H"], c["W"], c["rect"],
                               1e6 / float(c["unit_per_ms"]), c["t_offset"])
    assert bad == 0
    for k in R.KEYS:
        a, b = ref[k], st[k].numpy()
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
    return ref


def _statement_candidates_equal(c):
    """no_event_candidates of the case against build_no_event_tables on the sensor coordinates (the CPU route)."""
    from enerf_amd.event_sampler import build_no_event_tables
    rows, e = R.candidates(c)
    sl = slice(c["first"], c["last"])
    t_ns = (torch.from_numpy(c["t"][sl]) + c["t_offset"]).to(torch.float64) * (1e6 / float(c["unit_per_ms"]))
    ev = torch.stack([torch.from_numpy(c["x"][sl].astype(np.float64)), torch.from_numpy(c["y"][sl].astype(np.float64)), t_ns], 1)
    seen = []
    start_us, end_us, chunk_len_ms = c["span"]
    nev = build_no_event_tables(ev, c["H"], c["W"], start_us, end_us, chunk_len_ms,
                                keep=lambda j, cand: (seen.append(cand.numpy()), cand[:1])[1])
    assert nev["N_ev_chunks"] == len(rows) == len(e) - 1
    assert nev["start_time_us"] == e[:-1]
    for j, row in enumerate(rows):
        assert row.dtype == seen[j].dtype and np.array_equal(row, seen[j]), j
    return rows


# ---- against the loop oracle: the existing small cases and the small new ones ------------------------------------------
def test_reference_equals_the_grouping_loop_on_the_existing_small_cases():
    from test_gpu_event_dataset import H, W, _sensor_case
    x, y, t, p = small_stream()
    _oracle_equal(R._case(y.astype(np.int64) * 8 + x, t, p, 6, 8, rect=False) | {"rect": scale_map(6, 8)})
    x, y, t, p = small_stream(3)
    _oracle_equal(R._case(y.astype(np.int64) * 8 + x, t, p, 6, 8, rect=False, first=17, last=391) | {"rect": scale_map(6, 8)})
    pix = lambda x, y: y.astype(np.int64) * W + x                          # noqa: E731
    x, y, t, p = _sensor_case(1)                                           # the fractional map, a window inside the stream
    ref, g = _oracle_equal(R._case(pix(x, y), t, p, H, W, rect=False, first=137, last=4871) | {"rect": scale_map(H, W)})
    assert g["xy_numEvs_Idx"][:, 0].min() == 2
    x, y, t, p = _sensor_case(3, n=3000, t0=50_000_000, ties=False)        # stamps that collide in fp32
    _oracle_equal(R._case(pix(x, y), t, p, H, W, rect=False) | {"rect": scale_map(H, W)})
    x, y, t, p = _sensor_case(4, n=3000)                                   # identity map, -1 / +1 polarity
    ref, g = _oracle_equal(R._case(pix(x, y), t, (2 * p - 1), H, W, rect=False, first=3, last=2990))
    assert np.array_equal(ref["events"][:, :2], np.floor(ref["events"][:, :2])) and set(np.unique(ref["events"][:, 3])) == {-1.0, 1.0}


@pytest.mark.parametrize("case", [lambda: R.case_exact_fit(0), lambda: R.case_exact_fit(1), lambda: R.case_two_events(0),
                                  lambda: R.case_two_events(1)] + [lambda u=u: R.case_time_units(*u) for u in R.TIME_UNITS],
                         ids=["fit-even", "fit-odd", "two", "two-offset", "ns", "offset", "ns-offset"])
def test_reference_equals_the_grouping_loop_on_the_small_new_cases(case):
    c = case()
    assert c["last"] - c["first"] < 6000
    _oracle_equal(c)


def test_no_event_candidates_equal_the_loop_oracles():
    """provider.py:1283-1351 restated (no_event_tables): the index list it hands to np.random.choice is 1-based."""
    for H, W in R.SENSORS:
        for span in R.SPANS:
            cases = [R.case_edge_events(H, W, span), R.case_full_and_empty_chunks(H, W, span, True),
                     R.case_full_and_empty_chunks(H, W, span, False)]
            for c in cases:
                rows, e = R.candidates(c)
                seen = {}

                def choice(j, idxs, size):
                    seen[j] = idxs.astype(np.int64) - 1
                    return idxs[:0]

                ev_ns = np.stack([c["x"], c["y"], c["t"].astype(np.float64) * 1000.0], 1)
                ref = O.no_event_tables(ev_ns, ev_ns[:, :2], H, W, c["span"][0], c["span"][1], np.zeros((H, W, 2)), choice,
                                        chunk_len_ms=c["span"][2])
                assert ref["tss_bds"]["N_ev_chunks"][0] == span[0] == len(rows)
                assert ref["tss_bds"]["start_time_us"] == e[:-1]
                for j in range(span[0]):
                    assert np.array_equal(rows[j], seen[j]), (H, W, span, j)


# ---- against the torch statement: every case of the device tests, at full size ----------------------------------------
def test_scan_carry_case():
    c = R.case_scan_carry()
    ref = _statement_equal(c)
    assert ref["N"] == len(c["t"]) == R.SCAN_TILE * 257 + 3 and ref["P"] == 30 * 41
    assert ref["pol_cumsum"][R.SCAN_TOP] < -350_000                        # where k_scan_top's carry enters


def test_big_sensor_case_and_the_reference_time():
    c = R.case_big_sensor()
    HW = c["H"] * c["W"]
    assert HW % 32 == 0 and HW > R.SCAN_TOP and 32 * (HW // 32) > R.SCAN_TOP
    t0 = time.perf_counter()
    ref = R.reference(c)
    t1 = time.perf_counter()
    rows, e = R.candidates(c)
    t2 = time.perf_counter()
    print(f"big sensor: tables {t1 - t0:.2f} s, candidates {t2 - t1:.2f} s")
    E = len(c["t"])
    assert ref["P"] == HW == min(E // 2, HW) and ref["N"] == E               # P = pmax - 1, through the H * W branch
    assert len(rows) == 32 and len(rows[c["empty"]]) == HW and all(len(rows[j]) >= HW - 200 for j in c["sparse"])
    assert all(0 < len(r) < HW - 200 for j, r in enumerate(rows) if j != c["empty"] and j not in c["sparse"])
    _statement_equal(c)
    _statement_candidates_equal(c)


@pytest.mark.parametrize("case", [R.case_segment_boundaries, R.case_many_long_segments, lambda: R.case_exact_fit(0),
                                  lambda: R.case_exact_fit(1), lambda: R.case_two_events(0), lambda: R.case_two_events(1)],
                         ids=["boundaries", "many-long", "fit-even", "fit-odd", "two", "two-offset"])
def test_small_sensor_cases(case):
    c = case()
    ref = _statement_equal(c)
    E, HW = c["last"] - c["first"], c["H"] * c["W"]
    assert 1 <= ref["P"] < min(E // 2, HW) + 1


def test_the_cases_are_what_they_say():
    c = R.case_segment_boundaries()
    ref = R.reference(c)
    pix = c["y"].astype(np.int64) * 6 + c["x"]
    assert tuple(int((pix == q).sum()) for q in c["pixels"]) == R.SEGMENT_LENGTHS
    assert ref["P"] == 35 and set(R.SEGMENT_LENGTHS[1:]) <= set(ref["num_at_xy"].tolist())
    ref = R.reference(R.case_many_long_segments())
    assert ref["P"] == 1230 > 1024 and ref["num_at_xy"].min() == 36 and ref["num_at_xy"].max() == 40
    for odd in (0, 1):
        c = R.case_exact_fit(odd)
        ref = R.reference(c)
        assert len(c["t"]) == 1400 + odd and ref["P"] == 700 == len(c["t"]) // 2 and ref["N"] == 1400
    for off in (0, 1):
        ref = R.reference(R.case_two_events(off))
        assert (ref["N"], ref["P"]) == (2, 1) and ref["order"].tolist() == [0, 1]
    ref = R.reference(R.case_no_pair())
    assert (ref["N"], ref["P"]) == (0, 0) and ref["pol_cumsum"].tolist() == [0.0]


@pytest.mark.parametrize("unit", R.TIME_UNITS, ids=["ns", "offset", "ns-offset"])
def test_time_unit_cases(unit):
    c = R.case_time_units(*unit)
    ref = _statement_equal(c)
    t_win = c["t"][c["first"]:c["last"]]
    assert len(np.unique(ref["events"][:, 2])) < len(np.unique(t_win)) // 2  # distinct stamps collide in fp32
    c["span"] = R.time_units_span(c)
    rows = _statement_candidates_equal(c)
    assert len(rows) == 3 and c["span"][0] != np.floor(c["span"][0])
    hw = c["H"] * c["W"]
    assert all(0 < len(r) < hw for r in rows)


@pytest.mark.parametrize("sensor", R.SENSORS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bitmap_cases(sensor):
    H, W = sensor
    for span in R.SPANS:
        _statement_candidates_equal(R.case_edge_events(H, W, span))
        rows = _statement_candidates_equal(R.case_full_and_empty_chunks(H, W, span, True))
        assert len(rows[0]) == 0 and (span[0] == 1 or len(rows[1]) == H * W)
        if span[0] == 1:
            rows = _statement_candidates_equal(R.case_full_and_empty_chunks(H, W, span, False))
            assert len(rows[0]) == H * W


def test_sort_segments_are_unique_entries_of_the_whole_range_between_canaries():
    fill = [f for _ in R.SORT_LENGTHS for f in R.FILLINGS]
    lengths = [n for n in R.SORT_LENGTHS for _ in R.FILLINGS]
    idx, N, num, first, want = R.segments(lengths, fill, seed=1)
    inside = np.zeros(idx.size, bool)
    for n, b in zip(num, first):
        inside[b:b + n] = True
    assert N == int(first[-1] + num[-1]) and idx.size == N + 5 and not inside[N:].any()
    vals = idx[inside]
    assert len(np.unique(vals)) == vals.size and vals.min() == 0 and vals.max() == 0xfffffffe
    assert (idx[~inside] == R.CANARY).all() and (want[~inside] == R.CANARY).all() and (~inside).sum() == 3 * len(num) + 5
    k = lengths.index(4097)
    for j, f in enumerate(R.FILLINGS):
        seg = idx[first[k + j]:first[k + j] + 4097].astype(np.int64)
        d = np.diff(seg)
        assert {"ascending": (d > 0).all(), "descending": (d < 0).all(), "shuffled": (d > 0).any() and (d < 0).sum() > 1000,
                "smallest last": (d[:-1] > 0).all() and seg[-1] == seg.min()}[f], f
        assert np.array_equal(want[first[k + j]:first[k + j] + 4097], np.sort(seg))
