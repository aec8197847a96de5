"""enerf_amd/event_dataset.py without a GPU: the torch statement keyed on the sensor pixel against the loop restatement of
the reference (oracle/event_collate.py) on a fractional rectify map -- where build_event_tables merges pixels --, the
window borders of the two real-camera loaders against numbers worked by hand, the CPU route of EventStream, and the new
entry points' declarations."""
import ctypes
import re

import numpy as np
import pytest
import torch

from oracle import event_collate as O


def scale_map(H, W):
    """x' = 0.6 x + 0.3, y' = 0.6 y + 0.2: compresses, so neighbouring sensor pixels truncate into one cell."""
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    return np.stack([0.6 * xs + 0.3, 0.6 * ys + 0.2], axis=2)


def small_stream(seed=0, H=6, W=8, n=400):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, W, n).astype(np.uint16)
    y = rng.integers(0, H, n).astype(np.uint16)
    t = np.cumsum(rng.integers(1, 40, n)).astype(np.int64) + 1000          # microseconds, strictly ascending
    p = rng.integers(0, 2, n).astype(np.int8)                              # the h5 files' 0 / 1
    return x, y, t, p


def reference_rows(x, y, t, p, rect, ns_per_unit=1000.0, t_offset=0):
    """The [n, 4] fp32 rows the reference's loaders hand to the grouping loop, in stream order."""
    rect32 = rect.astype(np.float32)
    xi, yi = x.astype(np.int64), y.astype(np.int64)
    t_ns = ((t + t_offset).astype(np.float64) * ns_per_unit).astype(np.float32)
    return np.stack([rect32[yi, xi, 0], rect32[yi, xi, 1], t_ns, np.where(p > 0, 1.0, -1.0).astype(np.float32)], axis=1)


def assert_tables_equal_group(tab, g):
    cpu = {k: v.cpu() for k, v in tab.items() if torch.is_tensor(v)}
    assert np.array_equal(cpu["events"].numpy(), g["events"])
    assert np.array_equal(cpu["num_at_xy"].numpy(), g["xy_numEvs_Idx"][:, 0])
    assert np.array_equal(cpu["first_at_xy"].numpy(), g["xy_numEvs_Idx"][:, 1])
    assert np.array_equal(cpu["no_successor"].nonzero().flatten().numpy(), g["idx_no_successor"])
    assert np.array_equal(cpu["num_successor"].numpy(), g["num_successor_evs"])
    sums = np.concatenate([[0.0], np.cumsum(g["events"][:, 3].astype(np.float64))])
    assert np.array_equal(cpu["pol_cumsum"].numpy(), sums)


def test_statement_keeps_the_sensor_pixels_of_a_compressing_map_and_build_event_tables_does_not():
    from enerf_amd.event_dataset import tables_statement
    from enerf_amd.event_sampler import build_event_tables
    H, W = 6, 8
    x, y, t, p = small_stream()
    rect = scale_map(H, W)
    rows = reference_rows(x, y, t, p, rect)
    g = O.group_events(rows)
    assert len(g["xy_numEvs_Idx"]) == 48                                   # every sensor pixel has two events or more
    tab, bad = tables_statement(*(torch.from_numpy(a) for a in (x, y, t, p)), 0, len(t), H, W, rect)
    assert bad == 0
    assert_tables_equal_group(tab, g)
    merged = build_event_tables(torch.from_numpy(rows))                    # keyed on the truncated coordinates
    assert merged["num_at_xy"].shape[0] == 20
    assert merged["events"].shape == tab["events"].shape and not torch.equal(merged["events"], tab["events"])


def test_stream_on_the_cpu_runs_the_statement_and_the_no_event_statement():
    from enerf_amd.event_dataset import EventStream
    H, W = 6, 8
    x, y, t, p = small_stream(3)
    rect = scale_map(H, W)
    s = EventStream(x, y, t, p, H, W, rectify_map=rect)
    first, last = 17, 391
    g = O.group_events(reference_rows(x, y, t, p, rect)[first:last])
    tab = s.tables(first, last)
    assert_tables_equal_group(tab, g)
    assert s.last_report == {"N": len(g["events"]), "P": len(g["xy_numEvs_Idx"]), "bad": 0}
    assert tab["_packed"][1].dtype == torch.uint8 and tab["_packed"][0] is tab["events"]
    t0, t1 = float(t[first]), float(t[last - 1]) + 1.0
    picks = {}

    def choice(j, idxs, size):
        picks[j] = np.random.default_rng(40 + j).choice(idxs, size=size, replace=False) if size else idxs[:0]
        return picks[j]

    ev_ns = np.stack([x, y, t.astype(np.float64) * 1000.0], 1)[first:last]
    ref = O.no_event_tables(ev_ns, ev_ns[:, :2], H, W, t0, t1, rect, choice, chunk_len_ms=2.0)
    tab2, nev = s.batch_tables(first, last, t0, t1, chunk_len_ms=2.0,
                               keep=lambda j, cand: torch.from_numpy(picks[j].astype(np.int64) - 1))
    assert_tables_equal_group(tab2, g)
    assert nev["N_ev_chunks"] == ref["tss_bds"]["N_ev_chunks"][0] >= 3
    for j in range(nev["N_ev_chunks"]):
        assert np.array_equal(nev["coords"][j].numpy(), ref["coords"][j])
        assert nev["start_time_us"][j] == ref["tss_bds"]["start_time_us"][j]
        assert nev["end_time_us"][j] == ref["tss_bds"]["end_time_us"][j]
    assert s.window(float(t[first]), float(t[300])) == (first, 300)        # t0 <= t < t1, microseconds
    with pytest.raises(ValueError):
        s.tables(5, 5)
    with pytest.raises(ValueError):
        s.tables(0, 1)                                                      # no pixel with two events
    xb = x.copy()
    xb[100] = W
    sb = EventStream(xb, y, t, p, H, W, rectify_map=rect)
    with pytest.raises(ValueError):
        sb.tables(first, last)
    assert sb.last_report["bad"] == 1


def test_event_centres_worked_by_hand():
    """provider.py:174-178: one trigger period beyond the ends, half way between neighbours; :187-191: the 10 s cap."""
    from enerf_amd.event_dataset import event_centres
    tss = np.arange(20) * 50000.0                                           # 50 ms period
    c, shrink = event_centres(tss, [5, 2, 4], "tumvie")                     # frames at 100, 200, 250 ms
    # padded: 0, 100, 200, 250, 350 ms -> midpoints
    assert np.array_equal(c, [50000.0, 150000.0, 225000.0, 300000.0]) and shrink == 0.0
    tss = np.arange(400) * 50000.0                                          # 20 s
    c, shrink = event_centres(tss, [0, 100, 300], "tumvie")                 # frames at 0, 5, 15 s
    # padded: -0.1, 0, 5, 15, 15.1 s; the windows span 15.1 s: 5.1 s too many, shared by 3 windows x 2 ends
    assert np.array_equal(c, [-50000.0, 2500000.0, 10000000.0, 15050000.0]) and shrink == 850000.0
    tss = np.arange(10) * 40000.0
    c, shrink = event_centres(tss, [1, 2], "eds")                           # padded: -40, 40, 80, 160 ms
    assert np.array_equal(c, [0.0, 60000.0, 120000.0]) and shrink == 0.0
    c, shrink = event_centres(np.arange(400) * 40000.0, [0, 399], "eds")    # eds has no cap
    assert shrink == 0.0 and c[-1] - c[0] > 10e6
    with pytest.raises(ValueError):
        event_centres(tss, [1, 2], "esim")


def test_new_entry_points_are_declared_bound_and_the_header_stays_at_13():
    from enerf_amd import _lib as L
    from enerf_amd import build as B
    from enerf_amd import event_dataset as D
    names = ["enerf_event_tables_workspace", "enerf_event_tables_count", "enerf_event_tables_fill", "enerf_no_event_coords",
             "enerf_debug_event_segment_sort"]
    with open(L.HEADER_PATH) as f:
        header = f.read()
    assert L.header_abi_version() == 13 and "event_tables.hip" in B.SOURCES
    for n in names:
        assert n in L.SIGNATURES and re.search(r"^int " + n + r"\(", header, re.M), n
        assert getattr(L.lib(), n).argtypes == L.SIGNATURES[n]
    assert D.ENERF_EVT_SEGMENT_TILE == 4096 == int(re.search(r"ENERF_EVT_SEGMENT_TILE (\d+)", header).group(1))
    nbytes = ctypes.c_uint64(0)
    assert L.lib().enerf_event_tables_workspace(2000000, 480, 640, 3, ctypes.byref(nbytes)) == 0
    assert 480 * 640 * 16 + 2000000 * 4 < nbytes.value < 32 << 20
    assert L.lib().enerf_event_tables_workspace(0, 480, 640, 3, ctypes.byref(nbytes)) == -1
    assert L.lib().enerf_event_tables_workspace(100, 480, 1 << 20, 3, ctypes.byref(nbytes)) == -1
