"""csrc/event_tables.hip through enerf_amd/event_dataset.EventStream on the device, bit for bit against the
loop restatement of the reference (oracle/event_collate.py: group_events, no_event_tables) at the smallest shapes where
each mechanism can break: a sensor whose pixel count is no multiple of 32, a window strictly inside the stream whose length
is no multiple of a workgroup, segments sorted by a thread, in LDS and above the LDS tile, fp32 time ties, both polarity
encodings, the no-event chunks' edges, one event outside the sensor, and EventSampler.from_stream end to end."""
import numpy as np
import pytest
import torch

from oracle import event_collate as O
from test_event_dataset_host import assert_tables_equal_group, reference_rows, scale_map

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = 30, 41                                                              # 1230 pixels: no multiple of 32 or 64


def _stream(x, y, t, p, h, w, rect=None):
    from enerf_amd.event_dataset import EventStream
    return EventStream(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), torch.from_numpy(t).to(DEV),
                       torch.from_numpy(p).to(DEV), h, w, rectify_map=rect)


def _show(tab, x, y, t, p, first, last, h, w, rect):
    """Beside a mismatch: where the device tables leave the torch statement."""
    from enerf_amd.event_dataset import tables_statement
    st, _ = tables_statement(*(torch.from_numpy(a) for a in (x, y, t, p)), first, last, h, w, rect)
    for k in ("events", "num_at_xy", "first_at_xy", "no_successor", "num_successor", "pol_cumsum"):
        a, b = tab[k].cpu(), st[k]
        if a.shape != b.shape:
            print(f"{k}: device {tuple(a.shape)}, statement {tuple(b.shape)}")
        elif not torch.equal(a, b):
            bad = (a != b).reshape(a.shape[0], -1).any(1).nonzero().flatten()
            print(f"{k}: {bad.numel()} rows differ, first at {int(bad[0])}: device {a[bad[0]]}, statement {b[bad[0]]}")


def _check(tab, x, y, t, p, first, last, h, w, rect):
    eye = np.stack(np.meshgrid(np.arange(w), np.arange(h)), axis=2).astype(np.float64)
    g = O.group_events(reference_rows(x, y, t, p, eye if rect is None else rect)[first:last])
    try:
        assert_tables_equal_group(tab, g)
    except AssertionError:
        _show(tab, x, y, t, p, first, last, h, w, rect)
        raise
    ev, nos, nsucc, cs, num, fst = tab["_packed"]
    assert (ev.dtype, nos.dtype, nsucc.dtype, cs.dtype, num.dtype, fst.dtype) == (
        torch.float32, torch.uint8, torch.int64, torch.float64, torch.int64, torch.int64)
    assert all(v.is_cuda and v.is_contiguous() for v in tab["_packed"])
    return g


def _sensor_case(seed, n=5000, t0=1000, ties=True):
    """n events on the 30 x 41 sensor; pixel 0 fires once inside the window used below (and once before it), pixel 1
    exactly twice; time stamps repeat (steps of 0, 1, 2 microseconds)."""
    rng = np.random.default_rng(seed)
    pix = rng.integers(2, H * W, n)
    pix[50] = 0
    pix[1000] = 0
    pix[[2000, n - 500]] = 1
    x, y = (pix % W).astype(np.uint16), (pix // W).astype(np.uint16)
    t = (t0 + np.cumsum(rng.integers(0 if ties else 1, 3, n))).astype(np.int64)
    p = rng.integers(0, 2, n).astype(np.int8)
    return x, y, t, p


def test_fractional_map_window_inside_the_stream():
    x, y, t, p = _sensor_case(1)
    rect = scale_map(H, W)
    first, last = 137, 4871
    assert (last - first) % 256 != 0 and first > 0 and last < len(t)
    s = _stream(x, y, t, p, H, W, rect)
    tab = s.tables(first, last)
    g = _check(tab, x, y, t, p, first, last, H, W, rect)
    num = g["xy_numEvs_Idx"][:, 0]
    assert s.last_report == {"N": len(g["events"]), "P": len(num), "bad": 0}
    rect32 = rect.astype(np.float32)
    rows = g["events"]
    assert not ((rows[:, 0] == rect32[0, 0, 0]) & (rows[:, 1] == rect32[0, 0, 1])).any()       # one event: dropped
    assert int(((rows[:, 0] == rect32[0, 1, 0]) & (rows[:, 1] == rect32[0, 1, 1])).sum()) == 2  # two events: kept
    assert (num == 2).any() and num.max() <= 32                            # every segment sorted by one thread


@pytest.fixture(scope="module")
def long_segments():
    """4 x 4 sensor, 20 000 events: pixel 5 has ENERF_EVT_SEGMENT_TILE + 1000 of them (above the LDS tile), the other 15
    share the rest (about 1000 each: sorted in LDS)."""
    from enerf_amd.event_dataset import ENERF_EVT_SEGMENT_TILE
    rng = np.random.default_rng(2)
    n, hot = 20000, ENERF_EVT_SEGMENT_TILE + 1000
    others = np.array([q for q in range(16) if q != 5])
    pix = np.concatenate([np.full(hot, 5), others[rng.integers(0, 15, n - hot)]])
    pix = pix[rng.permutation(n)]
    x, y = (pix % 4).astype(np.uint16), (pix // 4).astype(np.uint16)
    t = (7 + np.cumsum(rng.integers(0, 3, n))).astype(np.int64)
    p = rng.integers(0, 2, n).astype(np.int8)
    rect = scale_map(4, 4)
    return x, y, t, p, rect, hot


def test_long_segments_in_lds_and_above_the_tile(long_segments):
    x, y, t, p, rect, hot = long_segments
    tab = _stream(x, y, t, p, 4, 4, rect).tables(0, len(t))
    g = _check(tab, x, y, t, p, 0, len(t), 4, 4, rect)
    num = g["xy_numEvs_Idx"][:, 0]
    assert num.max() == hot and len(num) == 16 and np.sort(num)[-2] <= 4096 and num.min() > 32


def test_same_bits_on_every_run(long_segments):
    x, y, t, p, rect, _ = long_segments
    s = _stream(x, y, t, p, 4, 4, rect)
    a, b = s.tables(0, len(t)), s.tables(0, len(t))
    for k in ("events", "num_at_xy", "first_at_xy", "no_successor", "num_successor", "pol_cumsum"):
        assert torch.equal(a[k], b[k]), k


def test_time_stamps_that_collide_in_fp32():
    """Near 5e7 us the fp32 nanoseconds are 4096 apart: consecutive microseconds are one fp32 value, and the order among
    them is stream order (the oracle's stable sort of the fp32 rows fed in stream order)."""
    x, y, t, p = _sensor_case(3, n=3000, t0=50_000_000, ties=False)
    rect = scale_map(H, W)
    rows = reference_rows(x, y, t, p, rect)
    assert len(np.unique(rows[:, 2])) < len(np.unique(t)) // 2
    tab = _stream(x, y, t, p, H, W, rect).tables(0, len(t))
    _check(tab, x, y, t, p, 0, len(t), H, W, rect)


def test_identity_map_and_signed_polarity():
    x, y, t, p = _sensor_case(4, n=3000)
    p = (2 * p - 1).astype(np.int8)                                        # esim's -1 / +1
    tab = _stream(x, y, t, p, H, W, None).tables(3, 2990)
    g = _check(tab, x, y, t, p, 3, 2990, H, W, None)
    assert set(np.unique(g["events"][:, 3])) == {-1.0, 1.0}
    assert np.array_equal(g["events"][:, :2], np.floor(g["events"][:, :2]))


def test_no_event_tables_three_chunks_with_the_tables_in_one_pass():
    """57 ms in three chunks of 19 ms: an event exactly on the edge between chunks 0 and 1 (belongs to 1), one past the
    last edge (belongs to none), every pixel firing in chunk 2 (the dummy row); the recorded choice of the oracle's run."""
    rng = np.random.default_rng(5)
    t0_us, dt = 1_000_000, 19_000
    rect = scale_map(H, W)
    parts = []
    for j, n in enumerate((500, 700)):                                     # sparse chunks: most pixels stay free
        parts.append((rng.integers(1, H * W, n), rng.integers(t0_us + j * dt, t0_us + (j + 1) * dt, n)))
    parts.append((np.array([0]), np.array([t0_us + dt])))                  # pixel 0, exactly on the edge
    parts.append((np.concatenate([np.arange(H * W), rng.integers(0, H * W, 300)]),
                  rng.integers(t0_us + 2 * dt, t0_us + 3 * dt, H * W + 300)))
    parts.append((np.array([7]), np.array([t0_us + 3 * dt + 5])))          # past the last edge
    pix, t = np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts]).astype(np.int64)
    order = np.argsort(t, kind="stable")
    pix, t = pix[order], t[order]
    assert not (pix[t < t0_us + dt] == 0).any()                            # pixel 0 is free in chunk 0 ...
    x, y = (pix % W).astype(np.uint16), (pix // W).astype(np.uint16)
    p = rng.integers(0, 2, len(t)).astype(np.int8)
    start_us, end_us = float(t0_us), float(t0_us + 3 * dt)
    picks = {}

    def choice(j, idxs, size):
        picks[j] = np.random.default_rng(60 + j).choice(idxs, size=size, replace=False) if size else idxs[:0]
        return picks[j]

    ev_ns = np.stack([x, y, t.astype(np.float64) * 1000.0], 1)
    ref = O.no_event_tables(ev_ns, ev_ns[:, :2], H, W, start_us, end_us, rect, choice, chunk_len_ms=20.0)
    assert ref["tss_bds"]["N_ev_chunks"][0] == 3 and ref["tss_bds"]["end_time_us"][0] == t0_us + dt
    keep = lambda j, cand: torch.from_numpy(picks[j].astype(np.int64) - 1)  # noqa: E731
    s = _stream(x, y, t, p, H, W, rect)
    tab, nev = s.batch_tables(0, len(t), start_us, end_us, chunk_len_ms=20.0, keep=keep)
    _check(tab, x, y, t, p, 0, len(t), H, W, rect)
    alone = s.no_event_tables(0, len(t), start_us, end_us, chunk_len_ms=20.0, keep=keep)
    assert s.last_report["N"] == 0
    for got in (nev, alone):
        assert got["N_ev_chunks"] == 3 and got["dt_us"] == ref["tss_bds"]["dt_us"][0]
        for j in range(3):
            assert got["coords"][j].dtype == torch.float32
            assert np.array_equal(got["coords"][j].cpu().numpy(), ref["coords"][j]), j
            assert got["start_time_us"][j] == ref["tss_bds"]["start_time_us"][j]
            assert got["end_time_us"][j] == ref["tss_bds"]["end_time_us"][j]
    assert nev["coords"][2].shape == (1, 2) and float(nev["coords"][2].abs().sum()) == 0.0
    # the candidates themselves: the pixels without an event in the chunk, ascending
    seen = []
    s.no_event_tables(0, len(t), start_us, end_us, chunk_len_ms=20.0,
                      keep=lambda j, cand: (seen.append(cand.cpu().numpy()), cand[:3])[1])
    tt = (t.astype(np.float64) * 1000.0) * 1e-3                            # the reference's microseconds
    for j in range(3):
        m = (tt >= ref["tss_bds"]["start_time_us"][j]) & (tt < ref["tss_bds"]["end_time_us"][j])
        hit = np.zeros(H * W, bool)
        hit[pix[m]] = True
        assert np.array_equal(seen[j], np.nonzero(~hit)[0]), j
    assert seen[0][0] == 0 and seen[1][0] != 0 and len(seen[2]) == 0       # the edge event fell into chunk 1
    # its own random choice: the right number, no duplicates, all event-free
    own = s.no_event_tables(0, len(t), start_us, end_us, chunk_len_ms=20.0,
                            generator=torch.Generator(device=DEV).manual_seed(1))
    rect32 = torch.from_numpy(rect.astype(np.float32))
    for j in range(2):
        c = own["coords"][j].cpu()
        assert c.shape[0] == len(seen[j]) // 3
        free = rect32.reshape(-1, 2)[torch.from_numpy(seen[j])]
        match = (c[:, None, :] == free[None, :, :]).all(2)
        assert bool(match.any(1).all()) and int(match.any(0).sum()) == c.shape[0]


def test_one_event_outside_the_sensor_is_counted_and_refused():
    x, y, t, p = _sensor_case(6, n=3000)
    x[1234] = W                                                            # one past the last column
    s = _stream(x, y, t, p, H, W, scale_map(H, W))
    with pytest.raises(ValueError, match="outside"):
        s.tables(0, len(t))
    assert s.last_report["bad"] == 1
    s.tables(1235, len(t))                                                 # a window without it is served


def _track(K, t_lo, t_hi, seed):
    from scipy.spatial.transform import Rotation
    from enerf_amd.pose_interp import PoseTrack
    rng = np.random.default_rng(seed)
    t = np.linspace(t_lo, t_hi, K)
    R = Rotation.from_rotvec(np.cumsum(rng.normal(size=(K, 3)) * 0.04, 0))
    pos = np.cumsum(rng.normal(size=(K, 3)) * 0.02, 0) + np.array([1.5, 0.3, 0.0])
    return PoseTrack(t, R.as_matrix(), pos, device=DEV)


@pytest.mark.parametrize("accumulate_evs", [0, 1])
def test_from_stream_equals_a_sampler_built_from_the_statement(accumulate_evs):
    from enerf_amd.event_dataset import tables_statement
    from enerf_amd.event_sampler import EventSampler, build_no_event_tables
    x, y, t, p = _sensor_case(7 + accumulate_evs, n=6000, t0=2000)
    rect = scale_map(H, W)
    s = _stream(x, y, t, p, H, W, rect)
    span = int(t[-1]) - 2000
    centres = [2000.0 + 0.1 * span, 2000.0 + 0.5 * span, 2000.0 + 0.8 * span]
    shrink = 0.02 * span
    track = _track(12, 1000.0 * 1e3, float(t[-1] + 1000) * 1e3, 3)
    intr = (35.0, 34.0, 20.0, 14.5)
    M = 256
    seed = 11
    got = EventSampler.from_stream(s, centres, track, intr, M, accumulate_evs=accumulate_evs, acc_max_num_evs=3,
                                   negative_event_sampling=1, shrink_us=shrink, seed=seed)
    assert len(got) == 2
    # the same tables from the torch statement (events) and build_no_event_tables on the sensor coordinates, with the
    # subsampling the stream drew
    gen = torch.Generator(device=DEV).manual_seed(seed)
    tabs, nevs = [], []
    dev = [torch.from_numpy(a).to(DEV) for a in (x, y, t, p)]
    for i in range(2):
        first, last = s.window(centres[i] + shrink, centres[i + 1] - shrink)
        assert np.all(t[first:last] >= centres[i] + shrink) and np.all(t[first:last] < centres[i + 1] - shrink)
        assert t[first - 1] < centres[i] + shrink and t[last] >= centres[i + 1] - shrink
        tab, bad = tables_statement(*dev, first, last, H, W, rect)
        assert bad == 0
        tabs.append(tab)
        ev = torch.stack([dev[0][first:last].double(), dev[1][first:last].double(), dev[2][first:last].double() * 1000.0], 1)
        nevs.append(build_no_event_tables(ev, H, W, centres[i], centres[i + 1], rectify_map=rect, generator=gen))
    want = EventSampler(tabs, track, intr, M, accumulate_evs, 3, no_events=nevs, seed=seed)
    rng = torch.Generator().manual_seed(5)
    for i in range(2):
        for k in ("events", "num_at_xy", "first_at_xy", "num_successor", "pol_cumsum"):
            assert torch.equal(got.tables[i][k], want.tables[i][k]), k
        for j in range(got.no_events[i]["N_ev_chunks"]):
            assert torch.equal(got.no_events[i]["coords"][j], want.no_events[i]["coords"][j]), (i, j)
        N, P = tabs[i]["events"].shape[0], tabs[i]["num_at_xy"].shape[0]
        n_chunks = nevs[i]["N_ev_chunks"]
        chunk = int(torch.randint(0, n_chunks, (1,), generator=rng))
        draws = {"chunk": chunk, "idx": torch.randint(0, nevs[i]["coords"][chunk].shape[0], (M // 2,), generator=rng),
                 "u": torch.rand(M // 2, 2, generator=rng, dtype=torch.float64)}
        if accumulate_evs:
            draws.update(start=torch.randint(0, N, (M,), generator=rng), u_end=torch.rand(M, generator=rng, dtype=torch.float64))
        else:
            draws.update(u_xy=torch.rand(P, generator=rng, dtype=torch.float64), choice=torch.randint(0, P, (M,), generator=rng))
        a, b = got.batch(i, draws=draws), want.batch(i, draws=draws)
        for k in ("rays_evs_o1", "rays_evs_d1", "rays_evs_o2", "rays_evs_d2", "pols", "start", "end", "rays_no_evs_o1",
                  "rays_no_evs_d1", "rays_no_evs_o2", "rays_no_evs_d2"):
            assert torch.equal(a[k], b[k]), k
        assert int(a["outside_track"]) == 0 and int(a["no_evs_outside_track"]) == 0
