"""The loader's side of EventStream on CPU tensors: the numpy statement (tests/event_stats_ref.py) against
the reference's own render_ev_accumulation (tests/golden/ref_event_accumulation.npz, minted by
tests/refcheck/mint_event_accumulation_golden.py), the CPU route of pixel_counts / accumulation_image / hot_pixels /
without_pixels against the statement, known answers worked out by hand, every refusal, and the pictures
EventSampler.from_stream writes.  Nothing here is rounded: every comparison is exact."""
import os

import numpy as np
import pytest
import torch

import event_stats_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_event_accumulation.npz")


def _stream(c, H, W, rect=None, **kw):
    from enerf_amd.event_dataset import EventStream
    return EventStream(*(torch.from_numpy(np.asarray(c[k])) for k in "xytp"), H, W, rectify_map=rect, **kw)


def _columns(s):
    return tuple(v.numpy() for v in (s.x, s.y, s.t, s.p))


# ---- the statement against the reference's function ----------------------------------------------------------------------
def test_statement_reproduces_the_reference_pictures():
    z = np.load(GOLDEN)
    H, W = int(z["H"]), int(z["W"])
    names = sorted(k[:-4] for k in z.files if k.endswith("_img"))
    assert names == ["float_coords", "one_pixel", "sensor_01", "sensor_pm1", "single"]
    for n in names:
        img = R.render(z[n + "_x"], z[n + "_y"], z[n + "_pol"], H, W)
        assert img.dtype == z[n + "_img"].dtype == np.uint8 and np.array_equal(img, z[n + "_img"]), n
    # the fixture holds what it was made for: both colours, cells hit under both polarities, coordinates off the sensor
    x, y, pol = z["sensor_pm1_x"].astype(int), z["sensor_pm1_y"].astype(int), z["sensor_pm1_pol"]
    both = set(zip(y[pol > 0], x[pol > 0])) & set(zip(y[pol < 0], x[pol < 0]))
    assert len(both) > 20
    xf, yf = z["float_coords_x"], z["float_coords_y"]
    assert (xf < 0).any() and (xf >= W).any() and ((xf >= W - 1) & (xf < W)).any() and (xf == W).any()
    assert (yf < 0).any() and (yf >= H).any() and ((yf >= H - 1) & (yf < H)).any() and (yf == H).any()
    assert np.array_equal(z["one_pixel_img"][2, 3], [0, 0, 255]) and (z["one_pixel_img"] != 255).any(-1).sum() == 1


def test_the_stream_draws_the_reference_picture_of_sensor_events():
    """The same fixture through EventStream: sensor coordinates, -1/+1 and 0/1 polarities."""
    z = np.load(GOLDEN)
    H, W = int(z["H"]), int(z["W"])
    for n in ("sensor_pm1", "sensor_01", "single", "one_pixel"):
        x = z[n + "_x"]
        c = {"x": x.astype(np.int64), "y": z[n + "_y"].astype(np.int64), "t": np.arange(x.size, dtype=np.int64), "p": z[n + "_pol"]}
        img = _stream(c, H, W).accumulation_image(0, x.size)
        assert img.dtype == torch.uint8 and np.array_equal(img.numpy(), z[n + "_img"]), n


# ---- the CPU route against the statement -------------------------------------------------------------------------------------
CASES = [(6, 8, 400, 11), (33, 65, 5000, 12), (48, 64, 20000, 13)]


@pytest.mark.parametrize("H,W,E,seed", CASES)
def test_cpu_route_equals_the_statement(H, W, E, seed):
    c = R.random_stream(seed, E, H, W, hot=3, hot_share=0.2)
    rect = R.random_map(seed, H, W)
    s = _stream(c, H, W, rect)
    for first, last in ((0, E), (E // 3, E // 3 + max(1, E // 2)), (E - 1, E)):
        w = {k: v[first:last] for k, v in c.items()}
        counts = s.pixel_counts(first, last)
        assert counts.dtype == torch.int32 and tuple(counts.shape) == (H, W, 2)
        assert np.array_equal(counts.numpy(), R.pixel_counts(w["x"], w["y"], w["p"], H, W))
        assert s.last_report == {"events": last - first, "bad": 0}
        assert int(counts.sum()) == last - first
        img = s.accumulation_image(first, last)
        assert img.dtype == torch.uint8 and np.array_equal(img.numpy(), R.accumulation_image(w["x"], w["y"], w["p"], H, W))
        img = s.accumulation_image(first, last, rectified=True)
        assert np.array_equal(img.numpy(), R.accumulation_image(w["x"], w["y"], w["p"], H, W, rect))
        for kw in ({"n_sigma": 0.0}, {"n_sigma": 1.5}, {"n_sigma": 5}, {"max_count": 3}):
            mask = s.hot_pixels(first, last, **kw)
            ref, report = R.hot_pixels(w["x"], w["y"], w["p"], H, W, **kw)
            assert mask.dtype == torch.bool and np.array_equal(mask.numpy(), ref)
            assert s.last_report == report
    mask = s.hot_pixels(n_sigma=1.5)                                       # the whole stream by default
    assert 0 < s.last_report["hot"] < H * W and s.last_report["events"] == E
    out = s.without_pixels(mask)
    for a, b in zip(_columns(out), R.without_pixels(c["x"], c["y"], c["t"], c["p"], mask.numpy())):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert s.last_report == {"kept": len(out), "removed": E - len(out)} and s.last_report["removed"] > 0
    assert torch.equal(out.rectify_map.view(torch.int32), s.rectify_map.view(torch.int32))       # (bits: the map has NaNs)


# ---- hot pixels by hand --------------------------------------------------------------------------------------------------------
def _repeat_stream(pixels_and_counts, W):
    """A stream with `count` events at each (y, x), interleaved; -> columns dict."""
    ys, xs = [], []
    for (y, x), n in pixels_and_counts:
        ys += [y] * n
        xs += [x] * n
    order = np.random.default_rng(5).permutation(len(xs))
    x, y = np.asarray(xs)[order], np.asarray(ys)[order]
    return {"x": x, "y": y, "t": np.arange(x.size, dtype=np.int64) * 7, "p": np.where(np.arange(x.size) % 3 == 0, 1, -1)}


def test_hot_pixels_equal_counts_have_no_outlier():
    """Every active pixel holds 5 events: mu = 5, Q / n = 25, sigma = 0, T = 5 for any n_sigma: nothing is above it."""
    H, W = 6, 8
    c = _repeat_stream([((y, x), 5) for y in range(H) for x in range(0, W, 2)], W)
    s = _stream(c, H, W)
    for n_sigma in (0, 0.5, 3, 100.0):
        assert not s.hot_pixels(n_sigma=n_sigma).any()
        assert s.last_report == {"active": 24, "events": 120, "threshold": 5, "hot": 0, "hot_events": 0}


def test_hot_pixels_one_outlier_among_singles():
    """One pixel with 1000 events and 47 with one: n = 48, S = 1047, Q = 1 000 047; mu = 21.8125, sigma = sqrt(Q / n -
    mu^2) = sqrt(20358.52...) = 142.68...; n_sigma = 3 -> T = floor(449.86...) = 449: the one pixel; n_sigma = 7 -> T =
    floor(1020.59...) = 1020: none; n_sigma = 0 -> T = 21: the one pixel."""
    H, W = 6, 8
    cells = [(y, x) for y in range(H) for x in range(W)]
    c = _repeat_stream([(cells[17], 1000)] + [(q, 1) for q in cells[:17] + cells[18:]], W)
    s = _stream(c, H, W)
    for n_sigma, T, hot in ((3, 449, 1), (7, 1020, 0), (0, 21, 1)):
        mask = s.hot_pixels(n_sigma=n_sigma)
        assert s.last_report == {"active": 48, "events": 1047, "threshold": T, "hot": hot, "hot_events": 1000 * hot}
        want = np.zeros((H, W), bool)
        want[cells[17]] = bool(hot)
        assert np.array_equal(mask.numpy(), want)


def test_hot_pixels_max_count_is_a_strict_bound():
    H, W = 6, 8
    c = _repeat_stream([((1, 2), 9), ((3, 4), 10), ((5, 7), 11), ((0, 0), 1)], W)
    s = _stream(c, H, W)
    for max_count, hot in ((9, [(3, 4), (5, 7)]), (10, [(5, 7)]), (11, []), (0, [(1, 2), (3, 4), (5, 7), (0, 0)])):
        mask = s.hot_pixels(max_count=max_count)
        assert sorted(map(tuple, np.argwhere(mask.numpy()))) == sorted(hot)
        assert s.last_report["threshold"] == max_count and s.last_report["hot"] == len(hot)
        assert s.last_report["active"] == 4 and s.last_report["events"] == 31


# ---- without_pixels ------------------------------------------------------------------------------------------------------------
def test_without_pixels_is_boolean_indexing_and_keeps_the_stream_usable():
    H, W, E = 33, 65, 6000
    c = R.random_stream(21, E, H, W)
    rect = R.random_map(21, H, W)
    from enerf_amd.event_dataset import EventStream
    s = _stream(c, H, W, rect, unit_per_ms=1000, t_offset=123)
    mask = torch.zeros(H, W, dtype=torch.bool)
    mask[::2, 1::2] = True
    mask[1::2, ::2] = True
    out = s.without_pixels(mask)
    keep = ~mask.numpy()[c["y"].astype(int), c["x"].astype(int)]
    for a, k in zip(_columns(out), "xytp"):
        assert np.array_equal(a, c[k][keep])
    assert (out.H, out.W, out.unit_per_ms, out.t_offset) == (H, W, 1000, 123)
    assert torch.equal(out.rectify_map.view(torch.int32), s.rectify_map.view(torch.int32))       # (bits: the map has NaNs)
    assert s.last_report == {"kept": int(keep.sum()), "removed": int((~keep).sum())}
    fresh = EventStream(*(torch.from_numpy(c[k][keep]) for k in "xytp"), H, W, rect, 1000, 123)
    assert torch.equal(out.index.ms_to_idx, fresh.index.ms_to_idx)
    t0 = float(c["t"][0] + 123)
    for a, b in ((t0 + 1000.5, t0 + 9000.25), (t0, t0 + 30000), (t0 + 20000, t0 + 20001)):
        assert out.window(a, b) == fresh.window(a, b)
    # nothing masked: an equal stream
    same = s.without_pixels(torch.zeros(H, W, dtype=torch.bool))
    for a, k in zip(_columns(same), "xytp"):
        assert np.array_equal(a, c[k])
    assert s.last_report == {"kept": E, "removed": 0}
    with pytest.raises(ValueError, match="removes every event"):
        s.without_pixels(torch.ones(H, W, dtype=torch.bool))
    assert s.last_report == {"kept": 0, "removed": E}


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_every_refusal():
    H, W, E = 6, 8, 50
    c = R.random_stream(3, E, H, W)
    s = _stream(c, H, W)
    calls = (lambda a, b: s.pixel_counts(a, b), lambda a, b: s.accumulation_image(a, b),
             lambda a, b: s.hot_pixels(a, b, max_count=1))
    for call in calls:
        with pytest.raises(ValueError, match="empty window"):
            call(7, 7)
        for a, b in ((-1, 4), (0, E + 1), (9, 3), (E + 1, E + 2)):
            with pytest.raises(ValueError, match="window"):
                call(a, b)
    with pytest.raises(ValueError, match="rectify_map"):
        s.accumulation_image(0, E, rectified=True)
    for kw in ({}, {"n_sigma": 2.0, "max_count": 5}):
        with pytest.raises(ValueError, match="exactly one"):
            s.hot_pixels(**kw)
    for kw in ({"n_sigma": -1.0}, {"n_sigma": float("nan")}, {"max_count": -1}, {"max_count": 2.5}):
        with pytest.raises(ValueError):
            s.hot_pixels(**kw)
    for bad_mask in (torch.zeros(H, W + 1, dtype=torch.bool), torch.zeros(H * W, dtype=torch.bool),
                     torch.zeros(H, W, dtype=torch.uint8), np.zeros((H, W), bool), torch.zeros(H, W, dtype=torch.bool, device="meta")):
        with pytest.raises(ValueError, match="mask"):
            s.without_pixels(bad_mask)
    # events outside the sensor: counted, named, and nothing is indexed with them
    for col, v in (("x", W), ("y", H), ("x", 65535)):
        d = {k: a.copy() for k, a in c.items()}
        d[col][[4, 20]] = v
        o = _stream(d, H, W, R.random_map(1, H, W))
        for call in (lambda: o.pixel_counts(0, E), lambda: o.accumulation_image(0, E),
                     lambda: o.accumulation_image(0, E, rectified=True), lambda: o.hot_pixels(n_sigma=1.0),
                     lambda: o.without_pixels(torch.zeros(H, W, dtype=torch.bool))):
            with pytest.raises(ValueError, match=f"2 event.s. outside the {W} x {H} sensor"):
                call()
            assert o.last_report == {"bad": 2}
        assert int(o.pixel_counts(5, 20).sum()) == 15                      # a window without them is served


def test_a_window_of_more_than_2_30_events_is_refused():
    """The limit of one call, checked on the arguments alone (a stream whose columns are meta tensors holds no memory)."""
    from enerf_amd.event_dataset import EventStream
    s = EventStream.__new__(EventStream)
    E = (1 << 30) + 1
    s.x = s.y = s.t = s.p = torch.empty(E, dtype=torch.int8, device="meta")
    s.H, s.W, s.device, s.rectify_map, s.last_report = 6, 8, torch.device("cpu"), None, None
    for call in (lambda: s.pixel_counts(0, E), lambda: s.accumulation_image(0, E), lambda: s.hot_pixels(max_count=1),
                 lambda: s.without_pixels(torch.zeros(6, 8, dtype=torch.bool, device="meta"))):
        with pytest.raises(ValueError, match="2\\^30"):
            call()


# ---- the pictures of from_stream ---------------------------------------------------------------------------------------------------
def _sampler_inputs():
    from enerf_amd.event_dataset import event_centres
    from enerf_amd.pose_interp import PoseTrack
    H, W, E = 12, 16, 6000
    g = np.random.default_rng(8)
    c = {"x": g.integers(0, W, E), "y": g.integers(0, H, E), "t": np.sort(g.integers(0, 100_000, E)).astype(np.int64),
         "p": g.choice(np.array([-1, 1]), E)}
    tss = np.arange(0, 6) * 20_000.0 + 10_000.0
    centres, shrink = event_centres(tss, [1, 2, 3], "eds")
    return H, W, c, centres, shrink, PoseTrack


def test_from_stream_writes_the_reference_pictures(tmp_path):
    from PIL import Image
    from enerf_amd.event_sampler import EventSampler
    H, W, c, centres, shrink, PoseTrack = _sampler_inputs()
    rect = R.random_map(4, H, W)
    n = 8
    pos = np.zeros((n, 3))
    pos[:, 0] = np.linspace(0, 0.1, n)
    track = PoseTrack(np.linspace(-1.0e6, 1.3e8, n), np.tile(np.eye(3), (n, 1, 1)), pos)
    intr = (20.0, 20.0, W / 2, H / 2)

    def make(stream, **kw):
        return EventSampler.from_stream(stream, centres, track, intr, 64, shrink_us=shrink, seed=1, **kw)

    s = _stream(c, H, W, rect)
    plain = make(s)
    viz = make(s, viz_dir=str(tmp_path / "a"))
    none = make(s, viz_dir=None)
    for a, b, d in zip(plain.tables, viz.tables, none.tables):
        for k in ("events", "num_at_xy", "first_at_xy", "no_successor", "num_successor", "pol_cumsum"):
            bits = (lambda v: v.view(torch.int32)) if k == "events" else (lambda v: v)          # (the map has NaNs)
            assert torch.equal(bits(a[k]), bits(b[k])) and torch.equal(bits(a[k]), bits(d[k]))
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{i:06d}{sfx}.png" for i in range(3) for sfx in ("", "_undist"))
    for i in range(3):
        first, last = s.window(centres[i] + shrink, centres[i + 1] - shrink)
        w = {k: v[first:last] for k, v in c.items()}
        for sfx, m in (("", None), ("_undist", rect)):
            got = np.asarray(Image.open(tmp_path / "a" / f"{i:06d}{sfx}.png").convert("RGB"))
            want = R.accumulation_image(w["x"], w["y"], w["p"], H, W, m)
            assert np.array_equal(got, want[..., ::-1])                    # cv2.imwrite reads the array as BGR
            assert (got[..., 0] == 0).any() and (got[..., 2] == 0).any()   # positive red, negative blue: both present
    # the reference's frame indices as names; without a map only the sensor picture
    make(_stream(c, H, W), viz_dir=str(tmp_path / "b"), viz_names=[4, 9, "000123"])
    assert sorted(os.listdir(tmp_path / "b")) == ["000004.png", "000009.png", "000123.png"]
    with pytest.raises(ValueError, match="viz_names"):
        make(s, viz_dir=str(tmp_path / "c"), viz_names=[1, 2])
