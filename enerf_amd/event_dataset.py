"""From a raw event stream to EventSampler: the stage of EventNeRFDataset that feeds every event step.

The reference reads a window of the stream per frame, moves every event through the sensor's `rectify_map` to
fractional, undistorted coordinates (nerf/provider.py:148-328), groups the events by pixel with a Python dict keyed on
the float pair (provider.py:1152-1199) and, with `--negative_event_sampling`, lists per 20 ms chunk the pixels that did
not fire (provider.py:1283-1351).  Here that is one object:

  event_centres   the window borders of load_event_data_tumvie / load_event_data_EDS (provider.py:169-198, :268-283)
  EventStream     the stream on the device (x, y uint16, t int64, p int8) with its sensor and map;
                  .window     EventSlicer.get_events' index arithmetic (event_window.EventTimeIndex)
                  .tables / .no_event_tables / .batch_tables
                              the dicts of event_sampler.build_event_tables / build_no_event_tables, built by
                              csrc/event_tables.hip on device tensors and by the torch statements
                              below on CPU tensors
                  .pixel_counts / .accumulation_image / .hot_pixels / .without_pixels
                              per-pixel counts, render_ev_accumulation's pictures (utils/plot_utils.py), a hot-pixel mask
                              and the stream without it, by csrc/event_stats.hip
  EventSampler.from_stream   (event_sampler.py) every frame's tables from a stream, then the sampler

Pixels are keyed on the SENSOR pixel y * W + x, which is what the reference's float key amounts to for an injective map:
`build_event_tables` keys on the truncated coordinates and merges the sensor pixels that a compressing map truncates into
one cell.  Stated deviation: a map that sends two sensor pixels to the identical fp32 pair would be one dict key in the
reference and stays two pixels here.

Time: t_ns = (float64)(t + t_offset) * ns_per_unit with ns_per_unit = 1e6 / unit_per_ms (1000 for the h5 files'
microseconds); the offset is in stream units and added first, as EventSlicer.get_events does.  The event rows hold
(float32) t_ns; the stream is time-sorted and fp32 rounding is monotone, so stream order is the reference's stable sort on
the fp32 time, ties included.  Polarity is +1 where p > 0 and -1 otherwise (0/1 files and -1/+1 files alike).
"""
import ctypes
import math
import re

import numpy as np
import torch

from .event_sampler import build_event_tables, build_no_event_tables
from .event_window import EventTimeIndex


def _segment_tile():
    from . import _lib as L
    with open(L.HEADER_PATH) as f:
        m = re.search(r"^#define\s+ENERF_EVT_SEGMENT_TILE\s+(\d+)", f.read(), re.M)
    if not m:
        raise RuntimeError(f"enerf_amd: no ENERF_EVT_SEGMENT_TILE in {L.HEADER_PATH}")
    return int(m.group(1))


# events of one pixel that csrc/event_tables.hip orders in LDS (include/enerf_hip.h is the one place the number lives)
ENERF_EVT_SEGMENT_TILE = _segment_tile()


def event_centres(tss_imgs_us, idxs, mode):
    """The borders of the frames' event windows.  provider.py:169-198 (tumvie), :268-283 (eds).

    tss_imgs_us: every image time stamp of the sequence (the trigger period is their mean spacing); idxs: the frames
    used.  Frame i of sorted(idxs) takes the events of [centres[i] + shrink, centres[i + 1] - shrink): half way to its
    neighbours, and one trigger period beyond the first and the last frame.  `shrink_us` is tumvie's memory cap: when the
    windows together span more than 10 s, every window gives up the excess in equal parts at both ends; 0 for eds.
    -> (centres_us float64 [n + 1], shrink_us float)."""
    if mode not in ("tumvie", "eds"):
        raise ValueError(f"event_centres: mode {mode!r} (tumvie or eds; esim has no time stamps to centre)")
    tss = np.asarray(tss_imgs_us, dtype=np.float64).reshape(-1)
    idxss = sorted(int(i) for i in idxs)
    if tss.size < 2 or not idxss:
        raise ValueError("event_centres: two time stamps and one frame at least")
    dt_ms = np.diff(tss).mean() / 1e3
    hi = 100 if mode == "tumvie" else 50
    if not 3 < dt_ms < hi:
        raise ValueError(f"event_centres: a trigger period of {dt_ms} ms ({mode}: 3 .. {hi})")
    ts = tss[idxss]
    c = np.insert(ts, 0, ts[0] - 2 * dt_ms * 1e3)
    c = np.insert(c, len(c), c[-1] + 2 * dt_ms * 1e3)
    c = c[:-1] + np.diff(c) / 2.
    if not np.all(np.diff(c) > 0):
        raise ValueError("event_centres: the frames' time stamps must increase")
    shrink = 0.0
    if mode == "tumvie":
        span, cap = c[-1] - c[0], 10 * 1e6
        if span > cap:
            shrink = float((span - cap) / (2 * len(idxss)))
    return c, shrink


def tables_statement(x, y, t, p, first, last, H, W, rectify_map=None, ns_per_unit=1000.0, t_offset=0):
    """The event tables of the window [first, last) as a torch statement, wherever the stream lives: build_event_tables
    on the SENSOR coordinates (integers: its pixel key is exact), then the kept events' coordinates through the map.
    -> (the dict of build_event_tables, bad) with bad = events outside the sensor (they are left out)."""
    xs = x[first:last].to(torch.int64)
    ys = y[first:last].to(torch.int64)
    ok = (xs < W) & (ys < H) & (xs >= 0) & (ys >= 0)
    bad = int((~ok).sum())
    t_ns = ((t[first:last].to(torch.int64) + int(t_offset)).to(torch.float64) * float(ns_per_unit)).to(torch.float32)
    pol = torch.where(p[first:last] > 0, 1.0, -1.0).to(torch.float32)
    ev = torch.stack([xs.to(torch.float32), ys.to(torch.float32), t_ns, pol], dim=1)[ok]
    tab = build_event_tables(ev)
    if rectify_map is not None:
        rm = torch.as_tensor(np.asarray(rectify_map) if not torch.is_tensor(rectify_map) else rectify_map)
        rm = rm.to(ev.device, torch.float32)
        rows = tab["events"].clone()
        rows[:, 0:2] = rm[rows[:, 1].to(torch.int64), rows[:, 0].to(torch.int64)]
        tab["events"] = rows
    return tab, bad


def chunk_edges(start_us, end_us, chunk_len_ms=20.0):
    """provider.py:1305-1313, :1348: the batch's span cut into int(duration_ms / chunk_len_ms) + 1 equal chunks, the edges
    accumulated in float64 as the reference does (`ts_iter += dt_us`).  -> (edges [n + 1] list, dt_us)."""
    if not end_us > start_us:
        raise ValueError("no-event tables: the batch must span a positive time")
    dur_ms = end_us / 1e3 - start_us / 1e3
    n_chunks = int(dur_ms / chunk_len_ms) + 1
    dt_us = 1e3 * dur_ms / n_chunks
    edges = [float(start_us)]
    for _ in range(n_chunks):
        edges.append(edges[-1] + dt_us)
    return edges, dt_us


_MAX_EVENTS = 1 << 30      # events of one call (kMaxEvents of csrc/event_tables.hip and csrc/event_stats.hip)


def _hot_threshold(n, S, Q, n_sigma, max_count):
    """EventStream.hot_pixels' integer threshold from the counts' exact moments, in Python floats."""
    if max_count is not None:
        return int(max_count)
    mu = S / n
    sigma = math.sqrt(max(Q / n - mu * mu, 0.0))
    return int(math.floor(mu + float(n_sigma) * sigma))


class EventStream:
    """A raw event stream with its sensor: x, y (sensor pixel), t (ascending, `unit_per_ms` units per millisecond), p
    (polarity), all [E] on one device; the sensor's H, W; `rectify_map` [H, W, 2] (x', y') or None for the identity
    (esim).  `t_offset` (stream units) and `ms_to_idx` are the h5 files' (EventSlicer).  Held as uint16 / uint16 / int64 /
    int8 (13 bytes an event) next to a float32 copy of the map.

    On device tensors .tables / .no_event_tables / .batch_tables run csrc/event_tables.hip (there is no fallback: a
    missing library raises); on CPU tensors they run tables_statement and build_no_event_tables on the sensor
    coordinates.  After each of them `last_report` holds {"N", "P", "bad"} of the window.

    The loader's side works the same way (csrc/event_stats.hip on device tensors, torch statements on CPU tensors, DESIGN.md
    4.22): .pixel_counts, .accumulation_image (the reference's loaded_events_undist_viz pictures), .hot_pixels and
    .without_pixels; each fills `last_report` as its docstring says."""

    def __init__(self, x, y, t, p, H, W, rectify_map=None, unit_per_ms=1000, t_offset=0, ms_to_idx=None):
        t = torch.as_tensor(t)
        dev = t.device
        if t.ndim != 1 or t.numel() == 0:
            raise ValueError("EventStream: t must be a non-empty 1-D tensor")
        self.H, self.W = int(H), int(W)
        if not (0 < self.H <= 65536 and 0 < self.W <= 65536):
            raise ValueError(f"EventStream: a {self.W} x {self.H} sensor")

        def coord(v, name):
            v = torch.as_tensor(v).to(dev)
            if v.shape != t.shape:
                raise ValueError(f"EventStream: {name} has shape {tuple(v.shape)}, t {tuple(t.shape)}")
            if v.dtype != torch.uint16:
                wide = v.to(torch.int64)
                if int(wide.min()) < 0 or int(wide.max()) > 65535:
                    raise ValueError(f"EventStream: {name} outside 0 .. 65535")
                v = wide.to(torch.uint16)
            return v.contiguous()

        self.x, self.y = coord(x, "x"), coord(y, "y")
        self.t = t.to(torch.int64).contiguous()
        p = torch.as_tensor(p).to(dev)
        if p.shape != t.shape:
            raise ValueError(f"EventStream: p has shape {tuple(p.shape)}, t {tuple(t.shape)}")
        self.p = torch.where(p > 0, 1, -1).to(torch.int8).contiguous()
        self.device = dev
        self.rectify_map = None
        if rectify_map is not None:
            rm = rectify_map if torch.is_tensor(rectify_map) else torch.as_tensor(np.asarray(rectify_map))
            if tuple(rm.shape) != (self.H, self.W, 2):
                raise ValueError(f"EventStream: rectify_map {tuple(rm.shape)}, ({self.H}, {self.W}, 2) expected")
            self.rectify_map = rm.to(dev, torch.float32).contiguous()
        self.unit_per_ms = unit_per_ms
        self.ns_per_unit = 1e6 / float(unit_per_ms)
        self.t_offset = int(t_offset)
        self.index = EventTimeIndex(self.t, unit_per_ms, t_offset, ms_to_idx)
        self.last_report = None

    def __len__(self):
        return self.t.numel()

    def window(self, t0_us, t1_us):
        """(first, one past last) of the events with t0_us <= t < t1_us (offset included), None when the millisecond
        index does not cover the window: EventTimeIndex.window in the stream's unit.  The borders are rounded up first:
        the time stamps are integers, so t >= 1000.5 is t >= 1001, which is how EventSlicer's comparison of an integer
        stamp with a fractional border (the centres are midpoints) comes out; the index itself would truncate them."""
        k = self.unit_per_ms / 1000
        return self.index.window(math.ceil(t0_us * k), math.ceil(t1_us * k))

    # ---- the three requests -------------------------------------------------------------------------------------------
    def tables(self, first, last):
        """The dict of build_event_tables for the window [first, last), "_packed" already in the kernels' layout."""
        return self._build(first, last, True, None)[0]

    def no_event_tables(self, first, last, start_us, end_us, chunk_len_ms=20.0, generator=None, keep=None):
        """The dict of build_no_event_tables for the events of [first, last) and the span [start_us, end_us)."""
        return self._build(first, last, False, (start_us, end_us, chunk_len_ms, generator, keep))[1]

    def batch_tables(self, first, last, start_us, end_us, chunk_len_ms=20.0, generator=None, keep=None):
        """(tables, no_event_tables) from ONE pass over the window: the chunks' hit bitmaps ride in the count pass."""
        return self._build(first, last, True, (start_us, end_us, chunk_len_ms, generator, keep))

    # ---- the loader's side: counts, pictures, hot pixels ---------------------------------------------
    def pixel_counts(self, first, last):
        """int32 [H, W, 2]: the events of the window [first, last) per sensor pixel, [..., 0] those of polarity -1,
        [..., 1] those of polarity +1.  last_report = {"events", "bad"}."""
        first, last = self._span(first, last)
        counts = self._stats(first, last, False, False)[0]
        self.last_report = {"events": last - first, "bad": 0}
        return counts

    def accumulation_image(self, first, last, rectified=False):
        """uint8 [H, W, 3]: what utils/plot_utils.py render_ev_accumulation returns for the window (provider.py:227-230,
        :313-316).  White; then, in stream order, every event paints its cell with its polarity, a later event over an
        earlier one: -1 (255, 0, 0), +1 (0, 0, 255).  The cell is the sensor pixel (y, x) or, `rectified`,
        (int(yr), int(xr)) of (xr, yr) = rectify_map[y, x] for the events with xr >= 0, yr >= 0, xr < W, yr < H in
        float32 (a NaN fails).  last_report = {"events", "bad"}."""
        first, last = self._span(first, last)
        if rectified and self.rectify_map is None:
            raise ValueError("EventStream.accumulation_image: rectified=True needs a rectify_map")
        _, last_event = self._stats(first, last, not rectified, bool(rectified))
        if self.device.type == "cuda":
            from . import _lib as L
            img = torch.empty(self.H, self.W, 3, dtype=torch.uint8, device=self.device)
            with torch.cuda.device(self.device):
                L.check(L.lib().enerf_event_accumulation_image(last_event.data_ptr(), self.p.data_ptr(), first, last, self.H,
                                                               self.W, img.data_ptr(), L.stream_handle()),
                        "event_accumulation_image")
        else:
            pol = self.p[first:last][(last_event - 1).clamp(min=0)]
            img = torch.full((self.H * self.W, 3), 255, dtype=torch.uint8)
            img[(last_event > 0) & (pol < 0)] = torch.tensor([255, 0, 0], dtype=torch.uint8)
            img[(last_event > 0) & (pol > 0)] = torch.tensor([0, 0, 255], dtype=torch.uint8)
            img = img.view(self.H, self.W, 3)
        self.last_report = {"events": last - first, "bad": 0}
        return img

    def hot_pixels(self, first=0, last=None, *, n_sigma=None, max_count=None):
        """bool [H, W]: the sensor pixels with more events in the window than a threshold T.  c = events per pixel (both
        polarities); over the n pixels with c > 0, S = sum c and Q = sum c * c (exact integers).  `max_count`: T =
        max_count.  `n_sigma`: T = floor(mu + n_sigma * sigma) with mu = S / n, sigma = sqrt(max(Q / n - mu * mu, 0)), in
        Python floats on the host -- an integer from exact integers, so both routes give the same mask.  Exactly one of
        the two; there is no default (the reference defines no filter).
        last_report = {"active": n, "events": S, "threshold": T, "hot", "hot_events"}."""
        if (n_sigma is None) == (max_count is None):
            raise ValueError("EventStream.hot_pixels: exactly one of n_sigma and max_count")
        if n_sigma is not None and not (math.isfinite(float(n_sigma)) and float(n_sigma) >= 0.0):
            raise ValueError(f"EventStream.hot_pixels: n_sigma = {n_sigma} (finite, >= 0)")
        if max_count is not None and (int(max_count) != max_count or int(max_count) < 0):
            raise ValueError(f"EventStream.hot_pixels: max_count = {max_count} (an integer >= 0)")
        first, last = self._span(first, len(self) if last is None else last)
        H, W, dev = self.H, self.W, self.device
        if dev.type == "cuda":
            from . import _lib as L
            lib = L.lib()
            with torch.cuda.device(dev):
                words = torch.empty(6, dtype=torch.int64, device=dev)          # n, S, Q, bad | hot, hot_events
                counts = self._stats_launch(first, last, False, False, words[3:4])[0]
                stream = L.stream_handle()
                L.check(lib.enerf_event_count_moments(counts.data_ptr(), H, W, words.data_ptr(), stream),
                        "event_count_moments")
                n, S, Q, bad = (int(v) for v in words[:4].tolist())            # the read-back before the mask
                self._sensor(bad)
                T = _hot_threshold(n, S, Q, n_sigma, max_count)
                mask = torch.empty(H, W, dtype=torch.uint8, device=dev)
                L.check(lib.enerf_event_hot_mask(counts.data_ptr(), H, W, min(T, 1 << 62), mask.data_ptr(),
                                                 words[4:].data_ptr(), stream), "event_hot_mask")
                hot, hot_events = (int(v) for v in words[4:].tolist())         # ... and the one after
            mask = mask.view(torch.bool)
        else:
            c = self._stats(first, last, False, False)[0].to(torch.int64).sum(-1)
            n, S, Q = int((c > 0).sum()), int(c.sum()), int((c * c).sum())
            T = _hot_threshold(n, S, Q, n_sigma, max_count)
            mask = c > min(T, 1 << 62)
            hot, hot_events = int(mask.sum()), int(c[mask].sum())
        self.last_report = {"active": n, "events": S, "threshold": T, "hot": hot, "hot_events": hot_events}
        return mask

    def without_pixels(self, mask):
        """A new EventStream without the events at the sensor pixels where `mask` (bool [H, W], on the stream's device) is
        set; the others keep their order.  H, W, the map, unit_per_ms and t_offset are carried over; the millisecond index
        is rebuilt.  A mask that leaves no event raises (a stream is never empty).  On the source stream last_report =
        {"kept", "removed"}."""
        if not torch.is_tensor(mask) or mask.dtype != torch.bool or tuple(mask.shape) != (self.H, self.W):
            raise ValueError(f"EventStream.without_pixels: the mask must be a bool tensor of shape ({self.H}, {self.W})")
        if mask.device != self.x.device:
            raise ValueError(f"EventStream.without_pixels: the mask is on {mask.device}, the stream on {self.x.device}")
        E = len(self)
        if E > _MAX_EVENTS:
            raise ValueError(f"EventStream.without_pixels: {E} events (at most 2^30 in one call)")
        mask = mask.contiguous()
        if self.device.type == "cuda":
            from . import _lib as L
            lib, dev = L.lib(), self.device
            with torch.cuda.device(dev):
                nbytes = ctypes.c_uint64(0)
                L.check(lib.enerf_event_stream_compact_workspace(E, ctypes.byref(nbytes)), "event_stream_compact_workspace")
                ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
                out = [torch.empty_like(v) for v in (self.x, self.y, self.t, self.p)]
                report = torch.empty(2, dtype=torch.int32, device=dev)
                L.check(lib.enerf_event_stream_compact(
                    self.x.data_ptr(), self.y.data_ptr(), self.t.data_ptr(), self.p.data_ptr(), E, self.H, self.W,
                    mask.view(torch.uint8).data_ptr(), ws.data_ptr(), *(v.data_ptr() for v in out), report.data_ptr(),
                    L.stream_handle()), "event_stream_compact")
                kept, bad = report.tolist()                                    # the one read-back: sizes the result
            self._sensor(bad)
            cols = [v[:kept].clone() for v in out] if 0 < kept < E else out
        else:
            xs, ys = self.x.to(torch.int64), self.y.to(torch.int64)
            self._sensor(int(((xs >= self.W) | (ys >= self.H)).sum()))
            keep = ~mask[ys, xs]
            kept = int(keep.sum())
            cols = [v[keep] for v in (self.x, self.y, self.t, self.p)]
        self.last_report = {"kept": kept, "removed": E - kept}
        if kept == 0:
            raise ValueError("EventStream.without_pixels: the mask removes every event")
        return EventStream(*cols, self.H, self.W, self.rectify_map, self.unit_per_ms, self.t_offset, None)

    def _span(self, first, last):
        first, last = int(first), int(last)
        if not 0 <= first <= last <= len(self):
            raise ValueError(f"EventStream: window [{first}, {last}) of a stream of {len(self)} events")
        if first == last:
            raise ValueError("EventStream: an empty window")
        if last - first > _MAX_EVENTS:
            raise ValueError(f"EventStream: a window of {last - first} events (at most 2^30 in one call)")
        return first, last

    def _sensor(self, bad):
        if bad > 0:
            self.last_report = {"bad": bad}
            raise ValueError(f"EventStream: {bad} event(s) outside the {self.W} x {self.H} sensor")

    def _stats_launch(self, first, last, want_sensor, want_rect, bad):
        """enerf_event_pixel_stats on the window -> (counts [H, W, 2] int32, the last-event array asked for, int32 [H * W]
        with 0 for no event, or None); `bad`: one int64 word on the device that takes the out-of-sensor count."""
        from . import _lib as L
        H, W, dev = self.H, self.W, self.device
        counts = torch.empty(H, W, 2, dtype=torch.int32, device=dev)
        last_event = torch.empty(H * W, dtype=torch.int32, device=dev) if want_sensor or want_rect else None
        L.check(L.lib().enerf_event_pixel_stats(
            self.x.data_ptr(), self.y.data_ptr(), self.p.data_ptr(), first, last, H, W,
            self.rectify_map.data_ptr() if want_rect else None, counts.data_ptr(),
            last_event.data_ptr() if want_sensor else None, last_event.data_ptr() if want_rect else None, bad.data_ptr(),
            L.stream_handle()), "event_pixel_stats")
        return counts, last_event

    def _stats(self, first, last, want_sensor, want_rect):
        """(counts, last-event array) of the window on either route, the sensor check made (one read-back on the device)."""
        H, W = self.H, self.W
        if self.device.type == "cuda":
            with torch.cuda.device(self.device):
                bad = torch.empty(1, dtype=torch.int64, device=self.device)
                out = self._stats_launch(first, last, want_sensor, want_rect, bad)
                self._sensor(int(bad))
            return out
        xs, ys = self.x[first:last].to(torch.int64), self.y[first:last].to(torch.int64)
        self._sensor(int(((xs >= W) | (ys >= H)).sum()))
        pix = ys * W + xs
        counts = torch.bincount(2 * pix + (self.p[first:last] > 0), minlength=2 * H * W).view(H, W, 2).to(torch.int32)
        last_event = None
        if want_sensor or want_rect:
            number = torch.arange(1, last - first + 1, dtype=torch.int64)
            cell = pix
            if want_rect:
                r = self.rectify_map[ys, xs]
                xr, yr = r[:, 0], r[:, 1]
                ok = (xr >= 0) & (yr >= 0) & (xr < W) & (yr < H)
                cell = yr[ok].to(torch.int64) * W + xr[ok].to(torch.int64)
                number = number[ok]
            last_event = torch.zeros(H * W, dtype=torch.int64).scatter_reduce(0, cell, number, "amax")
        return counts, last_event

    # ---- both routes --------------------------------------------------------------------------------------------------
    def _build(self, first, last, want_tables, no_ev):
        first, last = int(first), int(last)
        if not 0 <= first <= last <= len(self):
            raise ValueError(f"EventStream: window [{first}, {last}) of a stream of {len(self)} events")
        if first == last:
            raise ValueError("EventStream: an empty window")
        route = self._native if self.device.type == "cuda" else self._statement
        tab, nev, report = route(first, last, want_tables, no_ev)
        self.last_report = report
        return tab, nev

    def _check(self, report, want_tables):
        self.last_report = report
        if report["bad"] > 0:
            raise ValueError(f"EventStream: {report['bad']} event(s) outside the {self.W} x {self.H} sensor")
        if want_tables and (report["P"] < 1 or report["N"] < 2):
            raise ValueError("EventStream: the window has no pixel with two events")

    def _statement(self, first, last, want_tables, no_ev):
        xs, ys = self.x[first:last].to(torch.int64), self.y[first:last].to(torch.int64)
        bad = int(((xs >= self.W) | (ys >= self.H)).sum())
        report = {"N": 0, "P": 0, "bad": bad}
        self._check(report, False)
        tab = nev = None
        if want_tables:
            pix = ys * self.W + xs
            if int(torch.bincount(pix, minlength=1).max()) < 2:
                self._check(report, True)
            tab, _ = tables_statement(self.x, self.y, self.t, self.p, first, last, self.H, self.W, self.rectify_map,
                                      self.ns_per_unit, self.t_offset)
            report.update(N=tab["events"].shape[0], P=tab["num_at_xy"].shape[0])
            tab["_packed"] = (tab["events"].contiguous(), tab["no_successor"].to(torch.uint8), tab["num_successor"],
                              tab["pol_cumsum"], tab["num_at_xy"], tab["first_at_xy"])
        if no_ev is not None:
            start_us, end_us, chunk_len_ms, generator, keep = no_ev
            t_ns = (self.t[first:last] + self.t_offset).to(torch.float64) * self.ns_per_unit
            ev = torch.stack([xs.to(torch.float64), ys.to(torch.float64), t_ns], dim=1)
            nev = build_no_event_tables(ev, self.H, self.W, start_us, end_us, chunk_len_ms, self.rectify_map, generator, keep)
        return tab, nev, report

    def _native(self, first, last, want_tables, no_ev):
        from . import _lib as L
        lib, dev, H, W = L.lib(), self.device, self.H, self.W
        n_chunks, edges_dev, cand = 0, None, None
        if no_ev is not None:
            start_us, end_us, chunk_len_ms, generator, keep = no_ev
            edges, dt_us = chunk_edges(start_us, end_us, chunk_len_ms)
            n_chunks = len(edges) - 1
            edges_dev = torch.tensor(edges, dtype=torch.float64, device=dev)
            cand = torch.empty(n_chunks, H * W, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            nbytes = ctypes.c_uint64(0)
            L.check(lib.enerf_event_tables_workspace(last - first, H, W, n_chunks, ctypes.byref(nbytes)),
                    "event_tables_workspace")
            ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
            report_dev = torch.empty(4 + n_chunks, dtype=torch.int64, device=dev)
            stream = L.stream_handle()
            L.check(lib.enerf_event_tables_count(
                self.x.data_ptr(), self.y.data_ptr(), self.t.data_ptr(), first, last, H, W, self.ns_per_unit, self.t_offset,
                int(want_tables), edges_dev.data_ptr() if n_chunks else None, n_chunks, ws.data_ptr(), report_dev.data_ptr(),
                cand.data_ptr() if n_chunks else None, stream), "event_tables_count")
            rep = report_dev.tolist()                                      # the one read-back of the batch
            N, P = int(rep[0]), int(rep[1])
            report = {"N": N, "P": P, "bad": int(rep[2])}
            self._check(report, want_tables)
            tab = nev = None
            if want_tables:
                events = torch.empty(N, 4, dtype=torch.float32, device=dev)
                nos = torch.empty(N, dtype=torch.uint8, device=dev)
                nsucc = torch.empty(N, dtype=torch.int64, device=dev)
                cs = torch.empty(N + 1, dtype=torch.float64, device=dev)
                num = torch.empty(P, dtype=torch.int64, device=dev)
                fst = torch.empty(P, dtype=torch.int64, device=dev)
                rect = self.rectify_map.data_ptr() if self.rectify_map is not None else None
                L.check(lib.enerf_event_tables_fill(
                    self.x.data_ptr(), self.y.data_ptr(), self.t.data_ptr(), self.p.data_ptr(), first, last, H, W, rect,
                    self.ns_per_unit, self.t_offset, ws.data_ptr(), n_chunks, N, P, events.data_ptr(), nos.data_ptr(),
                    nsucc.data_ptr(), cs.data_ptr(), num.data_ptr(), fst.data_ptr(), stream), "event_tables_fill")
                tab = {"events": events, "num_at_xy": num, "first_at_xy": fst, "no_successor": nos.view(torch.bool),
                       "num_successor": nsucc, "pol_cumsum": cs, "_packed": (events, nos, nsucc, cs, num, fst)}
            if n_chunks:
                nev = {"coords": [], "start_time_us": [], "end_time_us": [], "N_ev_chunks": n_chunks, "dt_us": dt_us}
                rect = self.rectify_map.data_ptr() if self.rectify_map is not None else None
                bad_index = torch.zeros(1, dtype=torch.int32, device=dev)
                for j in range(n_chunks):
                    c = cand[j, :int(rep[4 + j])]
                    n_keep = int(c.numel() / n_chunks)
                    if keep is not None:
                        sel = torch.as_tensor(keep(j, c), device=dev, dtype=torch.int64).contiguous()
                    else:
                        sel = c[torch.randperm(c.numel(), device=dev, generator=generator)[:n_keep]]
                    n_sel = sel.numel()
                    xy = torch.empty(max(n_sel, 1), 2, dtype=torch.float32, device=dev)
                    L.check(lib.enerf_no_event_coords(sel.data_ptr() if n_sel else None, n_sel, rect, H, W, xy.data_ptr(),
                                                      bad_index.data_ptr(), stream), "no_event_coords")
                    nev["coords"].append(xy)
                    nev["start_time_us"].append(edges[j])
                    nev["end_time_us"].append(edges[j] + dt_us)
                if keep is not None and int(bad_index) > 0:
                    raise ValueError(f"EventStream: keep() chose {int(bad_index)} pixel(s) outside the sensor")
        return tab, nev, report
