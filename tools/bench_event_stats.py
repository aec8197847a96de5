"""The loader's side of EventStream on one GPU (csrc/event_stats.hip) beside the straightforward torch
statement of each pass, on the same GPU and the same data: a 2 M-event window on 640 x 480 and on 1280 x 720, uniform
pixels plus 20 hot pixels holding 5 % of the events, a map that moves every pixel by a fraction of a cell.

  pass            native (the entry points, no read-back)              torch statement
  counts          enerf_event_pixel_stats, counts only                 bincount of 2 * (y * W + x) + (p > 0); and the same
                                                                       through index_put_(accumulate=True)
  counts + last   the same call with both last-event arrays            -- (no statement: the image's baseline stands for it)
  image           enerf_event_accumulation_image                       the window's x, y, p copied to the host and
                                                                       numpy's mask[y, x] = pol with the three colour
                                                                       assignments, as the reference runs it (wall clock)
  moments + mask  enerf_event_count_moments + enerf_event_hot_mask     c = counts.sum(-1), (c > 0).sum(), c.sum(),
                  (device time), and EventStream.hot_pixels with its   (c * c).sum(), read back, c > T, its two sums read
                  two read-backs (wall clock)                          back (wall clock)
  compaction      enerf_event_stream_compact (device time), and        keep = ~mask[y, x]; the four columns indexed by it
                  EventStream.without_pixels whole (wall clock)        (wall clock: the index reads its count back)

Every native result is asserted equal to its statement before anything is timed.  The variants of a pass take turns in
`--rounds` rounds of `--reps` repetitions after a warm-up; medians over the rounds, one JSON line per sensor, appended to
`--out`.  `bytes_per_event`: what a pass must move per event (stream columns read and written, the map's 8 bytes, 4 bytes
an atomic), `of_hbm`: that traffic over the device time as a fraction of HBM_TBS, the measured HBM rate DESIGN.md quotes.

    python tools/bench_event_stats.py [--reps 10] [--rounds 5] [--out profiles/event_stats_bench.jsonl]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from enerf_amd import _lib as L  # noqa: E402
from enerf_amd.event_dataset import EventStream  # noqa: E402

HBM_TBS = 6.29


def timed_once(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return a.elapsed_time(b) * 1e3 / reps, wall * 1e6 / reps             # microseconds per repetition


def timed_in_turn(variants, reps, rounds, warmup):
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    got = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            got[k].append(timed_once(fn, reps))
    return {k: {"device_us": round(statistics.median(d for d, _ in v), 1), "wall_us": round(statistics.median(w for _, w in v), 1),
                "device_us_rounds": [round(d, 1) for d, _ in v]} for k, v in got.items()}


def make_stream(H, W, E, dev):
    g = np.random.default_rng(H)
    x, y = g.integers(0, W, E), g.integers(0, H, E)
    at, which = g.random(E) < 0.05, g.integers(0, 20, E)
    hx, hy = g.integers(0, W, 20), g.integers(0, H, 20)
    x, y = np.where(at, hx[which], x).astype(np.uint16), np.where(at, hy[which], y).astype(np.uint16)
    t = np.sort(g.integers(1_000_000, 1_050_000, E)).astype(np.int64)
    p = g.choice(np.array([-1, 1], np.int8), E)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    rect = np.stack([xx + g.uniform(-0.7, 0.7, (H, W)), yy + g.uniform(-0.7, 0.7, (H, W))], -1).astype(np.float32)
    return EventStream(*(torch.from_numpy(v).to(dev) for v in (x, y, t, p)), H, W, rectify_map=rect), (x, y, p)


def host_image(x_dev, y_dev, p_dev, H, W):
    """The reference's procedure: the window on the host, numpy's assignment, the colours."""
    x, y, pol = x_dev.cpu().numpy(), y_dev.cpu().numpy(), p_dev.cpu().numpy().astype(np.int64)
    img = np.full((H, W, 3), 255, np.uint8)
    mask = np.zeros((H, W), np.int32)
    ok = (x >= 0) & (y >= 0) & (W > x) & (H > y)
    mask[y[ok].astype(np.int64), x[ok].astype(np.int64)] = pol[ok]
    img[mask == -1] = (255, 0, 0)
    img[mask == 1] = (0, 0, 255)
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--events", type=int, default=2_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "event_stats_bench.jsonl"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    lib = L.lib()
    E = a.events
    lines = [dict(what="device", name=torch.cuda.get_device_name(0), torch=torch.__version__, events=E, reps=a.reps,
                  rounds=a.rounds, hbm_tbs=HBM_TBS)]
    for H, W in ((480, 640), (720, 1280)):
        s, (xh, yh, ph) = make_stream(H, W, E, dev)
        HW = H * W
        counts = torch.empty(H, W, 2, dtype=torch.int32, device=dev)
        last_s = torch.empty(HW, dtype=torch.int32, device=dev)
        last_r = torch.empty(HW, dtype=torch.int32, device=dev)
        words = torch.zeros(8, dtype=torch.int64, device=dev)
        img = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
        hot = torch.empty(H, W, dtype=torch.uint8, device=dev)
        ptr = [v.data_ptr() for v in (s.x, s.y, s.t, s.p)]

        def stats(with_last):
            L.check(lib.enerf_event_pixel_stats(ptr[0], ptr[1], ptr[3], 0, E, H, W, s.rectify_map.data_ptr(), counts.data_ptr(),
                                                last_s.data_ptr() if with_last else None,
                                                last_r.data_ptr() if with_last else None, words[3:].data_ptr(),
                                                L.stream_handle()), "event_pixel_stats")

        def torch_index():
            return 2 * (s.y.to(torch.int64) * W + s.x.to(torch.int64)) + (s.p > 0)

        def torch_bincount():
            return torch.bincount(torch_index(), minlength=2 * HW).view(H, W, 2)

        def torch_index_put():
            out = torch.zeros(2 * HW, dtype=torch.int32, device=dev)
            return out.index_put_((torch_index(),), torch.ones((), dtype=torch.int32, device=dev), accumulate=True).view(H, W, 2)

        def image():
            L.check(lib.enerf_event_accumulation_image(last_s.data_ptr(), ptr[3], 0, E, H, W, img.data_ptr(),
                                                       L.stream_handle()), "event_accumulation_image")

        def moments_mask(T):
            L.check(lib.enerf_event_count_moments(counts.data_ptr(), H, W, words.data_ptr(), L.stream_handle()), "moments")
            L.check(lib.enerf_event_hot_mask(counts.data_ptr(), H, W, T, hot.data_ptr(), words[4:].data_ptr(),
                                             L.stream_handle()), "hot_mask")

        def torch_hot():
            c = counts.to(torch.int64).sum(-1)
            n, S, Q = torch.stack([(c > 0).sum(), c.sum(), (c * c).sum()]).tolist()
            mu = S / n
            T = int(mu + 5.0 * max(Q / n - mu * mu, 0.0) ** 0.5)
            m = c > T
            return m, torch.stack([m.sum(), c[m].sum()]).tolist()

        # ---- equal before anything is timed
        stats(True)
        assert int(words[3]) == 0
        ref = torch_bincount()
        assert torch.equal(counts, ref.to(torch.int32)) and torch.equal(counts, torch_index_put())
        image()
        assert np.array_equal(img.cpu().numpy(), host_image(s.x, s.y, s.p, H, W))
        mask = s.hot_pixels(n_sigma=5.0)
        report = dict(s.last_report)
        m, (n_hot, hot_events) = torch_hot()
        assert torch.equal(mask, m) and (n_hot, hot_events) == (report["hot"], report["hot_events"]) and n_hot > 0
        T = report["threshold"]
        moments_mask(T)
        assert torch.equal(hot.view(torch.bool), mask) and words[4:6].tolist() == [n_hot, hot_events]

        nbytes = ctypes.c_uint64(0)
        L.check(lib.enerf_event_stream_compact_workspace(E, ctypes.byref(nbytes)), "workspace")
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        outs = [torch.empty_like(v) for v in (s.x, s.y, s.t, s.p)]
        rep = torch.empty(2, dtype=torch.int32, device=dev)
        mask_u8 = mask.view(torch.uint8)

        def compact():
            L.check(lib.enerf_event_stream_compact(*ptr, E, H, W, mask_u8.data_ptr(), ws.data_ptr(),
                                                   *(v.data_ptr() for v in outs), rep.data_ptr(), L.stream_handle()), "compact")

        def torch_compact():
            keep = ~mask[s.y.to(torch.int64), s.x.to(torch.int64)]
            # (boolean indexing has no uint16 kernel: the two coordinate columns go through their int16 view)
            return [v.view(torch.int16)[keep].view(torch.uint16) if v.dtype == torch.uint16 else v[keep]
                    for v in (s.x, s.y, s.t, s.p)]

        compact()
        want = torch_compact()
        kept = int(rep[0])
        assert kept == want[0].numel() == E - hot_events and int(rep[1]) == 0
        for got, w in zip(outs, want):
            assert torch.equal(got[:kept].view(torch.int16) if got.dtype == torch.uint16 else got[:kept],
                               w.view(torch.int16) if w.dtype == torch.uint16 else w)
        whole = s.without_pixels(mask)
        assert len(whole) == kept and torch.equal(whole.t, want[2])

        res = {}
        res.update({"counts_" + k: v for k, v in timed_in_turn(
            {"native": lambda: stats(False), "native_with_last": lambda: stats(True), "torch_bincount": torch_bincount,
             "torch_index_put": torch_index_put}, a.reps, a.rounds, a.warmup).items()})
        stats(True)
        res.update({"image_" + k: v for k, v in timed_in_turn(
            {"native": image, "host_numpy": lambda: host_image(s.x, s.y, s.p, H, W)}, a.reps, a.rounds, a.warmup).items()})
        res.update({"hot_" + k: v for k, v in timed_in_turn(
            {"native_launches": lambda: moments_mask(T), "native_hot_pixels": lambda: s.hot_pixels(n_sigma=5.0),
             "torch": torch_hot}, a.reps, a.rounds, a.warmup).items()})
        res.update({"compact_" + k: v for k, v in timed_in_turn(
            {"native_launches": compact, "native_without_pixels": lambda: s.without_pixels(mask), "torch": torch_compact},
            a.reps, a.rounds, a.warmup).items()})
        f = kept / E
        bpe = {"counts_native": 5 + 4, "counts_native_with_last": 5 + 8 + 12, "compact_native_launches": 4 + 1 + 13 + 1 + 13 * f}
        traffic = {k: dict(bytes_per_event=round(b, 2),
                           of_hbm=round(b * E / (res[k]["device_us"] * 1e-6) / (HBM_TBS * 1e12), 4)) for k, b in bpe.items()}
        per_pixel = {"image_native": 4 + 3, "hot_native_launches": 8 + 8 + 1}
        traffic.update({k: dict(bytes_per_pixel=b, of_hbm=round(b * HW / (res[k]["device_us"] * 1e-6) / (HBM_TBS * 1e12), 4))
                        for k, b in per_pixel.items()})
        lines.append(dict(what="event_stats", H=H, W=W, events=E, hot_pixels=n_hot, hot_events=hot_events, kept=kept,
                          threshold=T, us=res, traffic=traffic))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
