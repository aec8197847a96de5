"""One event batch's tables on one GPU: EventStream.batch_tables (csrc/event_tables.hip) beside the torch
route it stands next to, build_event_tables followed by build_no_event_tables, on the same GPU and the same data.  Integer
(esim-like) coordinates and the identity map, where both routes are right and give the same tables (asserted before
anything is timed).  2 M events in a 50 ms window (three chunks), on 640 x 480 and on 1280 x 720.

  native     EventStream.batch_tables: count pass (with the chunks' bitmaps), rank and offset scans, one read-back,
             placement, segment sort, the finishing scan; per chunk one randperm and one gather launch
  torch      build_event_tables (three argsorts, unique, scatter_reduce, repeat_interleave, cumsum) +
             build_no_event_tables (per chunk: mask, scatter, nonzero, randperm, gather)

Both routes read counts back, so a repetition is timed as a whole: the wall clock around it with the device drained at
its end, and the device's own time between two events around it.  The routes take turns in `--rounds` rounds of `--reps`
repetitions after a warm-up; the medians over the rounds are reported, one JSON line per sensor, appended to `--out`.

    python tools/bench_event_tables.py [--reps 10] [--rounds 5] [--out profiles/event_tables_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from enerf_amd import event_sampler as E  # noqa: E402
from enerf_amd.event_dataset import EventStream  # noqa: E402

T0_US, SPAN_US = 1_000_000, 50_000


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
    return a.elapsed_time(b) / reps, wall * 1e3 / reps                  # milliseconds per repetition


def timed_in_turn(variants, reps, rounds, warmup):
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    got = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            got[k].append(timed_once(fn, reps))
    return {k: (statistics.median(d for d, _ in v), statistics.median(w for _, w in v), [round(w, 3) for _, w in v])
            for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--events", type=int, default=2_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "event_tables_bench.jsonl"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    lines = [dict(what="device", name=torch.cuda.get_device_name(0), torch=torch.__version__, events=a.events,
                  window_ms=SPAN_US / 1e3, reps=a.reps, rounds=a.rounds)]
    for H, W in ((480, 640), (720, 1280)):
        rng = np.random.default_rng(H)
        x = torch.from_numpy(rng.integers(0, W, a.events).astype(np.uint16)).to(dev)
        y = torch.from_numpy(rng.integers(0, H, a.events).astype(np.uint16)).to(dev)
        t = torch.from_numpy(np.sort(rng.integers(T0_US, T0_US + SPAN_US, a.events)).astype(np.int64)).to(dev)
        p = torch.from_numpy(rng.choice(np.array([-1, 1], np.int8), a.events)).to(dev)
        stream = EventStream(x, y, t, p, H, W)
        ev = torch.stack([x.double(), y.double(), t.double() * 1000.0, p.double()], 1)      # what the loaders hand over
        t0, t1 = float(T0_US), float(T0_US + SPAN_US)
        gen = torch.Generator(device=dev).manual_seed(0)

        def native():
            return stream.batch_tables(0, a.events, t0, t1, generator=gen)

        def torch_route():
            return E.build_event_tables(ev.float()), E.build_no_event_tables(ev, H, W, t0, t1, generator=gen)

        (tn, nn), (tt, nt) = native(), torch_route()
        for k in ("events", "num_at_xy", "first_at_xy", "no_successor", "num_successor", "pol_cumsum"):
            assert torch.equal(tn[k], tt[k]), k
        assert nn["N_ev_chunks"] == nt["N_ev_chunks"] == 3
        assert [c.shape for c in nn["coords"]] == [c.shape for c in nt["coords"]]
        res = timed_in_turn({"native": native, "torch": torch_route}, a.reps, a.rounds, a.warmup)
        lines.append(dict(what="event_tables", H=H, W=W, events=a.events, N=tn["events"].shape[0],
                          P=tn["num_at_xy"].shape[0], chunks=3,
                          **{f"{k}_{unit}_ms": round(v[i], 3) for k, v in res.items() for i, unit in enumerate(("device", "wall"))},
                          wall_ms_rounds={k: v[2] for k, v in res.items()},
                          speedup_wall=round(res["torch"][1] / res["native"][1], 2)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
