"""One event batch of the setting the shipped configs train with (accumulate_evs = 0) on one GPU: EventSampler.batch
(csrc/event_pairs.hip: k_event_single_pair_rays, k_no_event_rays) beside the torch statement of the reference's collate on
the same GPU.  Sensor 640 x 480, a 2 M-event batch of 100 ms, a 500-knot pose track; M = 20096 and 30096 pairs (the
shipped batch_size_evs), with and without the M / 2 no-event rays of --negative_event_sampling.

  sampler           EventSampler.batch: the draws (rand(P), randperm(P)[:M]; randint + rand for the no-event pixels) and one
                    launch for the pairs, one for the no-event rays
  kernel            each launch alone, from given draws (what the sampler adds to the draws)
  draw              torch.randperm(P)[:M] alone: the without-replacement draw the sampler still leaves to torch
  statement_poses   sample_event_pairs(accumulate=False) + event_pair_batch's gather from a pre-interpolated pose per event
                    (`poses_evs` [N, 3, 4] fp32: the reference's "fast, but large memory requirement") + get_event_rays
  statement_track   the same pairs with PoseTrack.poses_at at the 2 M gathered times instead of the per-event array
                    (with the no-event rays both statements add event_sampler.no_event_rays, CPU generator as usual)

Every variant is timed in `--rounds` rounds that take the variants in turn (`--reps` repetitions each after a warm-up):
device time between two events around the repetitions, and the host's enqueue time (the clock around the same loop before
the device is waited for); the medians over the rounds are reported, one JSON line per case.

    python tools/bench_event_batch.py [--reps 100] [--rounds 5]
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
from enerf_amd import event_sampler as E, scene  # noqa: E402
from enerf_amd.events import get_event_rays  # noqa: E402
from enerf_amd.pose_interp import PoseTrack  # noqa: E402

H, W = scene.H, scene.W
T0_NS, SPAN_NS = 1.0e9, 1.0e8


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed_once(fn, reps, cuda):
    if not cuda:
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        us = (time.perf_counter() - t0) * 1e6 / reps
        return us, us
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps, host * 1e6 / reps          # microseconds per repetition


def timed_in_turn(variants, reps, rounds, cuda):
    """{name: fn} -> {name: (median device us, median host us, [device us per round])}"""
    for fn in variants.values():
        for _ in range(10):
            fn()
    got = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            got[k].append(timed_once(fn, reps, cuda))
    return {k: (statistics.median(d for d, _ in v), statistics.median(h for _, h in v), [round(d, 2) for d, _ in v])
            for k, v in got.items()}


def make_case(n_events, knots, dev, seed=0):
    rng = np.random.default_rng(seed)
    ev = np.stack([rng.integers(0, W, n_events), rng.integers(0, H, n_events),
                   np.sort(rng.uniform(T0_NS, T0_NS + SPAN_NS, n_events)), rng.choice([-1.0, 1.0], n_events)], 1)
    ev = torch.from_numpy(ev).to(dev)
    t = np.linspace(T0_NS - 1e6, T0_NS + SPAN_NS + 1e6, knots)
    poses = np.stack([scene.pose(32.0 * k / (8 * knots)).numpy() for k in range(knots)])   # an eighth of the circle
    track = PoseTrack(t, poses[:, :3, :3], poses[:, :3, 3], device=dev)
    tables = E.build_event_tables(ev.float())
    no_evs = E.build_no_event_tables(ev, H, W, T0_NS * 1e-3, (T0_NS + SPAN_NS) * 1e-3,
                                     generator=torch.Generator(device=dev).manual_seed(seed))
    return tables, no_evs, track


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--events", type=int, default=2_000_000)
    ap.add_argument("--knots", type=int, default=500)
    ap.add_argument("--device", default="cuda", help="cpu: a rehearsal of the script (the statements only, no kernel)")
    a = ap.parse_args()
    dev = torch.device(a.device)
    cuda = dev.type == "cuda"
    if cuda:
        torch.cuda.set_device(0)
    emit(what="device", name=torch.cuda.get_device_name(0) if cuda else "cpu (rehearsal: not a measurement)",
         torch=torch.__version__, H=H, W=W, events=a.events, knots=a.knots, reps=a.reps, rounds=a.rounds)
    tables, no_evs, track = make_case(a.events, a.knots, dev)
    N, P = tables["events"].shape[0], tables["num_at_xy"].shape[0]
    poses_evs = track.poses_at(tables["events"][:, 2])                 # what the reference pre-interpolates, per event
    emit(what="case", N=N, P=P, chunks=no_evs["N_ev_chunks"], poses_evs_bytes=poses_evs.numel() * poses_evs.element_size(),
         table_bytes=sum(t.numel() * t.element_size() for t in E._packed(tables)),
         track_bytes=sum(getattr(track, n).numel() * 8 for n in ("knots", "rot", "rotvec", "tcoef")))
    gen = torch.Generator(device=dev).manual_seed(1)
    host_gen = torch.Generator().manual_seed(1)
    intr = scene.INTRINSICS
    tns = tables["events"][:, 2]
    for M in (20096, 30096):
        for with_no_evs in (False, True):
            sampler = E.EventSampler([tables], track, intr, M, no_events=[no_evs] if with_no_evs else None, seed=2)

            def statement_pairs(poses_of):
                s, e, pols, xs, ys = E.sample_event_pairs(tables, M, False, generator=gen)
                r = get_event_rays(xs, ys, poses_of(s).unsqueeze(0), poses_of(e).unsqueeze(0), intr)
                r["pols"] = pols
                if with_no_evs:
                    r.update(E.no_event_rays(no_evs, track, intr, M, generator=host_gen))
                return r

            variants = {"sampler": lambda: sampler.batch([0]),
                        "statement_poses": lambda: statement_pairs(lambda i: poses_evs[i]),
                        "statement_track": lambda: statement_pairs(lambda i: track.poses_at(tns[i])),
                        "draw": lambda: torch.randperm(P, device=dev, generator=gen)[:M]}
            if cuda:
                draws = {"u_xy": torch.rand(P, device=dev, generator=gen, dtype=torch.float64),
                         "choice": torch.randperm(P, device=dev, generator=gen)[:M].contiguous()}
                variants["kernel_pairs"] = lambda: E.event_single_pair_rays(tables, track, intr, M, draws=draws)
                if with_no_evs:
                    n_j = no_evs["coords"][0].shape[0]
                    nd = {"chunk": 0, "idx": torch.randint(0, n_j, (M // 2,), device=dev, generator=gen),
                          "u": torch.rand(M // 2, 2, device=dev, generator=gen, dtype=torch.float64)}
                    variants["kernel_no_events"] = lambda: E.no_event_pair_rays(no_evs, track, intr, M, draws=nd)
            res = timed_in_turn(variants, a.reps, a.rounds, cuda)
            if cuda:
                b = sampler.batch([0])
                assert all(int(b[k]) == 0 for k in b if k.endswith(("outside_track", "bad_choice", "bad_index")))
            emit(what="event_batch", M=M, no_event_rays=with_no_evs,
                 **{f"{k}_{unit}_us": round(v[i], 2) for k, v in res.items() for i, unit in enumerate(("device", "host"))},
                 device_us_rounds={k: v[2] for k, v in res.items()})


if __name__ == "__main__":
    main()
