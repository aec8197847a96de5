"""The implicit contrast threshold's medians (enerf_event_c_estimate, one launch) against the torch statement they
replace, and the one-call event step with a TrainLog attached against the same harness without.  One GPU, device events,
alternating windows, medians (tools/bench_event_loss.py's method).

  a  estimate   event_diag.estimate_C_thres (the kernel) against event_diag.estimate_C_thres_statement run on the device
                (four torch.where, four torch.median: each where is a read-back), at N = 20 096, C = 1 and N = 65 536,
                C = 3, each on random deltas and on all-zero deltas (every key of the radix select in one bin: early
                training, where both renders return the background)
  b  step       TrainHarness.step_events at tools/bench_gray.py's shape (20 096 pairs, bound 3, one channel, C_thres 0.2:
                the one-call native step), the SAME harness with a log attached and without, taking turns; a logged
                window ends with the log's flush (its one read-back), inside the timed span

A window is `--warmup` untimed calls, a device synchronisation, then `--reps` (part b: `--steps`) calls back to back between
two device events.  Every line carries all windows, their median and their spread (max - min): the run-to-run noise a
difference has to exceed.

    python tools/bench_c_estimate.py [--parts a,b] [--windows 5] [--label this]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from enerf_amd import event_diag, fused_render  # noqa: E402
from enerf_amd.events import EventOptions  # noqa: E402

DEV = "cuda"
PAIRS, BOUND = 20096, 3


def _inputs(n, C, zero, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    pols = torch.where(torch.rand(1, n, device=DEV, generator=g) < 0.5, 1.0, -1.0)
    delta = torch.zeros(1, n, C, device=DEV) if zero else pols[..., None] * 0.2 + 0.15 * torch.randn(1, n, C, device=DEV,
                                                                                                  generator=g)
    return pols.contiguous(), delta.contiguous()


def _window_us(fn, reps, warmup, after=None):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    if after is not None:
        after()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps


def _summary(xs, digits):
    return {"median": round(float(np.median(xs)), digits), "spread": round(float(max(xs) - min(xs)), digits),
            "windows": [round(float(x), digits) for x in xs]}


def _estimate_cases():
    cases = {}
    for n, C in ((20096, 1), (65536, 3)):
        for zero in (False, True):
            pols, delta = _inputs(n, C, zero)
            out = torch.empty(8, device=DEV)
            p2, d2 = pols[0][:, None].contiguous(), delta[0].contiguous()
            cases[f"n{n}_c{C}_" + ("zero" if zero else "random")] = (
                n, C, lambda pols=pols, delta=delta, out=out: event_diag.estimate_C_thres(pols, delta, out=out),
                lambda p2=p2, d2=d2: event_diag.estimate_C_thres_statement(p2, d2))
    return cases


class Step:
    """The one-call event step of a one-channel cuda_ray model through TrainHarness, with and without a log."""

    def __init__(self):
        from bench_gray import _event_batch
        from enerf_amd.network import NeRFNetwork
        from enerf_amd.train_log import TrainLog
        from enerf_amd.trainer import TrainHarness
        torch.manual_seed(0)
        self.model = NeRFNetwork(encoding="hashgrid", bound=BOUND, cuda_ray=True, out_dim_color=1).to(DEV)
        self.h = TrainHarness(self.model, lr=5e-3, occupancy="synthetic")
        self.opt = EventOptions(out_dim_color=1, use_luma=False, linlog=True, C_thres=0.2, event_only=True)
        self.batches = [_event_batch(PAIRS, 1, 1000 + i) for i in range(4)]
        self.log = TrainLog()
        self.i = self.native = 0
        orig = fused_render.train_step_events_native

        def counted(m, *a, **k):
            self.native += 1
            return orig(m, *a, **k)
        self._counted, self._orig = counted, orig

    def step(self, logged=False):
        data, nxt = self.batches[self.i % 4], self.batches[(self.i + 1) % 4]
        self.i += 1
        fused_render.train_step_events_native = self._counted
        self.h._log = self.log if logged else None      # (what train_one_epoch(log=...) does around its steps)
        try:
            self.h.step_events(data, self.opt, next_data=nxt)
            if logged:
                self.log.end_step(self.h.global_step, self.h.epoch, self.h.opt.param_groups[0]["lr"])
        finally:
            self.h._log = None
            fused_render.train_step_events_native = self._orig

    def window_ms(self, logged, steps, warmup):
        before = self.native
        if logged:
            self.log.begin(steps + warmup, DEV)
        us = _window_us(lambda: self.step(logged), steps, warmup, after=self.log.flush if logged else None)
        assert self.native - before >= 0.9 * steps, (self.native - before, steps)    # the one-call route was the one timed
        return us / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "c_estimate_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_c_estimate: no GPU (nothing here is measured without one)")
    parts, lines = a.parts.split(","), []
    head = {"bench": "c_estimate", "label": a.label, "device": torch.cuda.get_device_name(0)}
    if "a" in parts:
        cases = _estimate_cases()
        arms = [(n, r) for n in cases for r in ("kernel", "statement")]
        times = {arm: [] for arm in arms}
        for w in range(a.windows):
            for n, r in arms[w % len(arms):] + arms[:w % len(arms)]:
                times[(n, r)].append(_window_us(cases[n][2 if r == "kernel" else 3], a.reps, a.warmup))
        for n, (events, C, _, _) in cases.items():
            k, s = _summary(times[(n, "kernel")], 2), _summary(times[(n, "statement")], 2)
            lines.append(dict(head, part="a", case=n, events=events, channels=C, reps_per_window=a.reps,
                              kernel_us_per_call=k, statement_us_per_call=s, kernel_launches_per_call=1,
                              statement_over_kernel=round(s["median"] / k["median"], 2)))
    if "b" in parts:
        arm = Step()
        for _ in range(24):                     # out of the cold window (no sample budget during the first 16 renders)
            arm.step()
        names = ["plain", "logged"]
        times = {n: [] for n in names}
        for w in range(a.windows):
            for n in names[w % 2:] + names[:w % 2]:
                times[n].append(arm.window_ms(n == "logged", a.steps, a.warmup))
        p, q = _summary(times["plain"], 4), _summary(times["logged"], 4)
        lines.append(dict(head, part="b", pairs=PAIRS, bound=BOUND, steps_per_window=a.steps, ms_per_step_plain=p,
                          ms_per_step_logged=q, logged_minus_plain_us=round((q["median"] - p["median"]) * 1e3, 2),
                          launches_added_per_logged_step=2, rows_logged=len(arm.log.rows())))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
