"""The normalised event loss (C_thres = -1) and the no-event hinge as library calls against the torch statements they
replace, and the marching-route event step around them.  One GPU, device events, alternating windows, medians.

  a  loss_norm   events.event_loss_with_grads (one launch: enerf_event_loss_fwd_bwd_c) against events.event_loss +
                 autograd.grad on the same [1, 20096, C] images, for C = 1 and for C = 3 with luma
  b  hinge       events.no_event_loss_with_grads (enerf_no_event_loss_fwd_bwd_c) against events.no_event_loss +
                 autograd.grad at N = 10048, C = 1
  c  step        TrainHarness.step_events at shakeCarpet1_enerf's shape (20 096 pairs, bound 3, one channel), steady state:
                   manual       C_thres = -1 on the Python-driven route (train_step_events_manual)
                   native_norm  C_thres = -1 with native_normalised = True (the one-call step)
                   native_c02   C_thres = 0.2 on the one-call step, for scale

Parts a and b: a window is `--warmup` untimed calls, a device synchronisation, then `--reps` calls back to back between two
device events; the figure is microseconds per call of that window (what the stream spends per call, host enqueue
included where the host is the slower side -- it is, for the ~50 small launches of the autograd route).  Part c: the same
with steps.  The arms of a part take turns, rotating the order from window to window; every line carries all windows, their
median and their spread (max - min), which is the run-to-run noise a difference has to exceed.  Launch counts of parts a
and b come from a pass of their own under torch.profiler (device kernels per call), in a child process, after the timings.

Part c runs on any commit whose TrainHarness has step_events (`--parts c --arms manual --label parent` on the parent of
the commit that added the kernels: there the manual route takes its loss through autograd).

    python tools/bench_event_loss.py [--parts a,b,c] [--arms manual,native_norm,native_c02] [--windows 5] [--label this]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from enerf_amd import events, fused_render, scene  # noqa: E402
from enerf_amd.events import EventOptions  # noqa: E402

DEV = "cuda"
PAIRS, NO_EVENT_RAYS, BOUND = 20096, 10048, 3


def _images(n, C, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = (torch.rand(1, n, C, device=DEV, generator=g) ** 3).clamp(1e-4, 1.0)
    b = (a + 0.05 * torch.randn(1, n, C, device=DEV, generator=g)).clamp(1e-4, 1.0)
    pols = torch.randint(-3, 4, (1, n), device=DEV, generator=g).float()
    return a, b, pols


def _autograd_event_loss(a, b, pols, opt):
    ar, br = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
    loss, _ = events.event_loss(ar, br, pols, opt)
    return torch.autograd.grad(loss, [ar, br])


def _autograd_hinge(a, b, opt):
    ar, br = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
    return torch.autograd.grad(events.no_event_loss(ar, br, opt), [ar, br])


def _loss_cases():
    """name -> (fused call, autograd call) of parts a and b."""
    cases = {}
    for C, luma in ((1, False), (3, True)):
        a, b, pols = _images(PAIRS, C)
        opt = EventOptions(out_dim_color=C, use_luma=luma, linlog=True, C_thres=-1, event_only=True)
        cases[f"loss_norm_c{C}" + ("_luma" if luma else "")] = (
            "a", PAIRS, lambda a=a, b=b, pols=pols, opt=opt: events.event_loss_with_grads(a, b, pols, opt),
            lambda a=a, b=b, pols=pols, opt=opt: _autograd_event_loss(a, b, pols, opt))
    a, b, _ = _images(NO_EVENT_RAYS, 1)
    opt = EventOptions(out_dim_color=1, use_luma=False, linlog=True, C_thres=0.2, w_no_ev=1.0)
    cases["hinge_c1"] = ("b", NO_EVENT_RAYS, lambda: events.no_event_loss_with_grads(a, b, opt),
                         lambda: _autograd_hinge(a, b, opt))
    return cases


def _window_us(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps


def _summary(xs, digits):
    return {"median": round(float(np.median(xs)), digits), "spread": round(float(max(xs) - min(xs)), digits),
            "windows": [round(float(x), digits) for x in xs]}


def count_launches():
    """Device kernels per call of both routes of every loss case (torch.profiler); prints one JSON object."""
    from torch.profiler import ProfilerActivity, profile
    out = {}
    for name, (_, _, fused, autograd) in _loss_cases().items():
        for route, fn in (("fused", fused), ("autograd", autograd)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            calls = 10
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                for _ in range(calls):
                    fn()
                torch.cuda.synchronize()
            kernels = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
                       and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
            out[f"{name}.{route}"] = len(kernels) / calls
    print(json.dumps(out), flush=True)


class Step:
    """The event step of a one-channel cuda_ray model through TrainHarness (tools/bench_gray.py's arm)."""

    def __init__(self, C_thres, native_normalised, want_native):
        from enerf_amd.network import NeRFNetwork
        from enerf_amd.trainer import TrainHarness
        from bench_gray import _event_batch
        torch.manual_seed(0)
        self.model = NeRFNetwork(encoding="hashgrid", bound=BOUND, cuda_ray=True, out_dim_color=1).to(DEV)
        self.h = TrainHarness(self.model, lr=5e-3, occupancy="synthetic")
        self.h.native_normalised = native_normalised
        self.opt = EventOptions(out_dim_color=1, use_luma=False, linlog=True, C_thres=C_thres, event_only=True)
        self.batches = [_event_batch(PAIRS, 1, 1000 + i) for i in range(4)]
        self.i, self.native, self.want_native = 0, 0, want_native
        orig = fused_render.train_step_events_native

        def counted(m, *a, **k):
            if m is self.model:
                self.native += 1
            return orig(m, *a, **k)
        self._counted, self._orig = counted, orig

    def step(self):
        data, nxt = self.batches[self.i % 4], self.batches[(self.i + 1) % 4]
        self.i += 1
        fused_render.train_step_events_native = self._counted
        try:
            self.h.step_events(data, self.opt, next_data=nxt)
        finally:
            fused_render.train_step_events_native = self._orig

    def window_ms(self, steps, warmup):
        before = self.native
        us = _window_us(self.step, steps, warmup)
        took = self.native - before
        # the arm ran on the route it is named for (warm-up steps included in the count)
        assert (took >= 0.9 * steps) if self.want_native else took == 0, (took, steps)
        return us / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--arms", default="manual,native_norm,native_c02")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--label", default="this")
    ap.add_argument("--no-launch-counts", action="store_true")
    ap.add_argument("--count-launches", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "event_loss_normalised_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_event_loss: no GPU (nothing here is measured without one)")
    if a.count_launches:
        return count_launches()
    parts, lines = a.parts.split(","), []
    head = {"bench": "event_loss_normalised", "label": a.label, "device": torch.cuda.get_device_name(0)}
    cases = {n: c for n, c in _loss_cases().items() if c[0] in parts} if ("a" in parts or "b" in parts) else {}
    if cases:
        arms = [(n, r) for n in cases for r in ("fused", "autograd")]
        times = {arm: [] for arm in arms}
        for w in range(a.windows):
            for n, r in arms[w % len(arms):] + arms[:w % len(arms)]:
                times[(n, r)].append(_window_us(cases[n][2 if r == "fused" else 3], a.reps, a.warmup))
        counts = {}
        if not a.no_launch_counts:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--count-launches"], capture_output=True,
                                   text=True, timeout=300)
                counts = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else {}
            except Exception as e:                                   # noqa: BLE001  (the timings stand without the counts)
                print(f"launch counts not measured: {e!r}", file=sys.stderr)
        for n, (part, rays, _, _) in cases.items():
            f, g = _summary(times[(n, "fused")], 2), _summary(times[(n, "autograd")], 2)
            lines.append(dict(head, part=part, case=n, rays=rays, reps_per_window=a.reps, fused_us_per_call=f,
                              autograd_us_per_call=g, autograd_over_fused=round(g["median"] / f["median"], 2),
                              fused_launches_per_call=counts.get(n + ".fused"),
                              autograd_launches_per_call=counts.get(n + ".autograd")))
    if "c" in parts:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        make = {"manual": lambda: Step(-1, False, False), "native_norm": lambda: Step(-1, True, True),
                "native_c02": lambda: Step(0.2, False, True)}
        names = a.arms.split(",")
        arms = {n: make[n]() for n in names}
        for arm in arms.values():               # out of the cold window (no sample budget during the first 16 renders)
            for _ in range(24):
                arm.step()
        times = {n: [] for n in names}
        for w in range(a.windows):
            for n in names[w % len(names):] + names[:w % len(names)]:
                times[n].append(arms[n].window_ms(a.steps, a.warmup))
        for n in names:
            lines.append(dict(head, part="c", arm=n, pairs=PAIRS, bound=BOUND, steps_per_window=a.steps,
                              ms_per_step=_summary(times[n], 4), samples_per_step=int(arms[n].model.mean_count) * 2))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
