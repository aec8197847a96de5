"""The stratified sampler (cuda_ray off: NeRFRenderer.run, the route every shipped config trains with) on one GPU, native
route (enerf_amd/stratified.py) vs the PyTorch statement (sampler.render_stratified), alternating windows:

  (a) event   shakeCarpet1_enerf's event-only step: bound 3, 20 096 pairs x 512 samples, out_dim_color 1, C_thres 0.2,
              Adam lr 5e-3 (two renders + event loss + backward + Adam)
  (b) rgb     an RGB step at 4096 rays x 512 (MSE, Adam)
  (c) frame   one 640 x 480 eval frame, staged=True, max_ray_batch=5096

Every window: `--warmup` untimed steps, a device synchronisation, then `--steps` steps between two device events.  Prints
one JSON line per shape and arm (ms per step or frame, samples/s) and one per shape with the masked fraction and the
largest output difference between the arms on the same inputs.

    python tools/bench_stratified.py [--shapes event,rgb,frame] [--steps 10] [--warmup 3] [--windows 2] [--fp16]

--fp16: the `fp16 = True` regime, three arms per shape in rotating order: "native_f16" (the native route at
mlp_precision 3 with its fp16 colour rows, GradScaler host protocol, no autocast), "autocast" (the statement under
torch.autocast(float16) + GradScaler: what `fp16 = True` on a cuda_ray-off model ran before the native fp16 regime) and
"native_f32" (the native route in the default arithmetic, for reference).  The comparison line gives the largest
output difference between native_f16 and autocast.
"""
import contextlib
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from enerf_amd import events, scene, stratified  # noqa: E402
from enerf_amd.events import EventOptions  # noqa: E402
from enerf_amd.network import NeRFNetwork  # noqa: E402

DEV = "cuda"
T = 512


def _model(bound, C, seed=0):
    torch.manual_seed(seed)
    return NeRFNetwork(encoding="hashgrid", bound=bound, cuda_ray=False, out_dim_color=C).to(DEV).train()


def _adam(model):
    return torch.optim.Adam(model.get_params(5e-3), betas=(0.9, 0.99), eps=1e-15)


def _event_batch(n, seed):
    g = torch.Generator().manual_seed(seed)
    inds = torch.randint(0, scene.H * scene.W, (n,), generator=g)
    k = seed % 32
    o1, d1 = scene.pixel_rays(scene.pose(k), inds, "cpu")
    o2, d2 = scene.pixel_rays(scene.pose(k + 1.0 / (360.0 / 32)), inds, "cpu")
    pols = torch.where(torch.rand(1, n, generator=g) < 0.5, -1.0, 1.0)
    data = {"images": torch.zeros(1, n, 1), "rays_evs_o1": o1, "rays_evs_d1": d1, "rays_evs_o2": o2, "rays_evs_d2": d2,
            "pols": pols}
    return {k_: v.to(DEV) for k_, v in data.items()}


class Event:
    name, rays, renders = "event", 20096, 2

    def __init__(self):
        self.model = _model(3, 1)
        self.adam = _adam(self.model)
        self.opt = EventOptions(out_dim_color=1, use_luma=False, linlog=True, C_thres=0.2, event_only=True,
                                render_kwargs={"num_steps": T, "upsample_steps": 0})
        self.batches = [_event_batch(self.rays, 1000 + i) for i in range(4)]
        self.i = 0

    def outputs(self, model):
        kw = dict(staged=False, perturb=True, num_steps=T, upsample_steps=0, out_dim_color=1)
        b = self.batches[0]
        bg = torch.full((1, 1, 1), 0.4, device=DEV)
        torch.manual_seed(7)
        o1 = model.render(b["rays_evs_o1"], b["rays_evs_d1"], bg_color=bg, **kw)["image"]
        o2 = model.render(b["rays_evs_o2"], b["rays_evs_d2"], bg_color=bg, **kw)["image"]
        loss, _ = events.event_loss(o1, o2, b["pols"], self.opt)
        return [o1, o2, loss.reshape(1)]

    def step(self):
        data = self.batches[self.i % len(self.batches)]
        self.i += 1
        self.adam.zero_grad(set_to_none=True)
        with _autocast(self):
            loss, _ = events.train_step_events(self.model, data, self.opt)
        _backward_step(self, loss)


class Rgb:
    name, rays, renders = "rgb", 4096, 1

    def __init__(self):
        self.model = _model(2, 3)
        self.adam = _adam(self.model)
        g = torch.Generator().manual_seed(5)
        self.batches = []
        for i in range(4):
            inds = torch.randint(0, scene.H * scene.W, (self.rays,), generator=g)
            ro, rd = scene.pixel_rays(scene.pose(i), inds, "cpu")
            self.batches.append((ro.to(DEV), rd.to(DEV), torch.rand(1, self.rays, 3, generator=g).to(DEV)))
        self.i = 0

    def outputs(self, model):
        ro, rd, _ = self.batches[0]
        torch.manual_seed(7)
        out = model.render(ro, rd, staged=False, bg_color=None, perturb=True, num_steps=T, upsample_steps=0,
                           out_dim_color=3)
        return [out["image"], out["depth"]]

    def step(self):
        ro, rd, target = self.batches[self.i % len(self.batches)]
        self.i += 1
        self.adam.zero_grad(set_to_none=True)
        with _autocast(self):
            out = self.model.render(ro, rd, staged=False, bg_color=None, perturb=True, num_steps=T, upsample_steps=0,
                                    out_dim_color=3)
            loss = ((out["image"] - target) ** 2).mean()
        _backward_step(self, loss)


class Frame:
    name, rays, renders = "frame", scene.H * scene.W, 1

    def __init__(self):
        self.model = _model(2, 3).eval()
        inds = torch.arange(self.rays)
        self.ro, self.rd = (x.to(DEV) for x in scene.pixel_rays(scene.pose(3), inds, "cpu"))

    def outputs(self, model):
        with torch.no_grad():
            out = model.render(self.ro, self.rd, staged=True, max_ray_batch=5096, bg_color=None, perturb=False,
                               num_steps=T, upsample_steps=0, out_dim_color=3)
        return [out["image"], out["depth"]]

    def step(self):
        with _autocast(self):
            self.outputs(self.model)


def _autocast(shape):
    return torch.autocast("cuda", dtype=torch.float16) if getattr(shape, "autocast", False) else contextlib.nullcontext()


def _backward_step(shape, loss):
    """plain backward + Adam, or the GradScaler's host protocol in the fp16 arms (scale, backward, step, update)"""
    sc = getattr(shape, "scaler", None)
    if sc is None:
        loss.backward()
        shape.adam.step()
        return
    sc.scale(loss).backward()
    sc.step(shape.adam)
    sc.update()


def _set(on):
    stratified.ENABLED = on


def _set_arm(shape, arm):
    """--fp16 arms: native_f16 / autocast / native_f32 (see the module docstring)"""
    _set(arm != "autocast")
    if arm == "native_f16":
        shape.model.mlp_precision = 3
    else:
        shape.model.__dict__.pop("mlp_precision", None)
    shape.autocast = arm == "autocast"
    if hasattr(shape, "adam"):
        if arm == "native_f32":
            shape.scaler = None
        else:
            if getattr(shape, "_scaler", None) is None:
                shape._scaler = torch.amp.GradScaler("cuda")
            shape.scaler = shape._scaler


def _window(shape, on, steps, warmup, arm=None):
    if arm is None:
        _set(on)
    else:
        _set_arm(shape, arm)
    calls = stratified.stats["calls"]
    for _ in range(warmup):
        shape.step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        shape.step()
    b.record()
    torch.cuda.synchronize()
    took = stratified.stats["calls"] - calls
    assert (took > 0) == on, (on, took)
    return a.elapsed_time(b) / steps


def _compare(shape):
    """largest |difference| between the arms' outputs on the same model, inputs and random draws; masked fraction"""
    model = shape.model
    stratified.KEEP_LAST = True
    _set(True)
    got = [x.detach().float() for x in shape.outputs(model)]
    last = stratified.last
    masked = float(last["count"].sum().item()) / float(last["w"].numel())
    stratified.KEEP_LAST = False
    stratified.last = None
    _set(False)
    ref = [x.detach().float() for x in shape.outputs(model)]
    diff = max(float((g - r).abs().nan_to_num(0.0).max().item()) for g, r in zip(got, ref))
    return masked, diff


def _compare_fp16(shape):
    """native_f16 vs autocast on the same model, inputs and random draws: largest |difference|, masked fraction"""
    stratified.KEEP_LAST = True
    _set_arm(shape, "native_f16")
    with _autocast(shape):
        got = [x.detach().float() for x in shape.outputs(shape.model)]
    last = stratified.last
    masked = float(last["count"].sum().item()) / float(last["w"].numel())
    stratified.KEEP_LAST = False
    stratified.last = None
    _set_arm(shape, "autocast")
    with _autocast(shape):
        ref = [x.detach().float() for x in shape.outputs(shape.model)]
    diff = max(float((g - r).abs().nan_to_num(0.0).max().item()) for g, r in zip(got, ref))
    return masked, diff


def main_fp16(a, classes):
    arms = a.arms.split(",")
    for name in a.shapes.split(","):
        shape = classes[name]()
        masked, diff = _compare_fp16(shape)
        steps = max(1, a.steps // 4) if name == "frame" else a.steps
        times = {arm: [] for arm in arms}
        for w in range(a.windows):
            order = arms[w % len(arms):] + arms[:w % len(arms)]
            for arm in order:
                times[arm].append(_window(shape, arm != "autocast", steps, a.warmup if name != "frame" else 1, arm))
        samples = shape.rays * shape.renders * T
        res = {}
        for arm in arms:
            ms = float(np.median(times[arm]))
            res[arm] = ms
            print(json.dumps({"shape": name, "arm": arm, "ms": round(ms, 3),
                              "windows_ms": [round(x, 3) for x in times[arm]], "samples_per_step": samples,
                              "samples_per_s": round(samples / ms * 1e3, 1)}), flush=True)
        line = {"shape": name, "masked_fraction": round(masked, 5), "max_abs_diff_f16_vs_autocast": diff}
        if "native_f16" in res and "autocast" in res:
            line["speedup_f16_over_autocast"] = round(res["autocast"] / res["native_f16"], 3)
        if "native_f16" in res and "native_f32" in res:
            line["speedup_f16_over_f32"] = round(res["native_f32"] / res["native_f16"], 3)
        print(json.dumps(line), flush=True)
        del shape
        torch.cuda.empty_cache()
    _set(True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="event,rgb,frame")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=2)
    ap.add_argument("--fp16", action="store_true")
    ap.add_argument("--arms", default="native_f16,autocast,native_f32", help="--fp16: arms to time (profiling: one)")
    a = ap.parse_args()
    classes = {"event": Event, "rgb": Rgb, "frame": Frame}
    if a.fp16:
        return main_fp16(a, classes)
    for name in a.shapes.split(","):
        shape = classes[name]()
        masked, diff = _compare(shape)
        steps = max(1, a.steps // 4) if name == "frame" else a.steps
        times = {True: [], False: []}
        for w in range(a.windows):
            for on in ((True, False) if w % 2 == 0 else (False, True)):
                times[on].append(_window(shape, on, steps, a.warmup if name != "frame" else 1))
        samples = shape.rays * shape.renders * T
        res = {}
        for on in (True, False):
            ms = float(np.median(times[on]))
            res["native" if on else "torch"] = ms
            print(json.dumps({"shape": name, "arm": "native" if on else "torch", "ms": round(ms, 3),
                              "windows_ms": [round(x, 3) for x in times[on]], "samples_per_step": samples,
                              "samples_per_s": round(samples / ms * 1e3, 1)}), flush=True)
        print(json.dumps({"shape": name, "masked_fraction": round(masked, 5), "max_abs_diff": diff,
                          "speedup_native_over_torch": round(res["torch"] / res["native"], 3)}), flush=True)
        del shape
        torch.cuda.empty_cache()
    _set(True)


if __name__ == "__main__":
    main()
