"""The background model (bg_radius > 0) on one GPU: the native node (enerf_amd/background.py, one launch forward, one plus a
small reduce backward) against the op-by-op statement it replaces (polar_from_ray, SH encoder, grid encoder, cat, two
nn.Linear, sigmoid and their autograd), from the same model, alternating in one process, warmed.

  node      forward + backward of the background alone at 4096 and 30 096 rays (training batches) and 307 200 rays (a 640 x
            480 frame; forward alone as well, which is what evaluation runs); device time between hip events, median
  step      TrainHarness.step_frames on a cuda_ray background model, native against background.ENABLED = False (the route
            every background model took before: the statement's launch chain into _train_ops); host clock around
            synchronised blocks of steps, median per step
  frame     model.render of 307 200 rays in evaluation mode, native (whole-frame pass) against ENABLED = False (rounds)

One JSON line per measurement, appended to profiles/background_bench.jsonl as well.

    python tools/bench_background.py [--reps 20] [--steps 48] [--out profiles/background_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from enerf_amd import background, raymarching, scene  # noqa: E402
from enerf_amd.network import NeRFNetwork  # noqa: E402

DEV = "cuda"
RADIUS = 3.0
OUT = None


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if OUT is not None:
        OUT.write(line + "\n")
        OUT.flush()


def rays(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(n, 3, device=DEV, generator=g), dim=-1)
    o = torch.nn.functional.normalize(torch.randn(n, 3, device=DEV, generator=g), dim=-1) * 1.5
    return o.contiguous(), d.contiguous()


def ev_time(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def node(model, n, reps):
    ro, rd = rays(n, n)
    g = torch.randn(n, model.out_dim_color, device=DEV)
    params = [model.encoder_bg.embeddings, model.bg_net[0].weight, model.bg_net[1].weight]

    def native(train):
        bg = background.background_from_rays(model, ro, rd)
        if train:
            torch.autograd.grad(bg, params, g)

    def statement(train):
        bg = model.background(raymarching.polar_from_ray(ro, rd, RADIUS), rd)
        if train:
            torch.autograd.grad(bg, params, g)

    for train in (True, False):
        for _ in range(3):
            native(train), statement(train)
        res = {}
        for _ in range(2):                                   # alternating: either arm sees the other's cache state
            for name, fn in (("native", native), ("statement", statement)):
                with torch.set_grad_enabled(train):
                    med, best = ev_time(lambda: fn(train), reps)
                res[name] = min(res.get(name, (med, best)), (med, best))
        emit(what="node", rays=n, mode="fwd+bwd" if train else "fwd", native_us=res["native"][0],
             statement_us=res["statement"][0], native_min_us=res["native"][1], statement_min_us=res["statement"][1],
             speedup=res["statement"][0] / res["native"][0])


def steps(n_rays, n_steps):
    import argparse as ap
    from enerf_amd.trainer import TrainHarness
    res = {}
    for native in (True, False, True, False):
        background.ENABLED = native
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3, bg_radius=RADIUS).to(DEV)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        g = torch.Generator(device=DEV).manual_seed(1)
        batches = []
        for b in range(4):
            (ro, rd), _ = scene.training_batch(b, n_rays, DEV, generator=g)
            batches.append({"rays_o": ro.view(1, -1, 3), "rays_d": rd.view(1, -1, 3),
                            "images": torch.rand(1, n_rays, 3, device=DEV, generator=g)})
        opt = ap.Namespace(out_dim_color=3, color_space="srgb", render_kwargs={})
        for i in range(20):                                   # past the first update_extra_state: a sample budget exists
            h.step_frames(batches[i % 4], opt)
        ts = []
        for blk in range(n_steps // 8):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(8):
                h.step_frames(batches[i % 4], opt)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / 8)
        key = "native" if native else "before"
        res[key] = min(res.get(key, 1e9), float(np.median(ts)))
    background.ENABLED = True
    emit(what="step_frames", rays=n_rays, native_ms=res["native"] * 1e3, before_ms=res["before"] * 1e3,
         speedup=res["before"] / res["native"])


def frame(reps):
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3, bg_radius=RADIUS).to(DEV).eval()
    model.encoder.embeddings.data.uniform_(-0.5, 0.5)
    scene.install_occupancy(model)
    inds = torch.arange(scene.H * scene.W, device=DEV)
    ro, rd = scene.pixel_rays(scene.pose(3), inds, DEV)
    res = {}
    with torch.no_grad():
        for native in (True, False, True, False):
            background.ENABLED = native
            model.render(ro, rd, staged=False, perturb=False)
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.render(ro, rd, staged=False, perturb=False)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            key = "native" if native else "before"
            res[key] = min(res.get(key, 1e9), float(np.median(ts)))
    background.ENABLED = True
    emit(what="frame", rays=int(ro.numel() // 3), native_ms=res["native"] * 1e3, before_ms=res["before"] * 1e3,
         speedup=res["before"] / res["native"])


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "background_bench.jsonl"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    OUT = open(a.out, "w")
    emit(what="device", name=torch.cuda.get_device_name(0), torch=torch.__version__)
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3, bg_radius=RADIUS).to(DEV)
    model.encoder_bg.embeddings.data.uniform_(-0.5, 0.5)
    for n in (4096, 30096, 307200):
        node(model, n, a.reps)
    del model
    steps(4096, a.steps)
    frame(max(3, a.reps // 4))
    OUT.close()


if __name__ == "__main__":
    main()
