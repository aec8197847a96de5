"""Event-only training on the stratified sampler (cuda_ray off), `fp16 = True`: does the native fp16 regime
(TrainHarness(fp16=True): stratified.py at mlp_precision 3, fp16 colour rows, GradScaler host protocol) train to the same
held-out quality as what `fp16 = True` ran before it, the PyTorch statement under torch.autocast(float16) + GradScaler
(TrainHarness(fp16="autocast"))?

Paired by seed: both arms start from the same weights and train on the same synthetic event batches (tools/psnr_ab_events.py's
teacher: the analytic scene seen from two poses DELTA_DEG apart, real-valued polarities).  Held-out metric on 16 K pixel
pairs of an untrained pose pair, rendered by the native route in its default arithmetic whatever the arm:
`event_db` = -10 log10 mean((delta - pols * C)^2).  Prints one line per run and a JSON summary with the paired
difference N - S (mean, standard deviation, standard error).

    python tools/psnr_ab_events_strat.py [steps] [pairs] [out.json] [first_seed]
"""
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from enerf_amd import scene, stratified  # noqa: E402
from enerf_amd.events import EventOptions, lin_log, rgb_to_luma  # noqa: E402
from enerf_amd.network import NeRFNetwork  # noqa: E402
from enerf_amd.trainer import TrainHarness  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 8
out_path = sys.argv[3] if len(sys.argv) > 3 else None
first_seed = int(sys.argv[4]) if len(sys.argv) > 4 else 0
RAYS = int(os.environ.get("ENERF_AB_RAYS", "4096"))
NUM_STEPS = int(os.environ.get("ENERF_AB_NUM_STEPS", "128"))
DELTA_DEG = 1.0
C_THRES = 0.2
DEV = "cuda"
KW = {"num_steps": NUM_STEPS, "upsample_steps": 0}


def teacher(ro, rd):
    b_ = (ro * rd).sum(-1)
    disc = b_ ** 2 - ((ro * ro).sum(-1) - 0.36)
    hit = disc > 0
    t = -b_ - torch.sqrt(disc.clamp(min=0))
    p = ro + rd * t.unsqueeze(-1)
    return torch.where(hit.unsqueeze(-1), scene.analytic_color(p).clamp(0, 1), torch.ones_like(p))


def linlog_luma(img):
    return lin_log(rgb_to_luma(img, esim=True) * 255, linlog_thres=20)


def pair(k, n_rays, gen):
    inds = torch.randint(0, scene.H * scene.W, (n_rays,), device=DEV, generator=gen)
    o1, d1 = scene.pixel_rays(scene.pose(k), inds, DEV)
    o2, d2 = scene.pixel_rays(scene.pose(k + DELTA_DEG / (360.0 / 32)), inds, DEV)
    pols = ((linlog_luma(teacher(o2, d2)) - linlog_luma(teacher(o1, d1))) / C_THRES).reshape(1, n_rays).contiguous()
    return {"images": torch.zeros(1, n_rays, 3, device=DEV), "rays_evs_o1": o1, "rays_evs_d1": d1, "rays_evs_o2": o2,
            "rays_evs_d2": d2, "pols": pols}


_g = torch.Generator(device=DEV).manual_seed(5)
data = [pair((b * 7) % 32, RAYS, _g) for b in range(32)]
_g = torch.Generator(device=DEV).manual_seed(77)
held = pair(10.37, 16384, _g)


def evaluate(model):
    model.eval()
    with torch.no_grad():
        kw = dict(staged=True, max_ray_batch=4096, bg_color=None, perturb=False, out_dim_color=3, **KW)
        i1 = model.render(held["rays_evs_o1"], held["rays_evs_d1"], **kw)["image"]
        i2 = model.render(held["rays_evs_o2"], held["rays_evs_d2"], **kw)["image"]
    model.train()
    p1, p2 = linlog_luma(i1.reshape(1, -1, 3)).reshape(-1), linlog_luma(i2.reshape(1, -1, 3)).reshape(-1)
    ev = float((((p2 - p1) - held["pols"].reshape(-1) * C_THRES) ** 2).mean())
    return -10 * math.log10(max(ev, 1e-30))


def run(arm, seed):
    torch.manual_seed(seed)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=False, out_dim_color=3).cuda()
    h = TrainHarness(model, lr=1e-2, fp16=True if arm == "N" else "autocast")
    assert h.strat_f16 == (arm == "N")
    opt = EventOptions(use_luma=True, linlog=True, C_thres=C_THRES, event_only=True, render_kwargs=dict(KW))
    calls = stratified.stats["calls"]
    torch.manual_seed(1000 + seed)
    torch.cuda.synchronize()
    t0 = time.time()
    for i in range(steps):
        loss = h.step_events(data[i % len(data)], opt)
    torch.cuda.synchronize()
    ms = 1e3 * (time.time() - t0) / steps
    native = stratified.stats["calls"] - calls
    return {"arm": arm, "seed": seed, "event_db": evaluate(model), "final_loss": float(loss), "ms_per_step": ms,
            "native_renders": native, "scale": float(h.scaler.get_scale())}


rows = []
for seed in range(first_seed, first_seed + pairs):
    for arm in "NS":
        r = run(arm, seed)
        rows.append(r)
        print(json.dumps(r), flush=True)
d = [a["event_db"] - b["event_db"] for a, b in zip(rows[0::2], rows[1::2])]
m = sum(d) / len(d)
sd = (sum((x - m) ** 2 for x in d) / max(len(d) - 1, 1)) ** 0.5
summary = {"steps": steps, "pairs": len(d), "rays": RAYS, "num_steps": NUM_STEPS,
           "arms": {"N": "TrainHarness(fp16=True): native stratified fp16 regime",
                    "S": "TrainHarness(fp16='autocast'): the statement under autocast(float16) + GradScaler"},
           "mean_event_db": {a: sum(r["event_db"] for r in rows if r["arm"] == a) / len(d) for a in "NS"},
           "mean_ms_per_step": {a: sum(r["ms_per_step"] for r in rows if r["arm"] == a) / len(d) for a in "NS"},
           "paired_N_minus_S_event_db": {"mean": m, "std": sd, "standard_error": sd / len(d) ** 0.5}}
print(json.dumps(summary), flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(dict(summary, runs=rows), f, indent=1)
