"""TrainHarness.save_mesh at R = 256 (the reference's defaults) on one GPU, against the reference's procedure on the same
GPU, alternating windows in one process:

  native      harness.save_mesh: lattice kernel + density_sigma in 2^21-point slabs, enerf_marching_cubes_*, PLY write
  reference   the reference's extract_fields (model.density in 128^3 blocks, each block copied to the host) and marching
              cubes on the host through mesh.marching_cubes_statement on the CPU (PyMCubes is not installed), PLY write

The model: a cuda_ray = False NeRFNetwork (bound 2) after `--train` RGB steps on the synthetic scene (rays through the
analytic colour sphere of enerf_amd/scene.py).  `--fp16`: the shipped `fp16 = True` harness (strat_f16) and the reference
procedure under autocast(float16).  Every window: one untimed call per arm, then `--reps` calls per arm, each between a
device synchronisation and a host clock; the native call is also split into field / marching cubes / PLY.  One JSON line
per arm and window, and a summary line with the medians.

    python tools/bench_mesh.py [--resolution 256] [--threshold auto|<float>] [--windows 3] [--reps 2] [--fp16]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from enerf_amd import mesh, scene  # noqa: E402
from enerf_amd.network import NeRFNetwork  # noqa: E402
from enerf_amd.trainer import TrainHarness  # noqa: E402

DEV = "cuda"


def _teacher(ro, rd):
    b_ = (ro * rd).sum(-1)
    disc = b_ ** 2 - ((ro * ro).sum(-1) - 0.36)
    hit = disc > 0
    t = -b_ - torch.sqrt(disc.clamp(min=0))
    p = ro + rd * t.unsqueeze(-1)
    return torch.where(hit.unsqueeze(-1), scene.analytic_color(p).clamp(0, 1), torch.ones_like(p))


def trained_harness(fp16, steps):
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=False, out_dim_color=3).to(DEV)
    h = TrainHarness(model, lr=1e-2, fp16=fp16)
    g = np.random.default_rng(0)
    for i in range(steps):
        v = g.normal(size=(4096, 3))
        o = 3.0 * v / np.linalg.norm(v, axis=1, keepdims=True)
        d = g.uniform(-0.8, 0.8, (4096, 3)) - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        ro, rd = (torch.tensor(a, dtype=torch.float32, device=DEV) for a in (o, d))
        h.step_rgb(ro, rd, _teacher(ro, rd), num_steps=128, upsample_steps=0, out_dim_color=3)
    torch.cuda.synchronize()
    return h


def reference_procedure(h, R, thr, path):
    """extract_fields + extract_geometry + export as the reference runs them (host blocks, host marching cubes)."""
    model = h.model
    box = model.aabb_infer.cpu().numpy()
    lo, hi = [float(v) for v in box[:3]], [float(v) for v in box[3:]]
    S = 128
    X, Y, Z = (list(torch.linspace(lo[a], hi[a], R).split(S)) for a in range(3))
    u = np.zeros([R, R, R], dtype=np.float32)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=bool(h.strat_f16)):
        for xi, xs in enumerate(X):
            for yi, ys in enumerate(Y):
                for zi, zs in enumerate(Z):
                    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                    pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                    val = model.density(pts.to(DEV))["sigma"].reshape(len(xs), len(ys), len(zs)).detach().cpu().numpy()
                    u[xi * S: xi * S + len(xs), yi * S: yi * S + len(ys), zi * S: zi * S + len(zs)] = val
    v, f = mesh.marching_cubes_statement(torch.from_numpy(u), thr)
    mesh.write_ply(path, mesh.to_world(v, R, box[:3], box[3:]), f)
    return int(f.shape[0])


def native_split(h, R, thr, path):
    """save_mesh's three parts timed apart (same calls as harness_save_mesh)."""
    model = h.model
    box = model.aabb_infer.cpu().numpy()
    prev = h._amp_scope() if (h.strat_f16 or h.amp_f16) else None
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        u = mesh.density_field(model, R, box[:3], box[3:])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        v, f = mesh.marching_cubes(u, thr)
        v = mesh.to_world(v, R, box[:3], box[3:])
        torch.cuda.synchronize()
        t2 = time.perf_counter()
    finally:
        if prev is not None:
            h._amp_restore(prev)
    mesh.write_ply(path, v, f)
    t3 = time.perf_counter()
    return {"field_ms": (t1 - t0) * 1e3, "mc_ms": (t2 - t1) * 1e3, "ply_ms": (t3 - t2) * 1e3,
            "vertices": int(v.shape[0]), "triangles": int(f.shape[0])}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--threshold", default="auto")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--train", type=int, default=100)
    ap.add_argument("--fp16", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh.py needs a GPU")
    R = a.resolution
    h = trained_harness(a.fp16, a.train)
    box = h.model.aabb_infer.cpu().numpy()
    if a.threshold == "auto":                # the reference's 10 when the short training reached it, else the 99th pct
        u = mesh.density_field(h.model, R, box[:3], box[3:])
        thr = 10.0 if float((u > 10).float().mean()) > 1e-4 else float(torch.quantile(u.view(-1)[::97].float(), 0.99))
        del u
    else:
        thr = float(a.threshold)
    lines = []

    def emit(d):
        d = dict(d, resolution=R, threshold=thr, fp16=bool(a.fp16))
        print(json.dumps(d), flush=True)
        lines.append(d)

    with tempfile.TemporaryDirectory() as tmp:
        pn, pr = os.path.join(tmp, "native.ply"), os.path.join(tmp, "reference.ply")
        h.save_mesh(pn, R, thr)                                  # warm-up of both arms
        reference_procedure(h, R, thr, pr)
        nat, ref = [], []
        for w in range(a.windows):
            arms = [("native", lambda: h.save_mesh(pn, R, thr)), ("reference", lambda: reference_procedure(h, R, thr, pr))]
            if w % 2:
                arms.reverse()
            for name, fn in arms:
                ts = [timed(fn)[0] for _ in range(a.reps)]
                (nat if name == "native" else ref).extend(ts)
                emit({"arm": name, "window": w, "ms": ts})
            emit(dict(native_split(h, R, thr, pn), arm="native_split", window=w))
        same = open(pn, "rb").read() == open(pr, "rb").read()
    emit({"summary": True, "native_ms_median": float(np.median(nat)), "reference_ms_median": float(np.median(ref)),
          "speedup": float(np.median(ref) / np.median(nat)), "ply_bytes_identical": same,
          "device": torch.cuda.get_device_name(0)})
    if a.out:
        with open(a.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
