"""TrainHarness.test and ViewRenderer on one GPU at the shipped shape: 640 x 480 views, `cuda_ray` off, num_steps 512,
upsample_steps 0, max_ray_batch 5096, color_space "linear", C = 1 and 3.

Per C, `--rounds` rounds; within a round the variants alternate (their order rotates from round to round), each over the
same `--views` views, after one warm-up pass:
    test_behind      TrainHarness.test(write_behind=True): render, ONE enerf_view_finish launch, PNG written behind the next
    test_sync        the same with write_behind=False: the copy's wait and the PNG encode between two renders
    reference        the reference's procedure restated in torch on the same GPU: render, linear_to_srgb on the device,
                     .cpu().numpy(), (x * 255).astype(uint8) on the host, synchronous write_png
    render_only      the renders alone (what none of them can go below)
each timed with the host clock around the whole call, which ends with the files written and the device drained: ms per
view.  Then, per C: the finish launch alone (device time between two events around `--reps` launches, 640 x 480 and the
320 x 240 -> 640 x 480 upsampling with the running mean) and ViewRenderer.frame beside the bare render of the same rays
at downscale 1 and 0.5 (host clock, drained; frame() restarts its count every call, so every call renders).  Every round is
one JSON line, appended to `--out` (profiles/test_views_bench.jsonl) and printed; a "median" line per variant closes each C.

    python tools/bench_test_views.py [--rounds 5] [--views 6] [--reps 200] [--out profiles/test_views_bench.jsonl]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from enerf_amd import evaluate as E  # noqa: E402
from enerf_amd import view  # noqa: E402
from enerf_amd.frame_sampler import FrameSampler  # noqa: E402

DEV = "cuda"
H, W = 480, 640
INTRINSICS = (500.0, 500.0, 320.0, 240.0)


def poses(n):
    """Cameras on a circle of radius 1.6 around the box, looking at its centre."""
    out = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    for k in range(n):
        a = 2 * np.pi * k / n
        c = np.array([1.6 * np.cos(a), 0.3, 1.6 * np.sin(a)])
        z = -c / np.linalg.norm(c)                          # get_rays looks along +z of the camera
        x = np.cross(np.array([0.0, 1.0, 0.0]), z)
        x /= np.linalg.norm(x)
        out[k, :3, :3] = np.stack([x, np.cross(z, x), z], 1)
        out[k, :3, 3] = c
    return out


def reference_procedure(harness, views, opt, save_path, C):
    """nerf/utils.py:768-804 as written there, with write_png for cv2.imwrite."""
    model = harness.model
    kw = E.render_kwargs(opt)
    os.makedirs(save_path, exist_ok=True)

    def loop():
        for i, data in enumerate(views):
            out = model.render(data["rays_o"], data["rays_d"], staged=True, bg_color=None, perturb=False, **kw)
            preds = out["image"].reshape(-1, H, W, C)
            preds = E.linear_to_srgb(preds)
            pred = preds[0].detach().cpu().numpy()
            E.write_png(os.path.join(save_path, f"ref_{i:04d}.png"), (pred * 255).astype(np.uint8))

    view._eval_scope(harness, loop)


def render_only(harness, views, opt):
    kw = E.render_kwargs(opt)
    view._eval_scope(harness, lambda: [harness.model.render(d["rays_o"], d["rays_d"], staged=True, bg_color=None,
                                                            perturb=False, **kw) for d in views])


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def device_us(fn, reps, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--num_steps", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "test_views_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_test_views: no GPU (this tool measures, it has no other mode)")
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="enerf_test_views_")
    with open(a.out, "a") as f:
        def emit(**kw):
            line = json.dumps(kw)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        emit(what="device", name=torch.cuda.get_device_name(0), torch=torch.__version__, H=H, W=W, views=a.views,
             num_steps=a.num_steps, max_ray_batch=5096)
        for C in (1, 3):
            torch.manual_seed(0)
            model = NeRFNetwork(encoding="hashgrid", bound=1, cuda_ray=False, out_dim_color=C).to(DEV)
            h = TrainHarness(model)
            opt = argparse.Namespace(out_dim_color=C, color_space="linear",
                                     render_kwargs={"num_steps": a.num_steps, "upsample_steps": 0, "max_ray_batch": 5096})
            sampler = FrameSampler(torch.from_numpy(poses(a.views)).to(DEV), INTRINSICS, H, W, num_rays=-1)
            views = [sampler.batch(i) for i in range(a.views)]
            variants = (
                ("test_behind", lambda: h.test(views, opt, os.path.join(tmp, "behind"), name="v", write_behind=True)),
                ("test_sync", lambda: h.test(views, opt, os.path.join(tmp, "sync"), name="v", write_behind=False)),
                ("reference", lambda: reference_procedure(h, views, opt, os.path.join(tmp, "ref"), C)),
                ("render_only", lambda: render_only(h, views, opt)),
            )
            for _, fn in variants:                              # warm-up: every shape of the timed window
                fn()
            per = {name: [] for name, _ in variants}
            for r in range(a.rounds):
                k = r % len(variants)                           # the order rotates: no variant keeps one position
                for name, fn in variants[k:] + variants[:k]:
                    ms = wall(fn) / a.views
                    per[name].append(ms)
                    emit(what="round", C=C, round=r, variant=name, ms_per_view=ms)
            for name, v in per.items():
                emit(what="median", C=C, variant=name, ms_per_view=statistics.median(v), min=min(v), max=max(v))
            # the written frames of the two test variants are the same files
            for i in range(a.views):
                x = open(os.path.join(tmp, "behind", f"v_{i:04d}.png"), "rb").read()
                assert x == open(os.path.join(tmp, "sync", f"v_{i:04d}.png"), "rb").read()
            # the finish launch alone
            img = torch.rand(H, W, C, device=DEV)
            dep = torch.rand(H, W, device=DEV)
            small, sdep = torch.rand(H // 2, W // 2, C, device=DEV), torch.rand(H // 2, W // 2, device=DEV)
            acc = torch.zeros(H, W, C, device=DEV)
            for name, fn in (
                    ("finish_test", lambda: view.finish(img, None, linear=True, outputs=("image_u8",))),
                    ("finish_frame_up2", lambda: view.finish(small, sdep, out_size=(H, W), linear=True, accum=acc, spp=3,
                                                             outputs=("image", "image_u8", "depth"))),
                    ("statement_test", lambda: view.finish_statement(img, None, linear=True, outputs=("image_u8",))),
                    ("statement_frame_up2", lambda: view.finish_statement(small, sdep, out_size=(H, W), linear=True,
                                                                          accum=acc, spp=3,
                                                                          outputs=("image", "image_u8", "depth")))):
                us = [device_us(fn, a.reps) for _ in range(3)]
                emit(what="finish", C=C, variant=name, device_us_median=statistics.median(us), device_us=us)
            # ViewRenderer.frame beside the bare render of the same rays
            kw = E.render_kwargs(opt)
            vr = view.ViewRenderer(h, H, W, INTRINSICS, opt)
            pose = poses(a.views)[0]
            for ds in (1.0, 0.5):
                rH, rW = int(H * ds), int(W * ds)
                s = FrameSampler(torch.from_numpy(pose[None]).to(DEV), tuple(x * ds for x in INTRINSICS), rH, rW,
                                 num_rays=-1)
                d = s.batch(0)

                def bare():
                    view._eval_scope(h, lambda: model.render(d["rays_o"], d["rays_d"], staged=True, bg_color=None,
                                                             perturb=1, **kw))

                def frame():
                    vr.reset()
                    vr.frame(pose, downscale=ds)
                bare(), frame()
                fr, br = [], []
                for r in range(a.rounds):
                    if r % 2:
                        fr.append(wall(frame))
                        br.append(wall(bare))
                    else:
                        br.append(wall(bare))
                        fr.append(wall(frame))
                    emit(what="frame_round", C=C, downscale=ds, round=r, bare_ms=br[-1], frame_ms=fr[-1])
                emit(what="frame_median", C=C, downscale=ds, bare_ms=statistics.median(br), frame_ms=statistics.median(fr),
                     overhead_ms=statistics.median(fr) - statistics.median(br))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
