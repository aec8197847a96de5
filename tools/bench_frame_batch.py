"""One frame batch on one GPU at 640 x 480 (V = 8 views, 3-channel images): FrameSampler.batch (csrc/frame_batch.hip)
beside the torch statement of the reference's collate on the same GPU.

  sampler     FrameSampler.batch: the draw(s) + enerf_frame_batch, with the error map + enerf_error_map_sample;
              uniform at N = 4096 and N = 20096, error map at N = 4096
  kernels     the launches alone, from given draws (what the sampler adds to the draws)
  statement   events.get_rays (the reference's get_rays without its error_map branch: two linspace, a meshgrid, two
              H*W-sized expand / gather, the element-wise chain, norm, matmul) + the image's copy and stacked gather of
              provider.py:1076-1079; for the error map, torch.multinomial(replacement=False) and the pixel mapping of
              get_rays lines 142-149 in front of it

Each is timed twice over `--reps` repetitions after a warm-up: device time between two events around the repetitions,
and the host's enqueue time (the clock around the same loop before the device is waited for).  One JSON line each.

    python tools/bench_frame_batch.py [--reps 200]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from enerf_amd import events, frame_sampler as F, scene  # noqa: E402

DEV = "cuda"
H, W, V, CI = scene.H, scene.W, 8, 3


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps, host * 1e6 / reps          # microseconds per repetition


def statement_batch(poses, images, error_map, v, N):
    """The reference's collate, frame side, in torch on the device."""
    if error_map is None:
        rays = events.get_rays(poses[v:v + 1], scene.INTRINSICS, H, W, N)
    else:
        coarse = torch.multinomial(error_map[v:v + 1], N, replacement=False)
        ix, iy = coarse // 128, coarse % 128
        sx, sy = H / 128, W / 128
        ix = (ix * sx + torch.rand(1, N, device=DEV) * sx).long().clamp(max=H - 1)
        iy = (iy * sy + torch.rand(1, N, device=DEV) * sy).long().clamp(max=W - 1)
        rays = events.get_rays(poses[v:v + 1], scene.INTRINSICS, H, W, N, inds=(ix * W + iy)[0])
        rays["inds_coarse"] = coarse
    im = images[[v]]
    rays["images"] = torch.gather(im.view(1, -1, CI), 1, torch.stack(CI * [rays["inds"]], -1))
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    emit(what="device", name=torch.cuda.get_device_name(0), torch=torch.__version__, H=H, W=W, V=V, Ci=CI)
    g = torch.Generator(device=DEV).manual_seed(0)
    poses = torch.stack([scene.pose(k) for k in range(V)]).to(DEV)
    images = torch.rand(V, H, W, CI, device=DEV, generator=g)
    emap = torch.rand(V, F.CELLS, device=DEV, generator=g) + 0.01
    for mode, N in (("uniform", 4096), ("uniform", 20096), ("error_map", 4096)):
        s = F.FrameSampler(poses, scene.INTRINSICS, H, W, images=images, num_rays=N, error_map=mode == "error_map")
        if s.error_map is not None:
            s.error_map.copy_(emap)
        dev_us, host_us = timed(lambda: s.batch([3], generator=g), a.reps)
        emit(what="sampler", mode=mode, N=N, device_us=dev_us, host_us=host_us)
        if mode == "uniform":
            inds = torch.randint(0, H * W, [N], device=DEV, generator=g)
            k_dev, k_host = timed(lambda: F.frame_batch(poses, 3, scene.INTRINSICS, H, W, inds, images), a.reps)
        else:
            e = torch.empty(F.CELLS, device=DEV).exponential_(generator=g)
            u, w = torch.rand(N, device=DEV, generator=g), torch.rand(N, device=DEV, generator=g)

            def both():
                _, inds = F.error_map_sample(emap[3], e, u, w, H, W)
                F.frame_batch(poses, 3, scene.INTRINSICS, H, W, inds, images)
            k_dev, k_host = timed(both, a.reps)
            s_dev, _ = timed(lambda: F.error_map_sample(emap[3], e, u, w, H, W), a.reps)
            emit(what="kernel", kernel="error_map_sample", N=N, device_us=s_dev)
        emit(what="kernels", mode=mode, N=N, device_us=k_dev, host_us=k_host)
        st_dev, st_host = timed(lambda: statement_batch(poses, images, s.error_map, 3, N), a.reps)
        emit(what="statement", mode=mode, N=N, device_us=st_dev, host_us=st_host)


if __name__ == "__main__":
    main()
