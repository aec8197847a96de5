"""TrainHarness.evaluate's pieces on one GPU at the eds00 val set's shape (V = 54 views of 640 x 480), C = 1 and 3, RGB and
event-only mode:

  render      model.render of one 640 x 480 view as evaluate calls it (staged, num_steps 512, upsample_steps 0,
              max_ray_batch 4096, bg_color 1) on a cuda_ray = False NeRFNetwork (bound 1), fp32; per view
  kernels     enerf_eval_stats / _correct / _ssim (with their reduction passes), each timed alone with hip events over
              all V views; and evaluate.metrics as called (the three plus the one read-back), host clock
  reference   the reference's procedure on copies: every view copied to the host, compute_pnsr in numpy fp32, SSIM as
              the scipy fp64 uniform_filter statement (skimage's stand-in), and for event-only the normal equations in
              numpy over all views, exp and the corrected metrics; host clock

One JSON line per measurement; the per-view times divide by V.  Kernel traffic: bytes each kernel must move per pixel
(fp32 loads and stores), divided by the time, against the 8 TB/s HBM peak.

    python tools/bench_eval.py [--views 54] [--reps 5] [--render-views 3] [--ref-views 54]
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
from enerf_amd import _lib as L, evaluate as E  # noqa: E402
from enerf_amd.network import NeRFNetwork  # noqa: E402

DEV = "cuda"
H, W = 480, 640
PEAK = 8.0e12


def emit(**kw):
    print(json.dumps(kw), flush=True)


def data(V, C, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(V, H, W, C, device=DEV, generator=g) * 1.1, torch.rand(V, H, W, C, device=DEV, generator=g)


def ev_time(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts))


def kernels(V, C, event_only, reps):
    pred, gt = data(V, C, 1 + C)
    lib, s = L.lib(), L.stream_handle()
    ws = E._workspace(V, H, W, pred.device)
    out = torch.zeros(V * E.COLS + 2, dtype=torch.float64, device=DEV)
    res, ab = out.data_ptr(), out.data_ptr() + V * E.COLS * 8
    pc, gj = torch.empty(V, H, W, device=DEV), torch.empty(V, H, W, device=DEV)
    px = V * H * W
    runs = {"stats": (lambda: L.check(lib.enerf_eval_stats(pred.data_ptr(), gt.data_ptr(), V, H, W, C, int(event_only),
                                                           ws.data_ptr(), res, s), "stats"), 8 * C)}
    if event_only:
        runs["correct"] = (lambda: L.check(lib.enerf_eval_correct(pred.data_ptr(), gt.data_ptr(), V, H, W, C, ws.data_ptr(),
                                                                  res, ab, pc.data_ptr(), gj.data_ptr(), s), "correct"),
                           8 * C + 8)
        runs["ssim"] = (lambda: L.check(lib.enerf_eval_ssim(gj.data_ptr(), pc.data_ptr(), V, H, W, 1, 255.0, ws.data_ptr(),
                                                            res, s), "ssim"), 8)
    else:
        # channel 0 at a pixel stride of C: the loads touch whole 64-byte lines, so C = 3 moves the full 12 bytes a pixel
        runs["ssim"] = (lambda: L.check(lib.enerf_eval_ssim(gt.data_ptr(), pred.data_ptr(), V, H, W, C, 1.0,
                                                            ws.data_ptr(), res, s), "ssim"), 8 * C)
    for name, (fn, bpp) in runs.items():
        fn()
        t = ev_time(fn, reps)
        emit(what="kernel", kernel=name, C=C, event_only=event_only, V=V, ms=t * 1e3, ms_per_view=t * 1e3 / V,
             bytes_per_pixel=bpp, TBps=bpp * px / t / 1e12, frac_of_peak=bpp * px / t / PEAK)
    E.metrics(pred, gt, event_only)
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        E.metrics(pred, gt, event_only)
        ts.append(time.perf_counter() - t0)
    t = float(np.median(ts))
    emit(what="metrics", C=C, event_only=event_only, V=V, ms=t * 1e3, ms_per_view=t * 1e3 / V)
    return pred, gt


def compute_pnsr(img0, img1, max_val):
    return -10 * np.log10(np.mean(np.power(img0.astype(np.float32) - img1.astype(np.float32), 2))) + 20 * np.log10(max_val)


def ssim_fp64(a, b, data_range):
    from scipy.ndimage import uniform_filter
    X, Y = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ux, uy = uniform_filter(X, 7), uniform_filter(Y, 7)
    uxx, uyy, uxy = uniform_filter(X * X, 7), uniform_filter(Y * Y, 7), uniform_filter(X * Y, 7)
    vx, vy, vxy = (49 / 48) * (uxx - ux * ux), (49 / 48) * (uyy - uy * uy), (49 / 48) * (uxy - ux * uy)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    S = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
    return S[3:-3, 3:-3].mean()


def reference(pred, gt, event_only, nviews):
    """The reference's host procedure (nerf/utils.py:1088-1215) on `nviews` views, host clock."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if not event_only:
        for j in range(nviews):
            g, p = gt[j].cpu().numpy(), pred[j].cpu().numpy()
            compute_pnsr(g, p, 1)
            ssim_fp64(g[..., 0], p[..., 0], 1)
    else:
        C = pred.shape[-1]
        logs = [E.log_images(pred[j:j + 1])[0] for j in range(nviews)]
        glogs = [E.log_images(gt[j:j + 1])[0] for j in range(nviews)]
        x, y = torch.stack(logs).cpu().numpy().ravel(), torch.stack(glogs).cpu().numpy().ravel()
        X = np.ones((x.size, 2))
        X[:, 1] = x
        beta = np.linalg.inv(X.T @ X) @ X.T @ y
        a, b = beta[1], beta[0]
        for j in range(nviews):
            pc = torch.exp(logs[j] * a + b).cpu()
            g = 255. * gt[j].cpu()
            gj = E.rgb_to_luma(g) if C == 3 else g[..., 0]
            compute_pnsr(gj.numpy(), pc.numpy(), 255)
            ssim_fp64(gj.numpy(), pc.numpy(), 255)
    return time.perf_counter() - t0


def render(nviews, reps):
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=1, cuda_ray=False, out_dim_color=3).to(DEV).eval()
    g = np.random.default_rng(0)
    rays = []
    for _ in range(nviews):
        o = torch.tensor([0.0, 0.0, 1.5], device=DEV) + torch.tensor(g.uniform(-0.2, 0.2, 3), dtype=torch.float32, device=DEV)
        v, u = torch.meshgrid(torch.linspace(-0.3, 0.3, H, device=DEV), torch.linspace(-0.4, 0.4, W, device=DEV),
                              indexing="ij")
        d = torch.stack([u, v, -torch.ones_like(u)], -1).reshape(1, H * W, 3)
        rays.append((o.reshape(1, 1, 3).expand(1, H * W, 3).contiguous(), (d / d.norm(dim=-1, keepdim=True)).contiguous()))
    kw = dict(E.RENDER_DEFAULTS, out_dim_color=3)
    with torch.no_grad():
        model.render(*rays[0], staged=True, bg_color=1, perturb=False, **kw)
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for ro, rd in rays:
                model.render(ro, rd, staged=True, bg_color=1, perturb=False, **kw)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / nviews)
    t = float(np.median(ts))
    emit(what="render", H=H, W=W, num_steps=512, ms_per_view=t * 1e3)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=54)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--render-views", type=int, default=3)
    ap.add_argument("--ref-views", type=int, default=54)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    emit(what="device", name=torch.cuda.get_device_name(0), torch=torch.__version__)
    t_render = render(a.render_views, max(1, a.reps // 2))
    summary = {"render_ms_per_view": t_render * 1e3}
    for C in (1, 3):
        for event_only in (False, True):
            pred, gt = kernels(a.views, C, event_only, a.reps)
            n = min(a.ref_views, a.views)
            t = reference(pred, gt, event_only, n)
            emit(what="reference", C=C, event_only=event_only, V=n, ms=t * 1e3, ms_per_view=t * 1e3 / n)
            summary[f"reference_ms_per_view_C{C}_{'ev' if event_only else 'rgb'}"] = t * 1e3 / n
            del pred, gt
            torch.cuda.empty_cache()
    emit(what="summary", **summary)


if __name__ == "__main__":
    main()
