"""Held-out evaluation: the reference's `Trainer.evaluate` / `evaluate_one_epoch` (nerf/utils.py:44-92, 763-766,
1028-1293) for `TrainHarness.evaluate`, with the metrics in HIP (csrc/eval_metrics.hip) and no skimage / cv2.

    render_views(harness, views, opt)        the reference's eval_step / eval_step_tumvie for every view, into one buffer
    metrics(pred, gt, event_only)            per-view SSE, SSIM and, event-only, the log-affine correction
    harness_evaluate(harness, views, ...)    the two strung together, the result dict, the validation/ files

Semantics, the same on every path; V views of H x W pixels, C = out_dim_color (1 or 3):
  * per-view MSE = SSE / (H W C), SSE = sum of (pred - gt)^2 with the difference in fp32 and the sum in fp64; pred is the
    unclipped render, gt the view's image (alpha composited on white for C + 1 channels; srgb_to_linear for
    color_space = "linear").  valid_loss = the mean over views of the MSE; psnr_meter = the mean of -10 log10(MSE)
    (PSNRMeter, :252-287).
  * RGB mode: psnr = -10 log10(MSE) per view (compute_pnsr at max_val 1, :89-92, :1096); ssim = SSIM(gt[..., 0],
    pred[..., 0]) at data_range 1 (:1110).
  * SSIM: skimage's structural_similarity defaults on one plane: 7 x 7 uniform window, sample covariance (x 49/48),
    K1 = 0.01, K2 = 0.03, S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), averaged over the
    (H - 6) x (W - 6) interior (the 3-pixel border is cropped, so the filter's boundary mode never matters), in fp64.
  * Event-only mode (:1166-1240): x = log(255 l(pred) + 1e-3), y = log(255 l(gt) + 1e-3) in fp32, l = the pixel (C = 1)
    or rgb_to_luma's esim weights (C = 3), rgb view only.  a, b: least squares of y on [1, x] over all views' pixels in
    fp64, closed form of the 2 x 2 normal equations; a NaN becomes 5.  pred_cor = exp(a x + b) in fp32 (a and b rounded
    to fp32, two roundings), unclipped; gt_j = l(255 gt).  psnr_corrected = -10 log10(MSE(gt_j, pred_cor)) +
    20 log10(255); ssim_corrected = SSIM(gt_j, pred_cor) at data_range 255.
Deviations from the reference: the dB numbers are computed in fp64 from the fp64 SSE (the reference's numpy works in
fp32); with `eval_stereo_views` the reference's PSNRMeter is also fed (event-view pred, itself), whose PSNR is +inf --
psnr_meter here covers the rgb views only; with color_space = "linear" and stereo views, the reference converts the gt a
second time in place (eval_step_tumvie) -- here it is converted once; no LPIPS (no weights on these machines).

On CUDA tensors `metrics` runs the library's kernels: three launches (plus their fixed-order reduction passes) and one
device-to-host read of the per-view results.  The torch statements `stats_statement`, `fit_statement`,
`correct_statement` and `ssim_statement` are the CPU path and the reference the GPU tests hold the kernels to.
"""
import ctypes
import math
import os
import struct
import zlib

import numpy as np
import torch

from . import _lib as L

COLS = 7                        # include/enerf_hip.h ENERF_EVAL_COLS: sse, sx, sy, sxx, sxy, sse_cor, ssim
COL_SSE_COR, COL_SSIM = 5, 6
WIN = 7
LUMA = (0.299, 0.587, 0.114)    # utils/event_utils.py rgb_to_luma, esim weights
RENDER_DEFAULTS = {"num_steps": 512, "upsample_steps": 0, "max_ray_batch": 4096}   # main_nerf.py's CLI defaults


def srgb_to_linear(x):
    return torch.where(x < 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


def linear_to_srgb(x):
    return torch.where(x < 0.0031308, 12.92 * x, 1.055 * x ** 0.41666 - 0.055)


def rgb_to_luma(rgb):
    """[..., 3] -> [...]: the esim weights in fp32, summed left to right."""
    f = torch.tensor(LUMA, dtype=torch.float32, device=rgb.device)
    p = rgb * f
    return (p[..., 0] + p[..., 1]) + p[..., 2]


def _check(pred, gt):
    if pred.dim() != 4 or pred.shape != gt.shape:
        raise ValueError(f"pred {tuple(pred.shape)} / gt {tuple(gt.shape)}: two [V, H, W, C] tensors expected")
    if pred.dtype != torch.float32 or gt.dtype != torch.float32:
        raise ValueError(f"pred {pred.dtype} / gt {gt.dtype}: float32 expected")
    V, H, W, C = pred.shape
    if C not in (1, 3):
        raise ValueError(f"{C} channels: 1 or 3 expected")
    if H < WIN or W < WIN:
        raise ValueError(f"{H} x {W} views: SSIM's 7 x 7 window needs at least 7 x 7")
    return V, H, W, C


# ------------------------------------------------------------------------------------------------------ statement
def log_images(img):
    """[V, H, W, C] in [0, 1] -> log(255 l(img) + 1e-3) [V, H, W] fp32."""
    lum = rgb_to_luma(img) if img.shape[-1] == 3 else img[..., 0]
    return torch.log(255 * lum + 1e-3)


def stats_statement(pred, gt, log_mode):
    """-> res [V, COLS] fp64 on pred's device: column 0 the SSE, columns 1..4 (log_mode) the sums of x, y, x^2, xy."""
    V = pred.shape[0]
    res = torch.zeros(V, COLS, dtype=torch.float64, device=pred.device)
    res[:, 0] = (pred - gt).double().pow(2).reshape(V, -1).sum(1)
    if log_mode:
        x, y = log_images(pred).double().reshape(V, -1), log_images(gt).double().reshape(V, -1)
        res[:, 1], res[:, 2], res[:, 3], res[:, 4] = x.sum(1), y.sum(1), (x * x).sum(1), (x * y).sum(1)
    return res


def fit_statement(res, n):
    """solve_normal_equations (:44-71) from the per-view sums: the 2 x 2 normal equations over all n pixels, closed
    form, fp64 -> (a, b) Python floats; a NaN becomes 5."""
    sx, sy, sxx, sxy = (float(v) for v in res[:, 1:5].double().cpu().numpy().sum(0))
    n = float(n)
    with np.errstate(all="ignore"):
        det = np.float64(n) * sxx - np.float64(sx) * sx
        b = (np.float64(sxx) * sy - np.float64(sx) * sxy) / det
        a = (np.float64(n) * sxy - np.float64(sx) * sy) / det
    return (5.0 if math.isnan(a) else float(a)), (5.0 if math.isnan(b) else float(b))


def correct_statement(pred, gt, a, b):
    """-> pred_cor = exp(a x + b), gt_j = l(255 gt) [V, H, W] fp32 and their SSE [V] fp64."""
    pred_cor = torch.exp(log_images(pred) * a + b)
    g = 255. * gt
    gt_j = rgb_to_luma(g) if gt.shape[-1] == 3 else g[..., 0]
    sse = (gt_j - pred_cor).double().pow(2).reshape(gt.shape[0], -1).sum(1)
    return pred_cor, gt_j, sse


def ssim_statement(x, y, data_range):
    """skimage.metrics.structural_similarity's defaults on planes x, y [V, H, W] -> mean SSIM [V] fp64."""
    X, Y = x.double()[:, None], y.double()[:, None]
    NP = WIN * WIN

    def box(t):
        return torch.nn.functional.avg_pool2d(t, WIN, stride=1)       # the interior's 7 x 7 means

    ux, uy, uxx, uyy, uxy = box(X), box(Y), box(X * X), box(Y * Y), box(X * Y)
    cov = NP / (NP - 1)
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    S = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return S.reshape(S.shape[0], -1).mean(1)


def _metrics_statement(pred, gt, event_only):
    V, H, W, C = _check(pred, gt)
    res = stats_statement(pred, gt, event_only)
    out = {"sse": res[:, 0].cpu().numpy()}
    if event_only:
        a, b = fit_statement(res, V * H * W)
        pred_cor, gt_j, sse = correct_statement(pred, gt, a, b)
        out.update(a=a, b=b, sse_cor=sse.cpu().numpy(), ssim=ssim_statement(gt_j, pred_cor, 255).cpu().numpy(),
                   pred_cor=pred_cor, gt_j=gt_j)
    else:
        out["ssim"] = ssim_statement(gt[..., 0], pred[..., 0], 1).cpu().numpy()
    return out


# --------------------------------------------------------------------------------------------------------- native
def _workspace(V, H, W, dev):
    n = ctypes.c_uint64(0)
    L.check(L.lib().enerf_eval_workspace(V, H, W, ctypes.byref(n)), "eval_workspace")
    return torch.empty(int(n.value), dtype=torch.uint8, device=dev)


def _metrics_native(pred, gt, event_only):
    V, H, W, C = _check(pred, gt)
    pred, gt = pred.contiguous(), gt.contiguous()
    lib, s, dev = L.lib(), L.stream_handle(), pred.device
    ws = _workspace(V, H, W, dev)
    out = torch.zeros(V * COLS + 2, dtype=torch.float64, device=dev)      # res [V, COLS], then a, b
    res, ab = out.data_ptr(), out.data_ptr() + V * COLS * 8
    L.check(lib.enerf_eval_stats(pred.data_ptr(), gt.data_ptr(), V, H, W, C, int(event_only), ws.data_ptr(), res, s),
            "eval_stats")
    planes = {}
    if event_only:
        pred_cor = torch.empty(V, H, W, dtype=torch.float32, device=dev)
        gt_j = torch.empty_like(pred_cor)
        L.check(lib.enerf_eval_correct(pred.data_ptr(), gt.data_ptr(), V, H, W, C, ws.data_ptr(), res, ab,
                                       pred_cor.data_ptr(), gt_j.data_ptr(), s), "eval_correct")
        L.check(lib.enerf_eval_ssim(gt_j.data_ptr(), pred_cor.data_ptr(), V, H, W, 1, 255.0, ws.data_ptr(), res, s),
                "eval_ssim")
        planes = {"pred_cor": pred_cor, "gt_j": gt_j}
    else:
        L.check(lib.enerf_eval_ssim(gt.data_ptr(), pred.data_ptr(), V, H, W, C, 1.0, ws.data_ptr(), res, s),
                "eval_ssim")
    host = out.cpu().numpy()                                   # the one read-back: 8 (V COLS + 2) bytes
    r = host[:V * COLS].reshape(V, COLS)
    o = {"sse": r[:, 0].copy(), "ssim": r[:, COL_SSIM].copy(), "res": r, **planes}
    if event_only:
        o.update(a=float(host[-2]), b=float(host[-1]), sse_cor=r[:, COL_SSE_COR].copy())
    return o


def metrics(pred, gt, event_only):
    """pred, gt [V, H, W, C] fp32 (C = 1 or 3) -> {"sse": [V], "ssim": [V]} (numpy fp64) and, event_only, "a", "b",
    "sse_cor" [V] and the planes "pred_cor", "gt_j" [V, H, W] fp32 (on pred's device); "ssim" is then the corrected
    SSIM.  CUDA tensors take the HIP kernels (and add "res", the [V, COLS] per-view results as read back), CPU tensors
    the torch statement."""
    if pred.is_cuda:
        return _metrics_native(pred, gt, event_only)
    return _metrics_statement(pred, gt, event_only)


def summarize(m, H, W, C, event_only):
    """The result dict of TrainHarness.evaluate from metrics' output."""
    mse = m["sse"] / float(H * W * C)
    with np.errstate(divide="ignore"):
        psnr = -10.0 * np.log10(mse)
    r = {"valid_loss": float(mse.mean()), "psnr_meter": float(psnr.mean()), "views": int(len(mse))}
    if event_only:
        with np.errstate(divide="ignore"):
            pc = -10.0 * np.log10(m["sse_cor"] / float(H * W)) + 20.0 * math.log10(255.0)
        r.update(a=m["a"], b=m["b"], psnr_corrected=[float(v) for v in pc], ssim_corrected=[float(v) for v in m["ssim"]],
                 psnr_corrected_mean=float(pc.mean()), ssim_corrected_mean=float(m["ssim"].mean()))
    else:
        r.update(psnr=[float(v) for v in psnr], ssim=[float(v) for v in m["ssim"]], psnr_mean=float(psnr.mean()),
                 ssim_mean=float(m["ssim"].mean()))
    return r


# --------------------------------------------------------------------------------------------------------- render
def _opt(opt, name, default):
    return getattr(opt, name, default) if opt is not None else default


def _stereo(opt):
    return _opt(opt, "mode", None) in ("tumvie", "eds") and bool(_opt(opt, "eval_stereo_views", 0))


def render_kwargs(opt):
    """What reaches model.render besides the eval_step's own: the CLI defaults, out_dim_color (the reference passes
    vars(opt)), then opt.render_kwargs."""
    kw = dict(RENDER_DEFAULTS, out_dim_color=int(_opt(opt, "out_dim_color", 3)))
    kw.update(_opt(opt, "render_kwargs", None) or {})
    return kw


def _gt(images, C, linear):
    """eval_step's gt: [1, H, W, C'] -> [H, W, C] fp32 (srgb_to_linear first for color_space = "linear", alpha
    composited on the background 1 when C' = C + 1)."""
    img = images[0].float()
    if linear:
        img = img.clone()
        img[..., :C] = srgb_to_linear(img[..., :C])
    if img.shape[-1] == C + 1:
        img = img[..., :C] * img[..., C:] + 1 * (1 - img[..., C:])
    if img.shape[-1] != C:
        raise ValueError(f"images with {img.shape[-1]} channels for out_dim_color = {C}")
    return img


def _render(model, rays_o, rays_d, H, W, C, kw):
    out = model.render(rays_o, rays_d, staged=True, bg_color=1, perturb=False, **kw)
    return out["image"].reshape(H, W, C), out["depth"].reshape(H, W)


@torch.no_grad()
def render_views(harness, views, opt):
    """The reference's eval_step (and eval_step_tumvie for mode tumvie / eds with eval_stereo_views) over `views`, in
    the harness's regime -> (pred [V, H, W, C], gt [V, H, W, C], depth [V, H, W]) on the model's device, and the event
    views' (pred, depth) lists (empty without stereo)."""
    model = harness.model
    dev = next(model.parameters()).device
    C = int(_opt(opt, "out_dim_color", 3))
    linear = _opt(opt, "color_space", "srgb") == "linear"
    stereo = _stereo(opt)
    kw = render_kwargs(opt)
    views = list(views)
    if not views:
        raise ValueError("evaluate: no views")
    H, W = int(views[0]["H"]), int(views[0]["W"])
    V = len(views)
    pred = torch.empty(V, H, W, C, dtype=torch.float32, device=dev)
    gt = torch.empty_like(pred)
    depth = torch.empty(V, H, W, dtype=torch.float32, device=dev)
    ev = []
    for i, data in enumerate(views):
        if (int(data["H"]), int(data["W"])) != (H, W):
            raise ValueError(f"view {i}: {data['H']} x {data['W']}, the first was {H} x {W}")
        ro, rd = data["rays_o"].to(dev), data["rays_d"].to(dev)
        img, dep = _render(model, ro, rd, H, W, C, kw)
        pred[i], depth[i] = img, dep
        gt[i] = _gt(data["images"].to(dev), C, linear)
        if stereo:
            He, We = int(data.get("H_ev", H)), int(data.get("W_ev", W))
            ev.append(_render(model, data["rays_evs_o"].to(dev), data["rays_evs_d"].to(dev), He, We, C, kw))
    return pred, gt, depth, ev


def _in_regime(harness, fn):
    """mesh.harness_save_mesh's choice: precision 3 for the fp16 regimes, autocast for the autocast route."""
    if harness.strat_f16 or harness.amp_f16:
        prev = harness._amp_scope()
        try:
            return fn()
        finally:
            harness._amp_restore(prev)
    if harness.fp16:
        with torch.autocast("cuda", dtype=torch.float16):
            return fn()
    return fn()


# ---------------------------------------------------------------------------------------------------------- files
def write_png(path, img):
    """8-bit grey ([H, W] / [H, W, 1]) or RGB ([H, W, 3]) PNG with the standard library's zlib."""
    a = np.ascontiguousarray(np.asarray(img, dtype=np.uint8))
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[..., 0]
    if a.ndim == 2:
        ctype = 0
    elif a.ndim == 3 and a.shape[2] == 3:
        ctype = 2
    else:
        raise ValueError(f"write_png: image of shape {a.shape}")
    H, W = a.shape[:2]
    raw = np.concatenate([np.zeros((H, 1), np.uint8), a.reshape(H, -1)], axis=1).tobytes()   # filter 0 on every row

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    png = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, ctype, 0, 0, 0)) \
        + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(png)
    return path


def read_png(path):
    """Parser of what write_png writes (8-bit, grey or RGB, filter 0) -> uint8 [H, W] or [H, W, 3]."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    W, H, depth, ctype = head[:4]
    assert depth == 8 and ctype in (0, 2)
    ch = 3 if ctype == 2 else 1
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + W * ch)
    assert (rows[:, 0] == 0).all()
    img = rows[:, 1:].reshape(H, W, ch)
    return img[..., 0] if ch == 1 else img


def to_u8(x):
    """The reference's (x * 255).astype(uint8), clipped to [0, 255] first instead of wrapping."""
    return np.clip(np.asarray(x, np.float32) * 255, 0, 255).astype(np.uint8)


def corrected_u8(x):
    """The corrected image: clipped to [0, 255], then rint (:1229-1230)."""
    return np.rint(np.clip(np.asarray(x, np.float32), 0, 255)).astype(np.uint8)


def _save(save_dir, name, pred, gt, depth, ev, m, event_only, linear):
    val = os.path.join(save_dir, "validation")

    def path(*p):
        f = os.path.join(val, *p)
        os.makedirs(os.path.dirname(f), exist_ok=True)
        return f

    P, G, D = pred.cpu().numpy(), gt.cpu().numpy(), depth.cpu().numpy()
    Pc = m["pred_cor"].cpu().numpy() if event_only else None
    for j in range(P.shape[0]):
        tag = f"{name}_{j:04d}"
        np.save(path("raw", tag + ".npy"), P[j])
        write_png(path("depth", tag + "_depth.png"), to_u8(D[j]))
        write_png(path("gt", tag + "_gt.png"), to_u8(G[j]))
        if event_only:
            write_png(path("prediction_corrected", tag + ".png"), corrected_u8(Pc[j]))
        else:
            shown = linear_to_srgb(pred[j]).cpu().numpy() if linear else P[j]
            write_png(path("prediction", tag + ".png"), to_u8(shown))
        if ev:
            ep, ed = ev[j]
            epn = ep.cpu().numpy()
            np.save(path("event_view", "raw", tag + ".npy"), epn)
            write_png(path("event_view", "depth_ev", tag + "_depth.png"), to_u8(ed.cpu().numpy()))
            if event_only:
                lum = rgb_to_luma(ep) if ep.shape[-1] == 3 else ep[..., 0]
                cor = torch.exp(torch.log(255 * lum + 1e-9) * m["a"] + m["b"])        # (:1185-1187, 1e-9 there)
                write_png(path("event_view", "prediction_corrected_ev", tag + ".png"), corrected_u8(cor.cpu().numpy()))
            else:
                write_png(path("event_view", "prediction_ev", tag + ".png"), to_u8(epn))
                write_png(path("event_view", "warped_gt_ev", tag + "_gt.png"), to_u8(epn))


# ----------------------------------------------------------------------------------------------------- entry point
def harness_evaluate(harness, views, opt, name="eval", save_dir=None, ema=None):
    """TrainHarness.evaluate: render every view under model.eval() (and the EMA's weights when given) in the harness's
    regime, the metrics of the module docstring, the files of the reference's validation/ tree under save_dir (rank 0
    only).  The previous training mode is restored, and the EMA's store / copy_to / restore bracket the renders."""
    import torch.distributed as dist
    model = harness.model
    event_only = bool(_opt(opt, "event_only", False))
    C = int(_opt(opt, "out_dim_color", 3))
    linear = _opt(opt, "color_space", "srgb") == "linear"
    was_training = model.training
    model.eval()
    if ema is not None:
        ema.store()
        ema.copy_to()
    try:
        with torch.no_grad():
            pred, gt, depth, ev = _in_regime(harness, lambda: render_views(harness, views, opt))
            m = metrics(pred, gt, event_only)
    finally:
        if ema is not None:
            ema.restore()
        model.train(was_training)
    V, H, W, _ = pred.shape
    r = summarize(m, H, W, C, event_only)
    rank0 = not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0
    if save_dir is not None and rank0:
        with torch.no_grad():
            _save(save_dir, name, pred, gt, depth, ev, m, event_only, linear)
    return r
