"""Views without ground truth: the reference's `Trainer.test` (nerf/utils.py:695-709, 768-804), `Trainer.test_gui` with
the GUI's accumulation (:870-918, nerf/gui.py:119-149) and the path loop of scripts/render.py:489-509, for
`TrainHarness.test`, `TrainHarness.render_path` and `ViewRenderer`.  What the reference does on the host between a rendered
fp32 frame and displayable bytes (`.cpu().numpy()`, `F.interpolate`, `linear_to_srgb`, `* 255`, `astype`, a numpy running
mean, `cv2.imwrite` inside the loop) is ONE launch here (csrc/view_finish.hip), and the files are written behind the render.

    finish(image, depth, ...)            a rendered frame -> the shown / written frame: the kernel on CUDA tensors, else ...
    finish_statement(...)                ... the torch statement: the CPU path, and what the tests hold the kernel to
    minmax(image) / minmax_statement     the frame's smallest and largest value, left on the device
    ViewRenderer(harness, H, W, intrinsics, opt).frame(pose, bg_color, downscale)       test_gui + the GUI's running mean
    harness_test / harness_render_path   the bodies of TrainHarness.test / .render_path

Semantics of `finish`, the same on every path; image [h, w, C] fp32 (C in 1..3), depth [h, w] or
None, output H x W; every fp32 operation is rounded on its own:
  1. nearest source pixel: F.interpolate(mode="nearest", size=(H, W))'s index, per axis min(int(floor(y * fp32(h / H))), h - 1);
  2. `minmax` ([2] on the device): v = (v - min) / (max - min) (scripts/render.py:502); 0 where max == min;
  3. `linear`: evaluate.linear_to_srgb, v < 0.0031308 ? 12.92 v : 1.055 v ** 0.41666 - 0.055;
  4. `accum` ([H, W, C], updated in place) with `spp` samples in it: a = (a * spp + v) / (spp + 1) (nerf/gui.py:143 in numpy
     fp32), v = a from here on; spp == 0 overwrites;
  5. bytes: evaluate.to_u8, uint8 of clip(v * 255, 0, 255), truncated; NaN gives 0.
The depth outputs take steps 1 and 5 only.
Deviations from the reference: its `(x * 255).astype(np.uint8)` wraps values above 255 where this clips (as
enerf_amd/evaluate.py documents); PNGs are written in RGB order by evaluate.write_png (no cv2: cv2.imwrite expects BGR, and
scripts/render.py hands it RGB); the raw frames of render_path are `raws/{i}.npy` (np.save appends to the script's
`{i}.png`); its depth PNG is one grey plane for every C (the script's reshape to [H, W, C] only works for C = 1).
"""
import os
import queue
import threading

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib as L
from . import evaluate as E
from . import frame_sampler as FS

OUTPUTS = ("image", "image_u8", "depth", "depth_u8")
LINEAR = 1                      # include/enerf_hip.h ENERF_VIEW_LINEAR
MINMAX_WS = 512                 # include/enerf_hip.h ENERF_VIEW_MINMAX_WS


# ------------------------------------------------------------------------------------------------------ statements
def nearest_index(h, w, H, W, device=None):
    """The source pixel F.interpolate(mode="nearest", size=(H, W)) reads for every output pixel -> i64 [H, W] (row * w +
    col).  The two axes are independent there, so each is asked of the function on an fp32 ramp of its own (exact, and the
    same index whatever the image's dtype: the function computes its scale in the tensor's type)."""
    rows = F.interpolate(torch.arange(h, dtype=torch.float32, device=device).view(1, 1, h, 1), size=(H, 1), mode="nearest")
    cols = F.interpolate(torch.arange(w, dtype=torch.float32, device=device).view(1, 1, 1, w), size=(1, W), mode="nearest")
    return rows.view(H, 1).long() * w + cols.view(1, W).long()


def to_u8_statement(v):
    """evaluate.to_u8 on a tensor of any device: uint8 of clip(v * 255, 0, 255), truncated; NaN gives 0."""
    s = v * 255
    return torch.where(s.isnan(), torch.zeros_like(s), s).clamp(0, 255).to(torch.uint8)


def minmax_statement(image):
    """-> [2] of image's dtype on its device: min and max over the values that are not NaN; (0, 1) when there is none."""
    v = image.reshape(-1)
    v = v[~v.isnan()]
    if v.numel() == 0:
        return torch.tensor([0.0, 1.0], dtype=image.dtype, device=image.device)
    return torch.stack(torch.aminmax(v))


def _check(image, depth, out_size, accum, outputs):
    if image.dim() != 3 or not 1 <= image.shape[2] <= 3:
        raise ValueError(f"image {tuple(image.shape)}: [h, w, 1..3] expected")
    h, w, C = image.shape
    H, W = (h, w) if out_size is None else (int(out_size[0]), int(out_size[1]))
    if depth is not None and tuple(depth.shape) != (h, w):
        raise ValueError(f"depth {tuple(depth.shape)}: [{h}, {w}] expected")
    if accum is not None and tuple(accum.shape) != (H, W, C):
        raise ValueError(f"accum {tuple(accum.shape)}: [{H}, {W}, {C}] expected")
    if outputs is None:                         # everything there is an input for
        outputs = OUTPUTS if depth is not None else OUTPUTS[:2]
    bad = [o for o in outputs if o not in OUTPUTS]
    if bad:
        raise ValueError(f"outputs {bad}: a subset of {OUTPUTS} expected")
    if depth is None and ("depth" in outputs or "depth_u8" in outputs):
        raise ValueError("a depth output without depth")
    if accum is not None and "image" not in outputs and "image_u8" not in outputs:
        raise ValueError("accum without the image or image_u8 output")
    return h, w, C, H, W, tuple(outputs)


def finish_statement(image, depth=None, out_size=None, linear=False, minmax=None, accum=None, spp=0, outputs=None):
    """The torch statement of the module docstring's five steps, in the tensors' own dtype (fp32: the CPU path; fp64: the
    yardstick of the tests) -> dict of the requested `outputs`; `accum` is updated in place.  Every divisor is a tensor:
    torch divides by a Python number through its reciprocal on the device, which rounds differently."""
    h, w, C, H, W, outputs = _check(image, depth, out_size, accum, outputs)
    dev, dt = image.device, image.dtype
    idx = None if (H, W) == (h, w) else nearest_index(h, w, H, W, dev).reshape(-1)
    out = {}
    if "image" in outputs or "image_u8" in outputs or accum is not None:
        v = image if idx is None else image.reshape(h * w, C)[idx].reshape(H, W, C)
        if minmax is not None:
            mn, mx = minmax[0].to(dt), minmax[1].to(dt)
            v = torch.where(mx == mn, torch.zeros_like(v), (v - mn) / (mx - mn))
        if linear:
            v = E.linear_to_srgb(v)
        if accum is not None:
            if spp:
                v = (accum * torch.full((), float(spp), dtype=dt, device=dev) + v) \
                    / torch.full((), float(spp + 1), dtype=dt, device=dev)
            accum.copy_(v)
            v = accum
        if "image" in outputs:
            out["image"] = v
        if "image_u8" in outputs:
            out["image_u8"] = to_u8_statement(v)
    if "depth" in outputs or "depth_u8" in outputs:
        d = depth if idx is None else depth.reshape(h * w)[idx].reshape(H, W)
        if "depth" in outputs:
            out["depth"] = d
        if "depth_u8" in outputs:
            out["depth_u8"] = to_u8_statement(d)
    return out


# --------------------------------------------------------------------------------------------------------- native
def _f32c(t, name):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name}: a contiguous float32 tensor expected, got {t.dtype}, contiguous={t.is_contiguous()}")
    return t


def minmax(image):
    """enerf_view_minmax on a CUDA tensor (two launches, nothing read back) -> fp32 [2] on the device; the statement
    otherwise."""
    if not image.is_cuda:
        return minmax_statement(image)
    _f32c(image, "image")
    buf = torch.empty(MINMAX_WS + 2, dtype=torch.float32, device=image.device)      # the partials, then min, max
    L.check(L.lib().enerf_view_minmax(image.data_ptr() if image.numel() else None, image.numel(), buf.data_ptr(),
                                      buf.data_ptr() + 4 * MINMAX_WS, L.stream_handle()), "view_minmax")
    return buf[MINMAX_WS:]


def finish(image, depth=None, out_size=None, linear=False, minmax=None, accum=None, spp=0, outputs=None):
    """A rendered frame -> {"image" [H, W, C] fp32, "image_u8" [H, W, C], "depth" [H, W] fp32, "depth_u8" [H, W]} (those
    named in `outputs`) in ONE launch of enerf_view_finish on CUDA tensors; CPU tensors take `finish_statement`.  With
    `accum` the "image" output IS `accum` (updated in place), not a copy."""
    if not image.is_cuda:
        return finish_statement(image, depth, out_size, linear, minmax, accum, spp, outputs)
    h, w, C, H, W, outputs = _check(image, depth, out_size, accum, outputs)
    _f32c(image, "image")
    dev = image.device
    for t, name in ((depth, "depth"), (minmax, "minmax"), (accum, "accum")):
        if t is not None:
            _f32c(t, name)
            if t.device != dev:
                raise ValueError(f"{name} lives on {t.device}, the image on {dev}")
    if minmax is not None and minmax.numel() != 2:
        raise ValueError(f"minmax {tuple(minmax.shape)}: [2] expected")
    out = {}
    if "image" in outputs:
        out["image"] = accum if accum is not None else torch.empty(H, W, C, dtype=torch.float32, device=dev)
    if "image_u8" in outputs:
        out["image_u8"] = torch.empty(H, W, C, dtype=torch.uint8, device=dev)
    if "depth" in outputs:
        out["depth"] = torch.empty(H, W, dtype=torch.float32, device=dev)
    if "depth_u8" in outputs:
        out["depth_u8"] = torch.empty(H, W, dtype=torch.uint8, device=dev)

    def p(t):
        return None if t is None else t.data_ptr()

    out_f32 = out.get("image")                  # (with accum: the running buffer itself, which the library allows)
    L.check(L.lib().enerf_view_finish(image.data_ptr(), p(depth), h, w, C, H, W, LINEAR if linear else 0, p(minmax),
                                      p(accum), int(spp), p(out_f32), p(out.get("image_u8")), p(out.get("depth")),
                                      p(out.get("depth_u8")), L.stream_handle()), "view_finish")
    return out


# ------------------------------------------------------------------------------------------------ writing behind
class FrameWriter:
    """Files written behind the render.  `submit(jobs)` takes one view's [(kind, path, tensor)] with kind "png"
    (evaluate.write_png) or "npy" (np.save): device tensors are copied asynchronously into one of `ring` sets of pinned
    host buffers and an event is recorded; ONE worker thread waits for that event only, encodes and writes, while the next
    view renders.  The ring bounds the memory: `submit` waits for a free set.  `close()` returns once the worker has
    drained and re-raises what it raised (so does the next `submit`).  `write_behind=False`: the same copies, then the
    event's wait and the writes in the caller, view by view."""

    def __init__(self, write_behind=True, ring=3):
        self.write_behind = bool(write_behind)
        self.error = None
        self._free = queue.Queue()
        for _ in range(max(1, int(ring))):
            self._free.put({})                  # a set of pinned buffers: (shape, dtype, position in the view) -> tensor
        self._work = queue.Queue()
        self._thread = None
        if self.write_behind:
            self._thread = threading.Thread(target=self._run, name="enerf-frame-writer", daemon=True)
            self._thread.start()

    @staticmethod
    def _write(kind, path, arr):
        if kind == "png":
            E.write_png(path, arr)
        elif kind == "npy":
            np.save(path, arr)
        else:
            raise ValueError(f"FrameWriter: kind {kind!r}")

    def _flush(self, item):
        slot, event, jobs = item
        try:
            if self.error is None:              # (after a failure the rest is drained, not written)
                if event is not None:
                    event.synchronize()
                for kind, path, host in jobs:
                    self._write(kind, path, host.numpy())
        except BaseException as e:              # noqa: BLE001 -- handed to the caller by submit() / close()
            self.error = e
        finally:
            self._free.put(slot)

    def _run(self):
        while True:
            item = self._work.get()
            if item is None:
                return
            self._flush(item)

    def submit(self, jobs):
        if self.error is not None:
            self.close()
        slot = self._free.get()                 # waits while every set of buffers is still being written
        staged, event = [], None
        for k, (kind, path, t) in enumerate(jobs):
            t = t.detach()
            if t.is_cuda:
                key = (tuple(t.shape), t.dtype, k)
                host = slot.get(key)
                if host is None:
                    host = slot[key] = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
                host.copy_(t, non_blocking=True)
            else:
                host = t
            staged.append((kind, path, host))
        if any(t.is_cuda for _, _, t in jobs):
            event = torch.cuda.Event()
            event.record()
        item = (slot, event, staged)
        if self.write_behind:
            self._work.put(item)
        else:
            self._flush(item)
            if self.error is not None:
                self.close()

    def close(self):
        if self._thread is not None:
            self._work.put(None)
            self._thread.join()
            self._thread = None
        if self.error is not None:
            e, self.error = self.error, None
            raise e


# --------------------------------------------------------------------------------------------------- entry points
def _frame(out, H, W, C):
    """model.render's output -> image [H, W, C], depth [H, W], fp32 and contiguous."""
    return out["image"].reshape(H, W, C).float().contiguous(), out["depth"].reshape(H, W).float().contiguous()


def _rays(poses, v, intrinsics, H, W):
    """Full-frame rays of poses[v] ([V, 4, 4] fp32 on the model's device) -> rays_o, rays_d [1, H W, 3]."""
    fn = FS.frame_batch if poses.is_cuda else FS.rays_statement
    ro, rd, _ = fn(poses, v, intrinsics, H, W)
    return ro[None], rd[None]


def _poses44(poses):
    """[n, 3, 4] / [n, 4, 4] (numpy or tensor) -> float32 numpy [n, 4, 4]."""
    p = poses.detach().cpu().numpy() if torch.is_tensor(poses) else np.asarray(poses)
    p = np.asarray(p, np.float32)
    if p.ndim == 2:
        p = p[None]
    if p.ndim != 3 or p.shape[1] not in (3, 4) or p.shape[2] != 4:
        raise ValueError(f"poses {p.shape}: [n, 3, 4] or [n, 4, 4] expected")
    out = np.tile(np.eye(4, dtype=np.float32), (p.shape[0], 1, 1))
    out[:, :p.shape[1]] = p
    return out


def _upload(host, dev):
    """A host array -> the device without a blocking copy (pinned staging memory, returned to torch's host pool once the
    copy has run)."""
    t = torch.from_numpy(np.ascontiguousarray(host))
    if dev.type != "cuda":
        return t.to(dev)
    pinned = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    pinned.copy_(t)
    return pinned.to(dev, non_blocking=True)


def _eval_scope(harness, fn, ema=None):
    """fn() under model.eval(), no_grad and the harness's regime, with the average's store / copy_to / restore around it
    when given; the previous training mode is restored."""
    model = harness.model
    was_training = model.training
    model.eval()
    try:
        if ema is not None:
            ema.store()
            ema.copy_to()
        try:
            with torch.no_grad():
                return E._in_regime(harness, fn)
        finally:
            if ema is not None:
                ema.restore()
    finally:
        model.train(was_training)


def harness_test(harness, views, opt, save_path, name=None, write_depth=None, write_behind=True):
    """TrainHarness.test: the reference's Trainer.test over `views` -> the list of the written image paths."""
    model = harness.model
    dev = next(model.parameters()).device
    C = int(E._opt(opt, "out_dim_color", 3))
    linear = E._opt(opt, "color_space", "srgb") == "linear"
    kw = E.render_kwargs(opt)
    if name is None:
        name = f"ngp_ep{harness.epoch:04d}"
    if write_depth is None:
        write_depth = harness.epoch % 100 == 0              # "save depth less often" (nerf/utils.py:797)
    os.makedirs(save_path, exist_ok=True)
    os.makedirs(os.path.join(save_path, "depth"), exist_ok=True)
    outputs = ("image_u8", "depth_u8") if write_depth else ("image_u8",)
    paths = []
    writer = FrameWriter(write_behind)

    def loop():
        for i, data in enumerate(views):
            H, W = int(data["H"]), int(data["W"])
            out = model.render(data["rays_o"].to(dev), data["rays_d"].to(dev), staged=True, bg_color=None, perturb=False,
                               **kw)
            image, depth = _frame(out, H, W, C)
            f = finish(image, depth if write_depth else None, linear=linear, outputs=outputs)
            path = os.path.join(save_path, f"{name}_{i:04d}.png")
            jobs = [("png", path, f["image_u8"])]
            if write_depth:
                jobs.append(("png", os.path.join(save_path, "depth", f"{name}_{i:04d}_depth.png"), f["depth_u8"]))
            writer.submit(jobs)
            paths.append(path)

    try:
        _eval_scope(harness, loop)
    finally:
        writer.close()
    return paths


def harness_render_path(harness, poses, intrinsics, H, W, opt, outdir, normalize=False, write_behind=True):
    """TrainHarness.render_path: the loop of scripts/render.py:489-509 over `poses` -> the list of the rgb paths."""
    model = harness.model
    dev = next(model.parameters()).device
    C = int(E._opt(opt, "out_dim_color", 3))
    kw = E.render_kwargs(opt)
    H, W = int(H), int(W)
    intrinsics = tuple(float(a) for a in intrinsics)
    for sub in ("rgb", "depth", "raws"):
        os.makedirs(os.path.join(outdir, sub), exist_ok=True)
    host = _poses44(poses)
    paths = []
    writer = FrameWriter(write_behind)

    def loop():
        dposes = _upload(host, dev)
        for i in range(host.shape[0]):
            ro, rd = _rays(dposes, i, intrinsics, H, W)
            image, depth = _frame(model.render(ro, rd, staged=True, bg_color=1, perturb=False, **kw), H, W, C)
            if normalize:
                f = finish(image, depth, minmax=minmax(image), outputs=("image", "image_u8", "depth_u8"))
                raw = f["image"]
            else:
                f = finish(image, depth, outputs=("image_u8", "depth_u8"))
                raw = image
            path = os.path.join(outdir, "rgb", f"{i}.png")
            writer.submit([("png", path, f["image_u8"]),
                           ("png", os.path.join(outdir, "depth", f"{i}_depth.png"), f["depth_u8"]),
                           ("npy", os.path.join(outdir, "raws", f"{i}.npy"), raw)])
            paths.append(path)

    try:
        _eval_scope(harness, loop)
    finally:
        writer.close()
    return paths


class ViewRenderer:
    """The reference's Trainer.test_gui (nerf/utils.py:870-918) with the accumulation its GUI keeps around it
    (nerf/gui.py:119-149), on the device.

        frame(pose, bg_color=None, downscale=1.0) -> {"image" [H, W, C] fp32, "depth" [H, W] fp32, "image_u8" [H, W, C],
                                                      "spp"}: device tensors, nothing is read back

    A call renders rH x rW = int(H downscale) x int(W downscale) rays of `pose` (a host [4, 4] / [3, 4] cam2world) with
    intrinsics * downscale, under model.eval(), no_grad, the harness's regime and -- when the harness keeps one -- its
    average; ONE enerf_view_finish launch then upsamples to H x W, applies linear_to_srgb for color_space = "linear" and
    folds the frame into the running mean.  "image" is that running buffer itself (valid until the next call), "spp" the
    samples in it; the render's `perturb` is max(samples so far, 1), the seed the GUI hands over.  The count starts again
    when pose, downscale or bg_color differ from the last call and stops growing at `max_spp`: from there on the last
    result is returned and nothing is rendered."""

    def __init__(self, harness, H, W, intrinsics, opt=None, max_spp=64):
        self.harness, self.opt = harness, opt
        self.H, self.W = int(H), int(W)
        self.intrinsics = tuple(float(a) for a in intrinsics)
        self.max_spp = int(max_spp)
        self.C = int(E._opt(opt, "out_dim_color", 3))
        self.linear = E._opt(opt, "color_space", "srgb") == "linear"
        self.spp = 0
        self._key = None
        self._pose = self._bg = self._accum = self._last = None

    @staticmethod
    def _bg_key(bg):
        if bg is None:
            return None
        if torch.is_tensor(bg):
            if bg.is_cuda:                      # (comparing values would read back: the same tensor, unchanged)
                return ("cuda", bg.data_ptr(), bg._version, tuple(bg.shape))
            return ("host", bg.detach().numpy().astype(np.float64).tobytes())
        return ("host", np.asarray(bg, np.float64).tobytes())

    def reset(self):
        """Start the sample count again at the next frame()."""
        self._key = None

    def frame(self, pose, bg_color=None, downscale=1.0):
        h = self.harness
        dev = next(h.model.parameters()).device
        host = _poses44(pose)
        if host.shape[0] != 1:
            raise ValueError(f"one pose per frame, got {host.shape[0]}")
        key = (host.tobytes(), float(downscale), self._bg_key(bg_color))
        if key != self._key:
            self._key, self.spp = key, 0
            self._pose = _upload(host, dev)
            bg = bg_color
            if bg is not None and not isinstance(bg, (int, float)):
                bg = bg.to(dev) if torch.is_tensor(bg) and bg.is_cuda else \
                    _upload(np.asarray(bg.detach().numpy() if torch.is_tensor(bg) else bg, np.float32), dev)
            self._bg = bg
        elif self.spp >= self.max_spp:
            return dict(self._last, spp=self.spp)
        H, W, C = self.H, self.W, self.C
        rH, rW = int(H * downscale), int(W * downscale)
        if rH < 1 or rW < 1:
            raise ValueError(f"downscale {downscale}: a {rH} x {rW} render")
        intrinsics = tuple(a * downscale for a in self.intrinsics)
        if self._accum is None or self._accum.device != dev:
            self._accum = torch.empty(H, W, C, dtype=torch.float32, device=dev)
        kw = E.render_kwargs(self.opt)

        def render():
            ro, rd = _rays(self._pose, 0, intrinsics, rH, rW)
            return h.model.render(ro, rd, staged=True, bg_color=self._bg, perturb=max(self.spp, 1), **kw)

        image, depth = _frame(_eval_scope(h, render, h.ema), rH, rW, C)
        f = finish(image, depth, out_size=(H, W), linear=self.linear, accum=self._accum, spp=self.spp,
                   outputs=("image", "image_u8", "depth"))
        self.spp += 1
        self._last = {"image": f["image"], "depth": f["depth"], "image_u8": f["image_u8"]}
        return dict(self._last, spp=self.spp)
