"""Frame batches on the device: the frame side of the reference's collate (provider.py:645-663 `NeRFDataset.collate` ->
nerf/utils.py:111-174 `get_rays`) with its `--error_map` option (main_nerf.py:181), and the error map's write-back of
`Trainer.train_step` (nerf/utils.py:610-632), in HIP (csrc/frame_batch.hip).

    FrameSampler(poses, intrinsics, H, W, images, num_rays, error_map)
        .batch(index)                    one view's rays, target pixels and pixel indices: the draw plus ONE launch when
                                         uniform, plus TWO with the error map; no H*W-sized temporary, no host read-back
        .update_error(index, inds_coarse, error)        the EMA of that view's row of the map: one launch

Semantics, the same on every path; every product, quotient and sum is rounded to fp32 on its own:
  * rays: pixel p -> i = p % W, j = p / W as fp32 (integer pixel coordinates, no +0.5); x = (i - cx) / fx,
    y = (j - cy) / fy; d = (x, y, 1) / sqrt((x^2 + y^2) + 1); rays_d = R d with R = poses[v, :3, :3], each component
    (R0 dx + R1 dy) + R2 dz; rays_o = poses[v, :3, 3]; target = images[v, p, :].  The reference's torch ops divide by
    fx through a reciprocal on the device and sum the matmul in the BLAS's order: both are within a few fp32 roundings.
  * uniform sampling: p = torch.randint(0, H W, [N]) (duplicates possible), as get_rays line 138.
  * error-map sampling: weights = the view's row of `error_map` [V, 128 * 128]; with e ~ Exp(1) per cell,
    key_c = weights[c] / e[c] where weights[c] > 0, else 0; the N cells with the largest key, ties to the smaller cell
    index, in that order, are `inds_coarse`.  That is sampling without replacement with probability proportional to the
    weights -- the exponential-race form torch.multinomial(replacement=False) itself uses on the device; torch's random
    stream is NOT reproduced, only the distribution and the result for given draws.  Cell c -> r = c // 128, q = c % 128,
    sx = fp32(H / 128), sy = fp32(W / 128); row = min(int(fp32(r) sx + u_row sx), H - 1), col = min(int(fp32(q) sy + u_col sy),
    W - 1), p = row W + col (get_rays lines 145-149).
  * write-back: map[v, inds_coarse[k]] = fp32(0.1) map[v, inds_coarse[k]] + fp32(0.9) error[k].
Deviation from the reference: torch.multinomial raises when fewer than N cells have a positive weight; here the cells of
weight <= 0 sort last (by cell index) and are taken once the positive ones are used up, so the call stays defined.

Device tensors run the kernels or raise; CPU tensors run the torch statements below (`rays_statement`,
`select_statement`, `pixels_statement`, `update_statement`), which are also what the tests hold the kernels to, with
`rays_fp64` (numpy) as the yardstick of the rays' rounding error.
"""
import numpy as np
import torch

from . import _lib as L

CELLS = 128 * 128               # include/enerf_hip.h ENERF_ERROR_MAP_CELLS
SIDE = 128


# ------------------------------------------------------------------------------------------------------ statements
def rays_statement(poses, v, intrinsics, H, W, inds=None, images=None):
    """-> rays_o, rays_d [N, 3] fp32 and target [N, Ci] (None without images) of view v; inds i64 [N], None = every pixel."""
    fx, fy, cx, cy = (float(a) for a in intrinsics)
    dev = poses.device
    if inds is None:
        inds = torch.arange(H * W, device=dev)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)  # noqa: E731
    i, j = (inds % W).float(), torch.div(inds, W, rounding_mode="floor").float()
    x, y = (i - f32(cx)) / f32(fx), (j - f32(cy)) / f32(fy)
    n = torch.sqrt((x * x + y * y) + 1.0)
    d = (x / n, y / n, 1.0 / n)
    R = poses[v, :3, :3].float()
    rays_d = torch.stack([(R[a, 0] * d[0] + R[a, 1] * d[1]) + R[a, 2] * d[2] for a in range(3)], dim=-1)
    rays_o = poses[v, :3, 3].float().expand_as(rays_d).contiguous()
    target = None if images is None else images[v].reshape(H * W, -1)[inds]
    return rays_o, rays_d, target


def rays_fp64(poses, v, intrinsics, W, inds):
    """The same rays evaluated in fp64 (numpy) from the fp32 inputs -> rays_d [N, 3] float64."""
    fx, fy, cx, cy = (np.float64(np.float32(a)) for a in intrinsics)
    inds = np.asarray(inds, np.int64)
    x, y = ((inds % W) - cx) / fx, ((inds // W) - cy) / fy
    d = np.stack([x, y, np.ones_like(x)], -1)
    d /= np.sqrt((d * d).sum(-1, keepdims=True))
    return d @ np.asarray(poses, np.float64)[v, :3, :3].T


def select_statement(weights, e, N):
    """weights, e fp32 [..., 16384] -> inds_coarse i64 [..., N]: the N largest keys weights / e (0 where weights <= 0),
    ties to the smaller cell."""
    key = torch.where(weights > 0, weights / e, torch.zeros_like(e))
    return torch.sort(key, dim=-1, descending=True, stable=True).indices[..., :N]


def pixels_statement(inds_coarse, u_row, u_col, H, W):
    """get_rays lines 145-149 with given jitters -> pixel indices i64, shaped like inds_coarse."""
    sx, sy = H / 128, W / 128
    r, q = torch.div(inds_coarse, SIDE, rounding_mode="floor"), inds_coarse % SIDE
    row = (r * sx + u_row * sx).long().clamp(max=H - 1)
    col = (q * sy + u_col * sy).long().clamp(max=W - 1)
    return row * W + col


def update_statement(row, inds_coarse, error):
    """-> the view's row [16384] after the EMA write-back at inds_coarse (nerf/utils.py:628-629)."""
    ema = 0.1 * row.gather(0, inds_coarse) + 0.9 * error
    return row.scatter(0, inds_coarse, ema)


# ------------------------------------------------------------------------------------------------------ kernels
def _f32c(t, name):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name}: a contiguous float32 tensor expected, got {t.dtype}, contiguous={t.is_contiguous()}")
    return t


def _i64c(t, name):
    if t.dtype != torch.int64 or not t.is_contiguous():
        raise ValueError(f"{name}: a contiguous int64 tensor expected, got {t.dtype}, contiguous={t.is_contiguous()}")
    return t


def frame_batch(poses, v, intrinsics, H, W, inds=None, images=None):
    """enerf_frame_batch on device tensors -> rays_o, rays_d [N, 3], target [N, Ci] or None."""
    L.check_cuda(poses, "poses")
    fx, fy, cx, cy = (float(a) for a in intrinsics)
    _f32c(poses, "poses")
    N = H * W if inds is None else _i64c(inds, "inds").numel()
    dev = poses.device
    rays_o = torch.empty(N, 3, dtype=torch.float32, device=dev)
    rays_d = torch.empty(N, 3, dtype=torch.float32, device=dev)
    Ci, target = 0, None
    if images is not None:
        _f32c(images, "images")
        if images.dim() != 4 or tuple(images.shape[:3]) != (poses.shape[0], H, W) or not 1 <= images.shape[3] <= 4:
            raise ValueError(f"images {tuple(images.shape)}: [{poses.shape[0]}, {H}, {W}, 1..4] expected")
        Ci = images.shape[3]
        target = torch.empty(N, Ci, dtype=torch.float32, device=dev)
    L.check(L.lib().enerf_frame_batch(poses.data_ptr(), poses.shape[0], int(v), fx, fy, cx, cy, H, W,
                                      None if inds is None else inds.data_ptr(), N,
                                      None if images is None else images.data_ptr(), Ci, rays_o.data_ptr(),
                                      rays_d.data_ptr(), None if target is None else target.data_ptr(),
                                      L.stream_handle()), "frame_batch")
    return rays_o, rays_d, target


def error_map_sample(weights, e, u_row, u_col, H, W, inds_coarse=None):
    """enerf_error_map_sample on device tensors -> (inds_coarse, inds) i64 [N].  With `inds_coarse` given the selection
    is skipped (weights and e are not read) and only the pixel mapping runs."""
    L.check_cuda(u_row, "u_row")
    N = _f32c(u_row, "u_row").numel()
    if _f32c(u_col, "u_col").numel() != N:
        raise ValueError("u_row and u_col differ in length")
    inds = torch.empty(N, dtype=torch.int64, device=u_row.device)
    if inds_coarse is None:
        if _f32c(weights, "weights").numel() != CELLS or _f32c(e, "e").numel() != CELLS:
            raise ValueError(f"weights and e: {CELLS} cells expected")
        inds_coarse = torch.empty(N, dtype=torch.int64, device=u_row.device)
        wp, ep = weights.data_ptr(), e.data_ptr()
    else:
        if _i64c(inds_coarse, "inds_coarse").numel() != N:
            raise ValueError("inds_coarse and u_row differ in length")
        wp = ep = None
    L.check(L.lib().enerf_error_map_sample(wp, ep, u_row.data_ptr(), u_col.data_ptr(), N, H, W, inds_coarse.data_ptr(),
                                           inds.data_ptr(), L.stream_handle()), "error_map_sample")
    return inds_coarse, inds


def error_map_update(row, inds_coarse, error):
    """enerf_error_map_update, in place on `row` [16384] (a view of the map)."""
    L.check_cuda(row, "error_map")
    if _f32c(row, "error_map row").numel() != CELLS:
        raise ValueError(f"error_map row: {CELLS} cells expected")
    if _i64c(inds_coarse, "inds_coarse").numel() != _f32c(error, "error").numel():
        raise ValueError("inds_coarse and error differ in length")
    L.check(L.lib().enerf_error_map_update(row.data_ptr(), inds_coarse.data_ptr(), error.data_ptr(), error.numel(),
                                           L.stream_handle()), "error_map_update")


# ------------------------------------------------------------------------------------------------------ the sampler
class FrameSampler:
    """One view per batch (the reference's loaders use batch size 1).  `poses` [V, 4, 4] fp32 cam2world, `intrinsics`
    (fx, fy, cx, cy), `images` [V, H, W, Ci] fp32 (Ci in 1..4) or None, all on one device; `num_rays` = -1: the full
    frame.  `error_map=True` keeps `self.error_map` = ones [V, 128 * 128] (provider.py:647) and samples from it."""

    def __init__(self, poses, intrinsics, H, W, images=None, num_rays=4096, error_map=False):
        if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4):
            raise ValueError(f"poses {tuple(poses.shape)}: [V, 4, 4] expected")
        self.poses = poses.float().contiguous()
        self.intrinsics = tuple(float(a) for a in intrinsics)
        self.H, self.W = int(H), int(W)
        if images is not None:
            if images.dim() != 4 or tuple(images.shape[:3]) != (poses.shape[0], self.H, self.W) \
                    or not 1 <= images.shape[3] <= 4:
                raise ValueError(f"images {tuple(images.shape)}: [{poses.shape[0]}, {H}, {W}, 1..4] expected")
            if images.device != poses.device:
                raise ValueError("images and poses live on different devices")
            images = images.float().contiguous()
        self.images = images
        self.num_rays = int(num_rays)
        self.error_map = (torch.ones(poses.shape[0], CELLS, dtype=torch.float32, device=poses.device)
                          if error_map else None)

    def __len__(self):
        """The number of views: one batch each per epoch (TrainHarness.train_one_epoch)."""
        return int(self.poses.shape[0])

    def _view(self, index):
        if torch.is_tensor(index):
            index = index.reshape(-1).tolist()
        elif not isinstance(index, (list, tuple)):
            index = [index]
        if len(index) != 1:
            raise ValueError(f"one view per batch: index {list(index)}")
        v = int(index[0])
        if not 0 <= v < self.poses.shape[0]:
            raise ValueError(f"view {v} of {self.poses.shape[0]}")
        return v

    def batch(self, index, generator=None, draws=None):
        """-> {"rays_o", "rays_d" [1, N, 3], "images" [1, N, Ci] (or [1, H, W, Ci] for the full frame), "inds" [1, N],
        "H", "W"} and, with the error map, "inds_coarse" [1, N] and "index".  `draws` replaces the random draws:
        {"inds"}; {"e", "u_row", "u_col"}; or {"inds_coarse", "u_row", "u_col"} (the selection is skipped)."""
        v = self._view(index)
        H, W, dev = self.H, self.W, self.poses.device
        cuda = dev.type == "cuda"
        rays = frame_batch if cuda else rays_statement
        out = {"H": H, "W": W}
        if self.num_rays <= 0:
            ro, rd, _ = rays(self.poses, v, self.intrinsics, H, W)
            if self.images is not None:
                out["images"] = self.images[v][None]
            out["rays_o"], out["rays_d"] = ro[None], rd[None]
            return out
        N = min(self.num_rays, H * W)
        draws = draws or {}
        if self.error_map is None or "inds" in draws:
            inds = draws["inds"] if "inds" in draws else torch.randint(0, H * W, [N], device=dev, generator=generator)
            inds = inds.reshape(-1).contiguous()
        else:
            if N > CELLS:
                raise ValueError(f"error_map: {N} rays without replacement from {CELLS} cells")
            given = draws.get("inds_coarse")
            e = None
            if given is None:
                e = draws["e"] if "e" in draws else \
                    torch.empty(CELLS, dtype=torch.float32, device=dev).exponential_(generator=generator)
            u_row = draws["u_row"] if "u_row" in draws else torch.rand(N, device=dev, generator=generator)
            u_col = draws["u_col"] if "u_col" in draws else torch.rand(N, device=dev, generator=generator)
            u_row, u_col = u_row.reshape(-1).contiguous(), u_col.reshape(-1).contiguous()
            if given is not None:
                given = given.reshape(-1).contiguous()
            if cuda:
                coarse, inds = error_map_sample(self.error_map[v], e, u_row, u_col, H, W, inds_coarse=given)
            else:
                coarse = given if given is not None else select_statement(self.error_map[v], e, N)
                inds = pixels_statement(coarse, u_row, u_col, H, W)
            out["inds_coarse"] = coarse[None]
            out["index"] = [v]
        ro, rd, target = rays(self.poses, v, self.intrinsics, H, W, inds, self.images)
        out["rays_o"], out["rays_d"], out["inds"] = ro[None], rd[None], inds[None]
        if target is not None:
            out["images"] = target[None]
        return out

    def update_error(self, index, inds_coarse, error):
        """Trainer.train_step's write-back (nerf/utils.py:610-632): the EMA of view `index`'s row at `inds_coarse` with
        the per-ray `error`."""
        if self.error_map is None:
            raise RuntimeError("this sampler keeps no error map")
        v = self._view(index)
        row = self.error_map[v]
        coarse = inds_coarse.reshape(-1).contiguous()
        error = error.detach().reshape(-1).float().contiguous()
        if row.is_cuda:
            error_map_update(row, coarse, error)
        else:
            row.copy_(update_statement(row, coarse, error))
