"""Mint tests/golden/ref_frame_batch.npz from the reference's own `get_rays` and `Trainer.train_step` (this container only).

    cd <repo> && python -B tests/refcheck/mint_frame_batch_golden.py

TEST INFRASTRUCTURE ONLY.  Runs the reference's `get_rays` (nerf/utils.py:111-174) on the CPU for three image sizes --
(30, 50): both cell scales below 1, many cells per pixel, the H - 1 / W - 1 clamp hit; (48, 64); (480, 640) -- with V = 3
non-identity poses, view index [2], intrinsics with non-integer cx, cy and N = 257, once uniform and once with a
non-constant error map.  `torch.randint`, `torch.multinomial` and `torch.rand` are wrapped for the call so that the draws
are stored beside the inputs and the outputs.  Also one error-map write-back of `Trainer.train_step` (lines 610-632), run
through the reference's method on a model stub whose render returns a fixed image: old row, inds_coarse, per-ray error,
new row.  Data only.
"""
import argparse as ap
import os
import sys

os.environ["MKL_CBWR"] = "COMPATIBLE,STRICT"          # the CPU settings tests/conftest.py pins for the suite
os.environ["OMP_NUM_THREADS"] = "8"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import ref_import  # noqa: E402

CASES = {"s30x50": (30, 50), "s48x64": (48, 64), "s480x640": (480, 640)}
V, VIEW, N = 3, 2, 257


def make_poses(seed):
    g = np.random.default_rng(seed)
    poses = np.zeros((V, 4, 4), np.float32)
    for v in range(V):
        q, _ = np.linalg.qr(g.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        poses[v, :3, :3] = q
        poses[v, :3, 3] = g.uniform(-2, 2, 3)
        poses[v, 3, 3] = 1
    return poses


def make_intrinsics(H, W):
    return np.array([0.9 * W + 0.37, 0.85 * W - 0.21, W / 2 - 0.3, H / 2 + 0.45], np.float32)


def make_error_map(seed):
    g = np.random.default_rng(seed)
    return g.uniform(0.01, 1.0, (V, 128 * 128)).astype(np.float32) ** 3


class Recorder:
    """torch.randint / multinomial / rand for the duration of one get_rays call: the real functions, their results kept."""

    def __enter__(self):
        self.calls = []
        self.real = {n: getattr(torch, n) for n in ("randint", "multinomial", "rand")}
        for n, f in self.real.items():
            setattr(torch, n, self._wrap(n, f))
        return self

    def _wrap(self, name, f):
        def g(*a, **k):
            out = f(*a, **k)
            self.calls.append((name, out.clone()))
            return out
        return g

    def __exit__(self, *exc):
        for n, f in self.real.items():
            setattr(torch, n, f)


def run_case(utils, tag, H, W, seed):
    poses, intr = make_poses(seed), make_intrinsics(H, W)
    emap = make_error_map(seed + 1)
    z = {f"{tag}_poses": poses, f"{tag}_intrinsics": intr, f"{tag}_error_map_row": emap[VIEW]}
    p = torch.from_numpy(poses)[[VIEW]]
    torch.manual_seed(seed)
    with Recorder() as rec:
        out = utils.get_rays(p, intr, H, W, N)
    assert [n for n, _ in rec.calls] == ["randint"]
    assert torch.equal(rec.calls[0][1].expand(1, N), out["inds"])
    z.update({f"{tag}_u_inds": out["inds"].numpy(), f"{tag}_u_rays_o": out["rays_o"].numpy().copy(),
              f"{tag}_u_rays_d": out["rays_d"].numpy()})
    with Recorder() as rec:
        out = utils.get_rays(p, intr, H, W, N, error_map=torch.from_numpy(emap)[[VIEW]])
    assert [n for n, _ in rec.calls] == ["multinomial", "rand", "rand"]
    assert torch.equal(rec.calls[0][1], out["inds_coarse"])
    z.update({f"{tag}_e_inds_coarse": out["inds_coarse"].numpy(), f"{tag}_e_u_row": rec.calls[1][1].numpy(),
              f"{tag}_e_u_col": rec.calls[2][1].numpy(), f"{tag}_e_inds": out["inds"].numpy(),
              f"{tag}_e_rays_o": out["rays_o"].numpy().copy(), f"{tag}_e_rays_d": out["rays_d"].numpy()})
    return z


def run_write_back(utils, seed):
    """Trainer.train_step on a stub model: its error-map lines, as data."""
    g = torch.Generator().manual_seed(seed)
    emap = torch.from_numpy(make_error_map(seed))
    inds_coarse = torch.randperm(128 * 128, generator=g)[:N][None]
    pred, images = torch.rand(1, N, 3, generator=g), torch.rand(1, N, 3, generator=g)
    model = ap.Namespace(bg_radius=0, render=lambda *a, **k: {"image": pred})
    T = utils.Trainer
    t = T.__new__(T)
    t.__dict__.update(opt=ap.Namespace(color_space="srgb"), out_dim_color=3, model=model, error_map=emap.clone(),
                      criterion=torch.nn.MSELoss(reduction="none"), device="cpu")
    data = {"rays_o": torch.zeros(1, N, 3), "rays_d": torch.zeros(1, N, 3), "images": images, "index": [VIEW],
            "inds_coarse": inds_coarse}
    t.train_step(data)
    error = ((pred - images) ** 2).mean(-1)
    assert torch.equal(t.error_map[:VIEW], emap[:VIEW])
    return {"wb_old": emap[VIEW].numpy(), "wb_inds_coarse": inds_coarse.numpy(), "wb_error": error.numpy(),
            "wb_new": t.error_map[VIEW].numpy()}


def main():
    ref_import.install()
    from nerf import utils
    z = {}
    for k, (tag, (H, W)) in enumerate(CASES.items()):
        z.update(run_case(utils, tag, H, W, 40 + 10 * k))
    z.update(run_write_back(utils, 77))
    for k, v in z.items():
        print(k, v.shape, v.dtype)
    out = os.path.join(ROOT, "tests", "golden", "ref_frame_batch.npz")
    np.savez_compressed(out, **z)
    print(f"wrote {out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
