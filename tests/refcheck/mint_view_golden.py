"""Mint tests/golden/ref_view.npz and tests/golden/ref_render_path.npz from the reference's own code (this container only).

    cd <repo> && python -B tests/refcheck/mint_view_golden.py

TEST INFRASTRUCTURE ONLY.  ref_view.npz: the reference's `Trainer.test` (nerf/utils.py:768-804) and `Trainer.test_gui`
(:870-918) inside its GUI's `NeRFGUI.test_step` accumulation (nerf/gui.py:116-149) on a seeded cuda_ray = False NeRFNetwork
on the CPU, with the C oracle behind the grid encoder (oracle/ref_import.py), for the cases of tests/test_view_host.py
(24 x 32 views, num_steps = 16, upsample_steps = 0).  cv2 is a mock: `cvtColor` reverses three channels (what RGB2BGR does),
`imwrite` records what it is handed; dearpygui is a mock and the GUI's two device timers are stubs.  torch is seeded before
every perturbed render (the same seeds the test uses).  Stored per case: the reference's fp32 frames and the bytes handed
to imwrite; for the GUI cases the running buffer after every call and the rays get_rays made (they differ from the
project's by an fp32 rounding in places) and how far the reference's own buffers move when every component of its rays is
moved by one fp32 rounding (`*_one_rounding`).  ref_render_path.npz: scripts/render.py's `interpol_traj_between_rand_poses` and `compute_render_poses` and
utils/pose_utils.py's `quatList_to_poses_hom_and_tss` on 12 seeded poses.
"""
import os
import sys
import tempfile

os.environ["MKL_CBWR"] = "COMPATIBLE,STRICT"          # the CPU settings tests/conftest.py pins for the suite
os.environ["OMP_NUM_THREADS"] = "8"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import argparse as ap  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import ref_import  # noqa: E402
from oracle.make_golden import det_fill_  # noqa: E402
from test_eval_host import make_views, BOUND, FILL  # noqa: E402
from test_view_host import TEST_CASES, GUI_CASES, H, W, V, INTRINSICS, gui_pose, gui_bg, path_inputs  # noqa: E402


class Loader:
    batch_size = 1

    def __init__(self, views):
        self.views = views

    def __len__(self):
        return len(self.views)

    def __iter__(self):
        return iter(self.views)


class Timer:
    def __init__(self, *a, **k):
        pass

    def record(self):
        pass

    def elapsed_time(self, other):
        return 1.0


def make_trainer(utils, NeRFNetwork, c, epoch):
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=BOUND, cuda_ray=False, out_dim_color=c["C"])
    det_fill_(list(model.parameters()), c["seed"], *FILL)
    opt = ap.Namespace(num_steps=16, upsample_steps=0, max_ray_batch=4096, color_space=c["color_space"],
                       out_dim_color=c["C"], max_spp=64)
    t = utils.Trainer.__new__(utils.Trainer)
    t.__dict__.update(name="mint", epoch=epoch, local_rank=0, world_size=1, model=model, ema=None, fp16=False, opt=opt,
                      out_dim_color=c["C"], workspace=tempfile.mkdtemp(prefix="enerf_view_mint_"), device="cpu", log_ptr=None)
    t.log = lambda *a, **k: None
    return t, model


def record_renders(model):
    frames = []
    render = model.render

    def recording(*a, **k):
        out = render(*a, **k)
        frames.append((out["image"].detach().clone(), out["depth"].detach().clone()))
        return out

    model.render = recording
    return frames


def run_test(utils, NeRFNetwork, tag, c):
    t, model = make_trainer(utils, NeRFNetwork, c, epoch=100)            # (epoch % 100 == 0: the depth files too)
    frames = record_renders(model)
    written = []
    utils.cv2.cvtColor = lambda img, code: img[..., ::-1] if img.shape[-1] == 3 else img
    utils.cv2.imwrite = lambda path, img: written.append((path, np.array(img)))
    views = make_views(c["seed"], V, H, W, c["C"], False)
    t.test(Loader(views), save_path=t.workspace, name="t")
    assert len(written) == 2 * V and len(frames) == V
    z = {f"{tag}_render": np.stack([f[0].reshape(H, W, c["C"]).numpy() for f in frames]),
         f"{tag}_depth": np.stack([f[1].reshape(H, W).numpy() for f in frames]),
         f"{tag}_bytes": np.stack([w[1] for w in written[0::2]]),
         f"{tag}_depth_bytes": np.stack([w[1] for w in written[1::2]]),
         f"{tag}_names": np.array([os.path.relpath(w[0], t.workspace) for w in written])}
    return z


def run_gui(utils, gui, NeRFNetwork, tag, c):
    z = gui_buffers(utils, gui, NeRFNetwork, c, nudge=False)
    # the reference's own sensitivity to ONE fp32 rounding of its rays: every component of rays_d moved to the next fp32
    # value up or down (seeded signs), everything else the same -- how far its buffers move is what a ray statement with
    # another operation order costs, and the bar's unit in tests/test_view_host.py
    moved = gui_buffers(utils, gui, NeRFNetwork, c, nudge=True)
    assert np.abs(moved["rays_d"] - z["rays_d"]).max() <= 2.0 ** -24
    return {f"{tag}_buffers": z["buffers"], f"{tag}_rays_o": z["rays_o"], f"{tag}_rays_d": z["rays_d"],
            f"{tag}_one_rounding": np.float64(np.abs(moved["buffers"] - z["buffers"]).max())}


def gui_buffers(utils, gui, NeRFNetwork, c, nudge):
    t, model = make_trainer(utils, NeRFNetwork, c, epoch=1)
    g = gui.NeRFGUI.__new__(gui.NeRFGUI)
    g.__dict__.update(opt=t.opt, W=W, H=H, trainer=t, bg_color=gui_bg(c), spp=1, need_update=True,
                      dynamic_resolution=False, downscale=c["downscale"],
                      cam=ap.Namespace(pose=gui_pose(c["seed"]), intrinsics=np.array(INTRINSICS)),
                      render_buffer=np.zeros((W, H, 3), np.float32))
    event, sync = torch.cuda.Event, torch.cuda.synchronize
    torch.cuda.Event, torch.cuda.synchronize = Timer, lambda: None
    buffers, rays = [], []
    get_rays = utils.get_rays

    def recording_rays(*a, **k):
        r = get_rays(*a, **k)
        if nudge:
            up = torch.rand(r["rays_d"].shape, generator=torch.Generator().manual_seed(c["seed"])) < 0.5
            inf = torch.where(up, torch.tensor(float("inf")), torch.tensor(-float("inf")))
            r["rays_d"] = torch.nextafter(r["rays_d"].contiguous(), inf)
        rays.append(r)
        return r

    utils.get_rays = recording_rays
    try:
        for k in range(c["calls"]):
            torch.manual_seed(c["seed"] * 100 + k)
            g.test_step()
            assert g.spp == k + 1
            buffers.append(np.array(g.render_buffer, copy=True))
    finally:
        torch.cuda.Event, torch.cuda.synchronize = event, sync
        utils.get_rays = get_rays
    assert all(b.dtype == np.float32 for b in buffers) and len(rays) == c["calls"]
    assert all(torch.equal(r["rays_d"], rays[0]["rays_d"]) for r in rays)
    return {"buffers": np.stack(buffers), "rays_o": rays[0]["rays_o"][0, 0].numpy(), "rays_d": rays[0]["rays_d"][0].numpy()}


def run_paths(render, pose_utils):
    poses, quats = path_inputs()
    np.random.seed(5)
    between, i0, i1 = render.interpol_traj_between_rand_poses(poses, 7)
    spiral = render.compute_render_poses(poses[:, :3, :4], mind=0.9, maxd=1.2, rad_scale=0.2)
    _, hom = pose_utils.quatList_to_poses_hom_and_tss(list(quats))
    return {"between": np.asarray(between), "between_idx": np.array([i0, i1]), "spiral": np.asarray(spiral),
            "quat_poses": np.asarray(hom)}


def main():
    ref_import.install()
    from nerf.network import NeRFNetwork
    from nerf import utils
    z = {}
    for tag, c in TEST_CASES.items():
        z.update(run_test(utils, NeRFNetwork, tag, c))
    from nerf import gui
    for tag, c in GUI_CASES.items():
        z.update(run_gui(utils, gui, NeRFNetwork, tag, c))
    for k, v in z.items():
        print(k, v.shape, v.dtype)
    out = os.path.join(ROOT, "tests", "golden", "ref_view.npz")
    np.savez_compressed(out, **z)
    print(f"wrote {out}: {os.path.getsize(out)} bytes")
    try:
        from unittest.mock import MagicMock
        for m in ("pandas", "matplotlib", "matplotlib.pyplot", "mpl_toolkits", "mpl_toolkits.mplot3d", "open3d", "yaml",
                  "plotly", "plotly.graph_objects", "seaborn"):
            try:
                __import__(m)
            except Exception:                      # noqa: BLE001
                sys.modules[m] = MagicMock()
        sys.path.insert(0, os.path.join(ref_import.REFERENCE, "scripts"))
        import render
        from utils import pose_utils
    except Exception as e:                         # noqa: BLE001
        print(f"scripts/render.py cannot be imported here ({e!r}): ref_render_path.npz NOT minted")
        raise
    p = run_paths(render, pose_utils)
    for k, v in p.items():
        print(k, v.shape, v.dtype)
    out = os.path.join(ROOT, "tests", "golden", "ref_render_path.npz")
    np.savez_compressed(out, **p)
    print(f"wrote {out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
