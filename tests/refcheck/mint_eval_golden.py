"""Mint tests/golden/ref_eval.npz from the reference's own evaluation loop (this container only).

    cd <repo> && python -B tests/refcheck/mint_eval_golden.py

TEST INFRASTRUCTURE ONLY.  Runs the reference's `Trainer.evaluate_one_epoch` (nerf/utils.py:1028-1293) on a seeded
cuda_ray = False NeRFNetwork on the CPU, with the C oracle behind the grid encoder (oracle/ref_import.py), over views made
by tests/test_eval_host.py's `make_views` (24 x 32, num_steps = 16, upsample_steps = 0), in three modes: RGB with C = 3;
event-only with C = 1, mode "eds" and the stereo views on; event-only with C = 3.  `ssim` (skimage) is replaced by the
scipy fp64 statement of its defaults and `compute_lpips` by a constant; `writer.add_scalar` goes to a recording stub, cv2
to a mock.  Stored per mode: the recipe, the reference's renders of the rgb views, a, b, the per-view PSNR /
psnr-corrected / SSIM as written to the writer, the PSNRMeter's measure and valid_loss.
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
from test_eval_host import MODES, make_views, BOUND, FILL  # noqa: E402


def ssim_fp64(im1, im2, data_range):
    """skimage.metrics.structural_similarity's defaults (win_size 7, uniform filter, sample covariance, K1 0.01, K2 0.03,
    the 3-pixel border cropped) in fp64 with scipy.ndimage.uniform_filter."""
    from scipy.ndimage import uniform_filter
    X, Y = np.asarray(im1, np.float64), np.asarray(im2, np.float64)
    ux, uy = uniform_filter(X, 7), uniform_filter(Y, 7)
    uxx, uyy, uxy = uniform_filter(X * X, 7), uniform_filter(Y * Y, 7), uniform_filter(X * Y, 7)
    cov = 49.0 / 48.0
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    return S[3:-3, 3:-3].mean()


class Writer:
    def __init__(self):
        self.log = []

    def add_scalar(self, tag, value, step):
        self.log.append((tag, float(value)))


class Loader:
    def __init__(self, views, mode):
        self.views, self.batch_size = views, 1
        self._data = ap.Namespace(mode=mode, H_ev=views[0]["H_ev"], W_ev=views[0]["W_ev"])

    def __len__(self):
        return len(self.views)

    def __iter__(self):
        return iter([{k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()} for d in self.views])


def run_mode(utils, NeRFNetwork, tag, m):
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=BOUND, cuda_ray=False, out_dim_color=m["C"])
    det_fill_(list(model.parameters()), m["seed"], *FILL)
    views = make_views(m["seed"], m["V"], m["H"], m["W"], m["C"], m["stereo"])
    renders = []
    render = model.render

    def recording_render(*a, **k):
        out = render(*a, **k)
        renders.append(out["image"].detach().clone())
        return out

    model.render = recording_render
    opt = ap.Namespace(num_steps=16, upsample_steps=0, max_ray_batch=4096, color_space="srgb", events=m["event_only"],
                       event_only=m["event_only"], out_dim_color=m["C"], eval_stereo_views=int(m["stereo"]))
    T = utils.Trainer
    t = T.__new__(T)
    ws = tempfile.mkdtemp(prefix="enerf_eval_mint_")
    t.__dict__.update(name="mint", epoch=1, eval_interval=1, local_rank=0, world_size=1, model=model, ema=None,
                      fp16=False, opt=opt, out_dim_color=m["C"], event_only=m["event_only"],
                      eval_stereo_views=int(m["stereo"]), writer=Writer(), global_step=0, use_tensorboardX=False,
                      stats={"valid_loss": [], "results": []}, use_loss_as_metric=False, best_mode="max",
                      workspace=ws, log_ptr=None, criterion=torch.nn.MSELoss(reduction="none"), device="cpu",
                      metrics=[utils.PSNRMeter(opt, None)])
    meter = {}
    measure = utils.PSNRMeter.measure

    def recording_measure(self):
        meter["v"] = measure(self)
        return meter["v"]

    utils.PSNRMeter.measure = recording_measure
    t.log = lambda *a, **k: None
    try:
        t.evaluate_one_epoch(Loader(views, m["mode"]), name="mint")
    finally:
        utils.PSNRMeter.measure = measure
    log = t.writer.log
    rgb_renders = torch.stack([r.reshape(m["H"], m["W"], m["C"]) for r in renders[::2 if m["stereo"] else 1]])
    z = {f"{tag}_pred": rgb_renders.numpy(), f"{tag}_valid_loss": np.float64(t.stats["valid_loss"][-1]),
         f"{tag}_meter": np.float64(meter["v"])}
    if m["event_only"]:
        z[f"{tag}_a"] = np.float64(dict(log)["a/"])
        z[f"{tag}_b"] = np.float64(dict(log)["b/"])
        z[f"{tag}_psnr_corrected"] = np.array([v for k, v in log if k.startswith("psnr-corrected/") and k[-1].isdigit()])
        z[f"{tag}_ssim"] = np.array([v for k, v in log if k.startswith("ssim/") and k[-1].isdigit()])
    else:
        z[f"{tag}_psnr"] = np.array([v for k, v in log if k.startswith("psnr/") and k[-1].isdigit()])
        z[f"{tag}_ssim"] = np.array([v for k, v in log if k.startswith("ssim/") and k[-1].isdigit()])
    for k, v in z.items():
        print(k, v if np.ndim(v) < 2 else v.shape)
    return z


def main():
    ref_import.install()
    from nerf.network import NeRFNetwork
    from nerf import utils
    utils.ssim = ssim_fp64
    utils.compute_lpips = lambda p, gt, rgb_channels=3: (0.0, 0.0)
    z = {}
    for tag, m in MODES.items():
        z.update(run_mode(utils, NeRFNetwork, tag, m))
    out = os.path.join(ROOT, "tests", "golden", "ref_eval.npz")
    np.savez_compressed(out, **z)
    print(f"wrote {out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
