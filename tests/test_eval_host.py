"""TrainHarness.evaluate on the CPU (enerf_amd/evaluate.py): the reference's own
Trainer.evaluate_one_epoch reproduced (tests/golden/ref_eval.npz, minted by tests/refcheck/mint_eval_golden.py), the SSIM
statement on known answers, the PNG writer and the NaN rule of the affine fit."""
import argparse as ap
import math

import numpy as np
import pytest
import torch

from util import det_fill_, golden

BOUND, FILL = 1, (-0.5, 0.5)
MODES = {                                    # the golden's three runs of the reference's evaluate_one_epoch
    "rgb": dict(seed=31, V=3, H=24, W=32, C=3, event_only=False, mode="eds", stereo=False),
    "ev1": dict(seed=32, V=4, H=24, W=32, C=1, event_only=True, mode="eds", stereo=True),
    "ev3": dict(seed=33, V=3, H=24, W=32, C=3, event_only=True, mode="eds", stereo=False),
}


def make_views(seed, V, H, W, C, stereo):
    """V val-split collate dicts: a pinhole camera on z = 1.5 looking down -z at the [-1, 1]^3 box, random images."""
    g = torch.Generator().manual_seed(seed)
    views = []
    for _ in range(V):
        c = (torch.rand(3, generator=g) - 0.5) * torch.tensor([0.6, 0.6, 0.2]) + torch.tensor([0.0, 0.0, 1.5])
        v, u = torch.meshgrid(torch.linspace(-0.3, 0.3, H), torch.linspace(-0.4, 0.4, W), indexing="ij")
        d = torch.stack([u - 0.5 * c[0], v - 0.5 * c[1], -torch.ones_like(u)], -1).reshape(1, H * W, 3)
        d = d / torch.sqrt(d[..., 0:1] * d[..., 0:1] + d[..., 1:2] * d[..., 1:2] + d[..., 2:3] * d[..., 2:3])
        o = c.reshape(1, 1, 3).expand(1, H * W, 3).contiguous()
        view = {"rays_o": o, "rays_d": d, "images": torch.rand(1, H, W, C, generator=g), "H": H, "W": W,
                "H_ev": H, "W_ev": W}
        if stereo:
            view["rays_evs_o"] = (o + torch.tensor([0.05, 0.0, 0.0])).contiguous()
            view["rays_evs_d"] = d.clone()
        views.append(view)
    return views


def _model(m):
    from enerf_amd.network import NeRFNetwork
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=BOUND, cuda_ray=False, out_dim_color=m["C"])
    det_fill_(list(model.parameters()), m["seed"], *FILL)
    return model


def _opt(m):
    return ap.Namespace(event_only=m["event_only"], out_dim_color=m["C"], color_space="srgb", mode=m["mode"],
                        eval_stereo_views=int(m["stereo"]), render_kwargs={"num_steps": 16})


# The reference's dB numbers are numpy fp32 (compute_pnsr, PSNRMeter: the mean, the log10 and the product each round to
# fp32), ours fp64 from the fp64 SSE: 1e-6 dB plus 3 fp32 roundings of the value.
DB = dict(rtol=3 * 2.0 ** -24, atol=1e-6)


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize("tag", list(MODES))
def test_evaluate_reproduces_the_reference_trainer(tag, cpu_oracle_backend, tmp_path):
    from enerf_amd import evaluate as E
    from enerf_amd.trainer import TrainHarness
    g, m = golden("ref_eval"), MODES[tag]
    model = _model(m)
    h = TrainHarness(model)
    views = make_views(m["seed"], m["V"], m["H"], m["W"], m["C"], m["stereo"])
    # the renders first: the metrics below are only as close as these are
    pred, gt, _, ev = E.render_views(h, views, _opt(m))
    np.testing.assert_allclose(pred.numpy(), g[f"{tag}_pred"], rtol=0, atol=1e-6)
    assert len(ev) == (m["V"] if m["stereo"] else 0)
    model.train()
    r = h.evaluate(views, _opt(m), name="t", save_dir=str(tmp_path))
    assert model.training
    assert r["views"] == m["V"]
    assert _rel(r["valid_loss"], float(g[f"{tag}_valid_loss"])) < 1e-6
    if m["stereo"]:
        assert math.isinf(float(g[f"{tag}_meter"]))           # the reference's pair (event view, itself): documented
    else:
        np.testing.assert_allclose(r["psnr_meter"], float(g[f"{tag}_meter"]), **DB)
    if m["event_only"]:
        assert _rel(r["a"], float(g[f"{tag}_a"])) < 1e-9 and _rel(r["b"], float(g[f"{tag}_b"])) < 1e-9
        np.testing.assert_allclose(r["psnr_corrected"], g[f"{tag}_psnr_corrected"], **DB)
        np.testing.assert_allclose(r["ssim_corrected"], g[f"{tag}_ssim"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(r["psnr_corrected_mean"], g[f"{tag}_psnr_corrected"].mean(), **DB)
        files = ["prediction_corrected/t_0000.png", "raw/t_0000.npy", "depth/t_0000_depth.png", "gt/t_0000_gt.png"]
        if m["stereo"]:
            files += ["event_view/prediction_corrected_ev/t_0000.png", "event_view/raw/t_0000.npy",
                      "event_view/depth_ev/t_0000_depth.png"]
    else:
        np.testing.assert_allclose(r["psnr"], g[f"{tag}_psnr"], **DB)
        np.testing.assert_allclose(r["ssim"], g[f"{tag}_ssim"], rtol=0, atol=1e-9)
        assert abs(r["psnr_meter"] - np.mean(r["psnr"])) < 1e-12
        files = ["prediction/t_0000.png", "raw/t_0000.npy", "depth/t_0000_depth.png", "gt/t_0000_gt.png"]
    for f in files:
        assert (tmp_path / "validation" / f).is_file(), f
    assert np.array_equal(np.load(tmp_path / "validation" / "raw" / "t_0000.npy"), pred[0].numpy())


@pytest.mark.parametrize("tag", list(MODES))
def test_statement_on_the_reference_renders(tag):
    """The metrics alone, on the reference's own renders: the same numbers to the fp64 bars."""
    from enerf_amd import evaluate as E
    g, m = golden("ref_eval"), MODES[tag]
    views = make_views(m["seed"], m["V"], m["H"], m["W"], m["C"], m["stereo"])
    pred = torch.from_numpy(g[f"{tag}_pred"])
    gt = torch.stack([v["images"][0] for v in views])
    r = E.summarize(E.metrics(pred, gt, m["event_only"]), m["H"], m["W"], m["C"], m["event_only"])
    assert _rel(r["valid_loss"], float(g[f"{tag}_valid_loss"])) < 1e-6
    if m["event_only"]:
        assert _rel(r["a"], float(g[f"{tag}_a"])) < 1e-9 and _rel(r["b"], float(g[f"{tag}_b"])) < 1e-9
        np.testing.assert_allclose(r["psnr_corrected"], g[f"{tag}_psnr_corrected"], **DB)
        np.testing.assert_allclose(r["ssim_corrected"], g[f"{tag}_ssim"], rtol=0, atol=1e-9)
    else:
        np.testing.assert_allclose(r["psnr"], g[f"{tag}_psnr"], **DB)
        np.testing.assert_allclose(r["ssim"], g[f"{tag}_ssim"], rtol=0, atol=1e-9)


def test_ssim_known_answers():
    from enerf_amd.evaluate import ssim_statement
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 9, 11, generator=g)
    assert torch.allclose(ssim_statement(x, x.clone(), 1.0), torch.ones(2, dtype=torch.float64), rtol=0, atol=1e-15)
    c = torch.full((1, 8, 8), 0.25)
    assert ssim_statement(c, c, 1.0).item() == 1.0
    # one 7 x 7 window, by hand: x = i / 48, y = 1 - x (i = 0 .. 48)
    i = torch.arange(49, dtype=torch.float64)
    xs, ys = i / 48, 1 - i / 48
    ux = uy = 0.5
    vx = vy = float(((xs - 0.5) ** 2).sum() / 48)
    vxy = -vx
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    want = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    got = ssim_statement(xs.reshape(1, 7, 7).float(), ys.reshape(1, 7, 7).float(), 1.0).item()
    assert abs(got - want) < 1e-7                          # (the planes are fp32: i / 48 is rounded once)
    with pytest.raises(ValueError):
        from enerf_amd.evaluate import metrics
        metrics(torch.zeros(1, 6, 9, 1), torch.zeros(1, 6, 9, 1), False)


def test_png_round_trip(tmp_path):
    from enerf_amd.evaluate import write_png, read_png, to_u8, corrected_u8
    g = np.random.default_rng(0)
    for shape in ((5, 7), (6, 4, 3), (3, 9, 1)):
        a = g.integers(0, 256, shape, dtype=np.uint8)
        p = str(tmp_path / f"{len(shape)}_{shape[-1]}.png")
        write_png(p, a)
        assert np.array_equal(read_png(p), a.reshape(shape[:2]) if a.ndim == 3 and shape[-1] == 1 else a)
        assert open(p, "rb").read()[:8] == b"\x89PNG\r\n\x1a\n"
    assert to_u8([-0.5, 0.0, 0.5, 1.0, 1.7]).tolist() == [0, 0, 127, 255, 255]
    assert corrected_u8([-3.0, 0.4, 0.6, 254.5, 300.0]).tolist() == [0, 0, 1, 254, 255]


def test_fit_nan_rule():
    from enerf_amd.evaluate import fit_statement, COLS
    res = torch.zeros(2, COLS, dtype=torch.float64)            # no pixels at all: 0 / 0 for both
    assert fit_statement(res, 0) == (5.0, 5.0)
    res[:, 1:5] = float("nan")
    assert fit_statement(res, 10) == (5.0, 5.0)
    # an exact line: y = 2 x + 1 over x = 0, 1, 2, 3
    x = torch.tensor([0.0, 1.0, 2.0, 3.0], dtype=torch.float64)
    y = 2 * x + 1
    res = torch.zeros(1, COLS, dtype=torch.float64)
    res[0, 1:5] = torch.stack([x.sum(), y.sum(), (x * x).sum(), (x * y).sum()])
    a, b = fit_statement(res, 4)
    assert abs(a - 2) < 1e-12 and abs(b - 1) < 1e-12
