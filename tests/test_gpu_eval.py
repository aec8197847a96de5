"""Evaluation metrics on the MI355X (csrc/eval_metrics.hip, enerf_amd/evaluate.py): the kernels
against the torch statement on the same device tensors, run-to-run bit equality, and TrainHarness.evaluate end to end on
the stratified route in fp32 and in the fp16 regime."""
import argparse as ap

import numpy as np
import pytest
import torch

from util import det_fill_

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(1, 7, 7, 1), (3, 8, 9, 3), (3, 37, 53, 1), (54, 37, 53, 3), (1, 480, 640, 1), (3, 480, 640, 3),
          (54, 480, 640, 1)]


def _views(V, H, W, C, seed):
    """pred in [0, 1.2) (above 1 on purpose) with zeroed pixels, gt in [0, 1] with zeros; view 0's pred a plane of tiny
    variance around 0.5."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    pred = torch.rand(V, H, W, C, device=DEV, generator=g) * 1.2
    gt = torch.rand(V, H, W, C, device=DEV, generator=g)
    pred[torch.rand(V, H, W, 1, device=DEV, generator=g).expand(V, H, W, C) < 0.05] = 0.0
    gt[torch.rand(V, H, W, C, device=DEV, generator=g) < 0.05] = 0.0
    pred[0] = 0.5 + 1e-4 * torch.rand(H, W, C, device=DEV, generator=g)
    return pred.contiguous(), gt.contiguous()


def _ulps(a, b):
    ia, ib = a.view(torch.int32).long(), b.view(torch.int32).long()
    ia = torch.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = torch.where(ib < 0, -(ib & 0x7fffffff), ib)
    return (ia - ib).abs().max().item()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("event_only", [False, True], ids=["rgb", "events"])
def test_kernels_against_the_statement(shape, event_only):
    from enerf_amd import evaluate as E
    V, H, W, C = shape
    pred, gt = _views(V, H, W, C, seed=7 * V + H + C)
    got = E.metrics(pred, gt, event_only)
    again = E.metrics(pred, gt, event_only)
    assert np.array_equal(got["res"].view(np.uint64), again["res"].view(np.uint64))          # the same bits
    st = E.stats_statement(pred, gt, event_only).cpu().numpy()
    cols = 5 if event_only else 1
    assert _rel(got["res"][:, :cols], st[:, :cols]) < 1e-12
    if event_only:
        assert (got["a"], got["b"]) == (again["a"], again["b"])
        assert torch.equal(got["pred_cor"], again["pred_cor"]) and torch.equal(got["gt_j"], again["gt_j"])
        a, b = E.fit_statement(torch.from_numpy(st), V * H * W)
        # 1e-9, unless the normal equations cancel (V = 1 with the tiny-variance plane: det = n^2 var(x)): then both
        # sides lose kappa = n sxx / det in fp64, and the bar is that loss
        n, sx, sxx = V * H * W, st[:, 1].sum(), st[:, 3].sum()
        kappa = n * sxx / (n * sxx - sx * sx)
        bar = max(1e-9, 1e-15 * kappa)
        assert _rel(got["a"], a) < bar and _rel(got["b"], b) < bar
        pc, gj, sse = E.correct_statement(pred, gt, got["a"], got["b"])         # the kernel's a, b: the planes alone
        assert _ulps(got["pred_cor"], pc) <= 2 and _ulps(got["gt_j"], gj) <= 2
        assert _rel(got["sse_cor"], sse.cpu().numpy()) < 1e-9
        want = E.ssim_statement(got["gt_j"], got["pred_cor"], 255).cpu().numpy()
    else:
        want = E.ssim_statement(gt[..., 0], pred[..., 0], 1).cpu().numpy()
    assert np.max(np.abs(got["ssim"] - want)) < 1e-5
    assert np.isfinite(got["ssim"]).all()


def test_ssim_kernel_known_answers():
    from enerf_amd import evaluate as E
    x = torch.rand(2, 19, 23, 1, device=DEV)
    m = E.metrics(x, x.clone(), False)
    assert np.abs(m["ssim"] - 1).max() < 1e-12 and (m["sse"] == 0).all()
    c = torch.full((1, 8, 8, 3), 0.25, device=DEV)
    assert E.metrics(c, c.clone(), False)["ssim"][0] == 1.0


# ----------------------------------------------------------------------------------------------------- end to end
def _scene_views(V, C, seed, step=10):
    """V synthetic cameras of enerf_amd/scene.py, every `step`-th pixel: 48 x 64 views, random gt."""
    from enerf_amd import scene
    H, W = scene.H // step, scene.W // step
    j, i = torch.meshgrid(torch.arange(H, device=DEV) * step, torch.arange(W, device=DEV) * step, indexing="ij")
    inds = (j * scene.W + i).reshape(-1)
    g = torch.Generator().manual_seed(seed)
    views = []
    for k in range(V):
        ro, rd = scene.pixel_rays(scene.pose(5 * k), inds, DEV)
        views.append({"rays_o": ro, "rays_d": rd, "images": torch.rand(1, H, W, C, generator=g), "H": H, "W": W})
    return views


class StandInEMA:
    def __init__(self, model):
        self.model, self.calls, self.saved = model, [], None

    def store(self):
        self.calls.append("store")
        self.saved = [p.detach().clone() for p in self.model.parameters()]

    def copy_to(self):
        self.calls.append("copy_to")

    def restore(self):
        self.calls.append("restore")
        for p, s in zip(self.model.parameters(), self.saved):
            p.data.copy_(s)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("event_only,C", [(False, 3), (True, 1), (True, 3)], ids=["rgb3", "events1", "events3"])
def test_harness_evaluate_end_to_end(fp16, event_only, C):
    from enerf_amd import evaluate as E, stratified
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    torch.manual_seed(3)
    model = NeRFNetwork(encoding="hashgrid", bound=1, cuda_ray=False, out_dim_color=C)
    det_fill_(list(model.parameters()), 3, -0.5, 0.5)
    model = model.to(DEV)
    h = TrainHarness(model, fp16=fp16)
    views = _scene_views(3, C, seed=11)
    opt = ap.Namespace(event_only=event_only, out_dim_color=C, color_space="srgb", render_kwargs={"num_steps": 64})
    model.train()
    assert "mlp_precision" not in model.__dict__
    ema = StandInEMA(model)
    calls = stratified.stats["calls"]
    r = h.evaluate(views, opt, ema=ema)
    assert stratified.stats["calls"] - calls >= len(views)            # the native route served every render
    assert model.training and "mlp_precision" not in model.__dict__
    assert ema.calls == ["store", "copy_to", "restore"]
    # the same renders, the torch statement on them (on the device)
    model.eval()
    pred, gt, _, _ = E._in_regime(h, lambda: E.render_views(h, views, opt))
    model.train()
    cpu = E.summarize(E._metrics_statement(pred, gt, event_only), pred.shape[1], pred.shape[2], C, event_only)
    assert abs(r["valid_loss"] - cpu["valid_loss"]) <= 1e-12 * cpu["valid_loss"]
    assert abs(r["psnr_meter"] - cpu["psnr_meter"]) < 1e-9
    if event_only:
        assert _rel(r["a"], cpu["a"]) < 1e-9 and _rel(r["b"], cpu["b"]) < 1e-9
        np.testing.assert_allclose(r["psnr_corrected"], cpu["psnr_corrected"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(r["ssim_corrected"], cpu["ssim_corrected"], rtol=0, atol=1e-5)
    else:
        np.testing.assert_allclose(r["psnr"], cpu["psnr"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(r["ssim"], cpu["ssim"], rtol=0, atol=1e-5)
