"""Host-side checks of the closed-form frame term (no GPU): frame_term.frame_term_statement against the reference's lines
written out under autograd (nerf/utils.py:595-604, 634, and the weight of :546), in fp64; the new entry point is declared,
bound and exported; and the route predicates of TrainHarness.closed_frames -- off by default, and with it on, every regime
the closed route does not serve keeps the step where it was."""
import argparse as ap
import ctypes
import os
import re

import pytest
import torch


def _reference_lines(out_image, images, bg_color, weight, C):
    """Trainer.train_step's ground truth, per-ray loss and mean; train_step_events' weight on the term."""
    pred_rgb = out_image.clone().requires_grad_(True)
    if images.shape[-1] == C + 1:
        gt_rgb = images[..., :C] * images[..., C:] + bg_color * (1 - images[..., C:])
    else:
        gt_rgb = images
    criterion = torch.nn.MSELoss(reduction="none")
    loss = criterion(pred_rgb, gt_rgb).mean(-1)
    total = weight * loss.mean()
    total.backward()
    return gt_rgb, loss.detach(), total.detach(), pred_rgb.grad


@pytest.mark.parametrize("weight", [1.0, 0.3])
@pytest.mark.parametrize("form", ["scalar", "shared", "per_ray"])
@pytest.mark.parametrize("alpha", [False, True])
@pytest.mark.parametrize("C", [1, 3])
def test_statement_equals_the_reference_lines_under_autograd(C, alpha, form, weight):
    from enerf_amd.frame_term import frame_term_statement
    g = torch.Generator().manual_seed(7 + C)
    B, N = 2, 37
    out = torch.rand(B, N, C, generator=g, dtype=torch.float64)
    images = torch.rand(B, N, C + int(alpha), generator=g, dtype=torch.float64)
    bg = {"scalar": 0.3, "shared": torch.rand(C, generator=g, dtype=torch.float64),
          "per_ray": torch.rand(B, N, C, generator=g, dtype=torch.float64)}[form]
    want = _reference_lines(out, images, bg, weight, C)
    got = frame_term_statement(out, images, bg, weight)
    assert got[1].shape == (B, N) and got[3].shape == out.shape
    for name, a, b in zip(("gt", "err", "loss", "g_out_image"), got, want):
        assert a.dtype == torch.float64, name
        assert float((a - b).abs().max()) <= 1e-12, name
    assert float(got[3].abs().max()) > 0


def test_frames_entry_point_is_declared_bound_and_exported():
    from enerf_amd import _lib
    name = "enerf_composite_rays_train_fwd_bwd_frames_c"
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "enerf_hip.h")).read()
    assert re.search(r"\bint %s\(" % name, header)
    u32, f32, vp = _lib._u32, _lib._f32, _lib._vp
    mse = _lib.SIGNATURES["enerf_composite_rays_train_fwd_bwd_mse_c"]
    # the MSE form's arguments with (target, grad_scale) replaced by (pixels, pix_stride, weight, gt_out, err_out)
    assert mse[12:14] == [vp, f32]
    assert _lib.SIGNATURES[name] == mse[:12] + [vp, u32, f32, vp, vp] + mse[14:]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    from enerf_amd.backends import _raymarching
    assert callable(_raymarching.composite_rays_train_fwd_bwd_frames)


# ------------------------------------------------------------------------------------------------ the route predicates
class _Routes:
    """A CPU harness whose two frame routes only record that they were taken, with fused_render.supported replaced by
    the one rule of it a CPU model can show (no background model): what is under test is the harness's own decision."""

    def __init__(self, monkeypatch, **harness_kw):
        from enerf_amd import fused_render
        from enerf_amd.network import NeRFNetwork
        from enerf_amd.trainer import TrainHarness
        model = NeRFNetwork(encoding="frequency", encoding_dir="frequency", bound=3, cuda_ray=False, out_dim_color=1)
        self.h = h = TrainHarness(model, lr=5e-3, **harness_kw)
        model.cuda_ray = True                       # (after the harness: no occupancy is installed on a CPU model)
        monkeypatch.setattr(fused_render, "supported", lambda m, ro, rd, bg, gamma: m.bg_radius <= 0)
        self.taken = []
        per_ray = lambda ro: torch.zeros(ro.shape[:-1])
        monkeypatch.setattr(h, "_step_frames_closed", lambda ro, *a: (self.taken.append("closed"), per_ray(ro))[1])
        monkeypatch.setattr(h, "_step_frames", lambda ro, *a: (self.taken.append("autograd"), per_ray(ro))[1])
        g = torch.Generator().manual_seed(1)
        self.batch = {"rays_o": torch.rand(1, 8, 3, generator=g), "rays_d": torch.rand(1, 8, 3, generator=g),
                      "images": torch.rand(1, 8, 2, generator=g)}

    def route(self, render_kwargs=None):
        del self.taken[:]
        self.h.step_frames(self.batch, ap.Namespace(out_dim_color=1, color_space="srgb", render_kwargs=render_kwargs or {}))
        assert len(self.taken) == 1
        return self.taken[0]

    def events_ok(self, **kw):
        from enerf_amd.events import EventOptions
        b = self.batch
        data = dict(b, rays_evs_o1=b["rays_o"], rays_evs_d1=b["rays_d"], images=b["images"][..., :1].contiguous())
        return bool(self.h._events_manual_ok(data, EventOptions(out_dim_color=1, use_luma=False, **kw)))


def test_switch_is_off_by_default_and_on_takes_the_closed_routes(monkeypatch):
    r = _Routes(monkeypatch)
    assert r.h.closed_frames is False
    assert r.route() == "autograd"
    assert r.events_ok(event_only=True) and not r.events_ok(event_only=False)
    r.h.closed_frames = True
    assert r.route() == "closed"
    assert r.route({"dt_gamma": 0.0, "max_steps": 512, "out_dim_color": 1}) == "closed"
    assert r.events_ok(event_only=True) and r.events_ok(event_only=False)


@pytest.mark.parametrize("regime", ["fp16", "amp_f16", "amp_bf16", "strat_f16", "avg", "graphs", "graph_counter",
                                    "bg_radius", "render_kwargs", "manual_mse"])
def test_switch_on_keeps_the_old_route_where_the_closed_one_does_not_serve(monkeypatch, regime):
    r = _Routes(monkeypatch)
    h = r.h
    h.closed_frames = True
    assert r.route() == "closed" and r.events_ok(event_only=False)
    kw = None
    if regime in ("fp16", "amp_f16", "amp_bf16", "strat_f16"):
        setattr(h, regime, True)
        monkeypatch.setattr(h, "_strat_f16_step", lambda fn, native, *a: fn(*a))
        monkeypatch.setattr(h, "_strat_f16_ok", lambda *a: False)
        monkeypatch.setattr(h, "_amp_scope", lambda: None)
        monkeypatch.setattr(h, "_amp_restore", lambda prev: None)
    elif regime == "avg":
        h.avg = object()
    elif regime == "graphs":
        h.use_graphs = True
    elif regime == "graph_counter":
        h.model.graph_counter = torch.zeros(2, dtype=torch.int32)
    elif regime == "bg_radius":
        h.model.bg_radius = 1.0
    elif regime == "manual_mse":
        h.manual_mse = False
    else:
        kw = {"upsample_steps": 0}
    assert r.route(kw) == "autograd"
    assert not r.events_ok(event_only=False, render_kwargs=kw or {})
    if regime not in ("bg_radius", "render_kwargs", "manual_mse"):
        assert r.events_ok(event_only=True)                     # the event-only route is decided as it was
