"""The marching route (cuda_ray = True) at 1 and 2 colour channels: NeRFNetwork(out_dim_color = 1) -- what every shipped
event-training config sets -- renders, trains and evaluates on the kernels the three-channel model uses.  Each check
mirrors a three-channel test of tests/test_gpu_training.py / test_gpu_baseline_configs.py (named in its docstring), with
that test's ray counts and tolerances; none of this could run before the compositing kernels took a channel count."""
import argparse as ap
import contextlib
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _model(C, bound=2, seed=0):
    from enerf_amd.network import NeRFNetwork
    torch.manual_seed(seed)
    return NeRFNetwork(encoding="hashgrid", bound=bound, cuda_ray=True, out_dim_color=C).to(DEV)


def _batches(n, n_rays, C, seed=11):
    """test_gpu_training._batches with the target cut to C channels."""
    from enerf_amd import scene
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for b in range(n):
        (ro, rd), _ = scene.training_batch(b, n_rays, DEV, generator=g)
        b_ = (ro * rd).sum(-1)
        disc = b_ ** 2 - ((ro * ro).sum(-1) - 0.36)
        t = -b_ - torch.sqrt(disc.clamp(min=0))
        p = ro + rd * t.unsqueeze(-1)
        tgt = torch.where((disc > 0).unsqueeze(-1), scene.analytic_color(p).clamp(0, 1), torch.ones_like(p))
        out.append((ro, rd, tgt[..., :C].contiguous()))
    return out


def _event_batch_of(data, i):
    ro, rd, tg = data[i % len(data)]
    ro2, rd2, _ = data[(i + 1) % len(data)]
    return {"images": tg.view(1, -1, tg.shape[-1]), "rays_evs_o1": ro.view(1, -1, 3), "rays_evs_d1": rd.view(1, -1, 3),
            "rays_evs_o2": ro2.view(1, -1, 3), "rays_evs_d2": rd2.view(1, -1, 3),
            "pols": torch.sign(tg[..., 0] - 0.5).view(1, -1)}


def _gray_options(**kw):
    """The shipped loss settings."""
    from enerf_amd.events import EventOptions
    return EventOptions(**dict(dict(out_dim_color=1, use_luma=False, linlog=True, C_thres=0.2, event_only=True), **kw))


@contextlib.contextmanager
def _counting(module, name, calls):
    orig = getattr(module, name)
    setattr(module, name, lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    try:
        yield
    finally:
        setattr(module, name, orig)


@contextlib.contextmanager
def _mlp_precision(mode):
    from enerf_amd import _lib
    prev = _lib.lib().enerf_mlp32_precision(mode)
    try:
        yield
    finally:
        _lib.lib().enerf_mlp32_precision(prev)


# ------------------------------------------------------------------------------------------------------- the render
@pytest.mark.parametrize("bg", ["none", "scalar", "tensor", "per_ray"])
@pytest.mark.parametrize("mean_count", [-1, 40000])
@pytest.mark.parametrize("C", [1, 2])
def test_fused_render_node_matches_op_by_op_route(monkeypatch, C, mean_count, bg):
    """test_gpu_training.test_fused_render_node_matches_op_by_op_route at C channels: the fused node against _train_ops,
    with a scalar, one colour and one colour per ray as background."""
    from enerf_amd import fused_network, fused_render, scene
    model = _model(C)
    model.encoder.embeddings.data.uniform_(-0.5, 0.5)
    scene.install_occupancy(model)
    model.train()
    g = torch.Generator(device=DEV).manual_seed(5)
    (ro, rd), _ = scene.training_batch(0, 3000, DEV, generator=g)
    ro, rd = ro.view(1, -1, 3), rd.view(1, -1, 3)
    gi = torch.randn(3000, C, device=DEV)
    bg_color = {"none": None, "scalar": 0.25, "tensor": torch.rand(1, 1, C, device=DEV),
                "per_ray": torch.rand(1, 3000, C, device=DEV)}[bg]
    calls = []
    orig = fused_render.render_train
    monkeypatch.setattr(fused_render, "render_train", lambda *a: (calls.append(1), orig(*a))[1])

    def run(fused):
        monkeypatch.setattr(fused_render, "ENABLED", fused)
        monkeypatch.setattr(fused_network, "ENABLED", fused)
        model.zero_grad()
        model.local_step = 0
        model.step_counter.zero_()
        model.mean_count = mean_count
        out = model.render(ro, rd, staged=False, bg_color=bg_color, perturb=True)
        assert out["image"].shape == (1, 3000, C)
        (out["image"].reshape(-1, C) * gi).sum().backward()
        return (out["image"].detach().reshape(-1, C), out["depth"].detach().reshape(-1), model.step_counter[0].clone(),
                {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})

    im1, dp1, c1, g1 = run(True)
    assert len(calls) == 1
    im0, dp0, c0, g0 = run(False)
    assert len(calls) == 1
    assert torch.equal(c1, c0)
    assert float((im1 - im0).abs().max()) < 2e-5
    assert float((dp1 - dp0).abs().max()) < 2e-5
    assert set(g1) == set(g0) and float(im0.std()) > 0.01
    for n in g0:
        assert float((g1[n] - g0[n]).abs().max()) <= 2e-4 * float(g0[n].abs().max()) + 1e-9, n


# ------------------------------------------------------------------------------------------------------- RGB steps
def test_manual_mse_step_matches_autograd_step(monkeypatch):
    """test_gpu_training.test_manual_mse_step_matches_autograd_step on a one-channel model and [N,1] targets."""
    from enerf_amd import fused_render
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 2048, 1)
    calls = []
    orig, orig_native = fused_render.train_step_mse, fused_render.train_step_native
    monkeypatch.setattr(fused_render, "train_step_mse", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    monkeypatch.setattr(fused_render, "train_step_native", lambda *a, **k: (calls.append(1), orig_native(*a, **k))[1])
    runs = []
    for manual in (False, True):
        model = _model(1)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        h.manual_mse = manual
        losses = [h.step_rgb(*data[i % len(data)]).clone() for i in range(40)]
        runs.append((torch.stack(losses).cpu(), model.step_counter.clone().cpu(),
                     {n: p.detach().clone() for n, p in model.named_parameters()}))
        assert len(calls) == (40 if manual else 0)
    (l0, c0, p0), (l1, c1, p1) = runs
    assert torch.equal(c0, c1)
    for n in p0:
        assert float((p0[n] - p1[n]).abs().mean()) <= 1e-3 * float(p0[n].abs().mean()), n
    rel = ((l0 - l1).abs() / l0.abs().clamp(min=1e-9))
    assert float(rel[:10].max()) < 5e-6, rel.tolist()
    assert float(rel.max()) < 3e-4, rel.tolist()


def test_native_step_call_equals_the_python_driven_step():
    """test_gpu_training.test_native_step_call_equals_the_python_driven_step at out_c = 1: enerf_train_step_mse with
    target / image [N,1]."""
    from enerf_amd import fused_render
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 4096, 1)
    runs = {}
    for native in (True, False):
        model = _model(1)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        h.native_step = native
        calls, losses, counters = [], [], []
        with _counting(fused_render, "train_step_native", calls):
            for i in range(40):
                nxt = data[(i + 1) % 4]
                losses.append(float(h.step_rgb(*data[i % 4], next_rays=(nxt[0], nxt[1]))))
                counters.append(model.step_counter[model.rendered_counter_slot].cpu().clone())
        torch.cuda.synchronize()
        runs[native] = (losses, torch.stack(counters), {n: p.detach().clone() for n, p in model.named_parameters()},
                        len(calls), {n for n, p in model.named_parameters() if p.grad is not None})
    (la, ca, pa, na, ga), (lb, cb, pb, nb, gb) = runs[True], runs[False]
    assert na == 39 and nb == 0
    assert torch.equal(ca, cb)
    assert np.abs(np.array(la) - np.array(lb)).max() <= 1e-5 * np.abs(lb).max()
    for n, a in pa.items():
        assert float((a - pb[n]).abs().mean()) <= 1e-4 * float(pb[n].abs().mean()) + 1e-9, n
    assert ga == gb


def test_training_reduces_loss():
    """test_gpu_training.test_training_reduces_loss's criterion on the one-channel model."""
    from enerf_amd.trainer import TrainHarness
    model = _model(1)
    h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
    data = _batches(8, 2048, 1)
    losses = []
    for i in range(160):
        ro, rd, tgt = data[i % len(data)]
        losses.append(float(h.step_rgb(ro, rd, tgt).detach()))
    first, last = np.mean(losses[:8]), np.mean(losses[-8:])
    assert np.isfinite(losses).all()
    assert last < 0.5 * first, (first, last)
    assert model.mean_count > 0 and model.iter_density == math.ceil(160 / 16)


def test_step_frames_takes_a_per_pixel_background():
    """TrainHarness.step_frames on a one-channel model: alpha images on a per-pixel [B,N,1] background land on the fused
    render node, as their three-channel form does."""
    from enerf_amd import fused_render
    from enerf_amd.trainer import TrainHarness
    model = _model(1)
    h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
    (ro, rd, tgt), = _batches(1, 2048, 1)
    images = torch.cat([tgt, torch.rand_like(tgt)], -1)                # grey + alpha
    calls = []
    with _counting(fused_render, "render_train", calls):
        losses = [float(h.step_frames({"rays_o": ro, "rays_d": rd, "images": images},
                                      ap.Namespace(out_dim_color=1, color_space="srgb", render_kwargs={})))
                  for _ in range(20)]
    assert len(calls) == 20 and np.isfinite(losses).all() and losses[-1] < losses[0]


# ----------------------------------------------------------------------------------------------------- event steps
def test_event_step_with_closed_render_backward_matches_autograd_step(monkeypatch):
    """test_gpu_training.test_event_step_with_closed_render_backward_matches_autograd_step with the shipped grayscale
    settings (out_dim_color = 1, use_luma = 0): the fused event loss runs on [N,1] images."""
    from enerf_amd import events, fused_render
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 2048, 1)
    opt = _gray_options()
    calls, fused_loss = [], []
    orig = events.train_step_events_manual
    monkeypatch.setattr(events, "train_step_events_manual", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    orig_native = fused_render.train_step_events_native
    monkeypatch.setattr(fused_render, "train_step_events_native",
                        lambda *a, **k: (calls.append(1), orig_native(*a, **k))[1])
    orig_loss = events.event_loss_with_grads
    monkeypatch.setattr(events, "event_loss_with_grads",
                        lambda a, *r: (fused_loss.append(tuple(a.shape)), orig_loss(a, *r))[1])
    runs = []
    for manual in (False, True):
        model = _model(1)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        h.manual_mse = manual
        torch.manual_seed(3)                                   # the step draws a random background colour
        losses = [h.step_events(_event_batch_of(data, i), opt,
                                next_data=_event_batch_of(data, i + 1) if manual else None).clone() for i in range(40)]
        runs.append((torch.stack(losses).cpu(), model.step_counter.clone().cpu(),
                     {n: p.detach().clone() for n, p in model.named_parameters()}))
        assert len(calls) == (40 if manual else 0)
    assert fused_loss and set(fused_loss) == {(1, 2048, 1)}    # the Python-driven steps of the cold window
    (l0, c0, p0), (l1, c1, p1) = runs
    assert torch.equal(c0, c1)
    assert float(((l0 - l1).abs() / l0.abs().clamp(min=1e-9)).max()) < 2e-4
    for n in p0:
        assert float((p0[n] - p1[n]).abs().mean()) <= 2e-3 * float(p0[n].abs().mean()), n


def test_native_event_step_call_equals_the_python_driven_event_step():
    """test_gpu_training.test_native_event_step_call_equals_the_python_driven_event_step with the shipped grayscale
    settings: enerf_train_step_events at out_c = 1."""
    from enerf_amd import fused_render
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 4096, 1)
    opt = _gray_options()
    runs = {}
    for native in (True, False):
        model = _model(1)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        h.native_step = native
        calls = []
        with _counting(fused_render, "train_step_events_native", calls):
            torch.manual_seed(3)
            losses = [h.step_events(_event_batch_of(data, i), opt, next_data=_event_batch_of(data, i + 1)).clone()
                      for i in range(40)]
        torch.cuda.synchronize()
        if native:
            assert int(model._native_events_ctx["a"].out_c) == 1
        runs[native] = (torch.stack(losses).cpu(), model.step_counter.clone().cpu(),
                        {n: p.detach().clone() for n, p in model.named_parameters()}, len(calls),
                        {n for n, p in model.named_parameters() if p.grad is not None})
    (la, ca, pa, na, ga), (lb, cb, pb, nb, gb) = runs[True], runs[False]
    assert na >= 24 and nb == 0
    assert torch.equal(ca, cb)
    assert float(((la - lb).abs() / lb.abs().clamp(min=1e-9)).max()) <= 1e-5
    for n, a in pa.items():
        assert float((a - pb[n]).abs().mean()) <= 1e-4 * float(pb[n].abs().mean()) + 1e-9, n
    assert ga == gb


def test_luma_options_on_a_one_channel_model_do_not_reach_the_one_call_step():
    from enerf_amd import fused_render
    from enerf_amd.trainer import TrainHarness
    model = _model(1)
    h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
    model.mean_count = 40000
    data = _event_batch_of(_batches(2, 2048, 1), 0)
    assert fused_render.native_events_supported(model, data, _gray_options(), h.opt)
    assert not fused_render.native_events_supported(model, data, _gray_options(use_luma=True), h.opt)
    assert not fused_render.native_events_supported(model, data, _gray_options(out_dim_color=3), h.opt)


@pytest.mark.parametrize("variant", ["normalised", "negative_event_sampling"])
def test_unfused_losses_run_on_the_manual_route_and_match_autograd(monkeypatch, variant):
    """C_thres = -1 (the normalised loss) and --negative_event_sampling stay in torch; their renders are the closed-form
    one-channel ones.  Tolerances: test_event_step_with_negative_event_sampling_closed_form_matches_autograd's."""
    from enerf_amd import events
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 2048, 1)
    calls = []
    orig = events.train_step_events_manual
    monkeypatch.setattr(events, "train_step_events_manual", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])

    def batch(i):
        b = _event_batch_of(data, i)
        if variant == "negative_event_sampling":
            v = lambda x: x.view(1, -1, 3)[:, :1024].contiguous()
            (ro3, rd3, _), (ro4, rd4, _) = data[(i + 2) % 4], data[(i + 3) % 4]
            b.update(rays_no_evs_o1=v(ro3), rays_no_evs_d1=v(rd3), rays_no_evs_o2=v(ro4), rays_no_evs_d2=v(rd4))
        return b

    if variant == "normalised":
        opt = _gray_options(C_thres=-1)
    else:
        opt = _gray_options(C_thres=0.05, negative_event_sampling=True, w_no_ev=5.0, epoch=2, epoch_start_noEvLoss=0)
    runs = []
    for manual in (False, True):
        model = _model(1)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        h.manual_mse = manual
        torch.manual_seed(3)
        losses = [h.step_events(batch(i), opt).clone() for i in range(24)]
        runs.append((torch.stack(losses).cpu(), model.step_counter.clone().cpu(),
                     {n: p.detach().clone() for n, p in model.named_parameters()}))
        assert len(calls) == (24 if manual else 0)
    (l0, c0, p0), (l1, c1, p1) = runs
    assert torch.equal(c0, c1)
    rel = (l0 - l1).abs() / l0.abs().clamp(min=1e-9)
    assert float(rel[:4].max()) < 1e-5 and float(rel.max()) < 3e-4, rel.tolist()
    for n in p0:
        assert float((p0[n] - p1[n]).abs().mean()) <= 2e-3 * float(p0[n].abs().mean()), n


def test_fp16_closed_form_event_step_runs_under_the_scaler():
    """test_gpu_training.test_fp16_closed_form_event_step_runs_under_the_scaler with the shipped grayscale settings."""
    from enerf_amd.trainer import TrainHarness
    from test_gpu_baseline_configs import _event_batch
    model = _model(1)
    h = TrainHarness(model, lr=1e-2, occupancy="synthetic", fp16=True)
    opt = _gray_options()
    data = _event_batch(4096, DEV)
    losses = [float(h.step_events(data, opt)) for _ in range(40)]
    assert h.amp_f16 and np.isfinite(losses).all() and losses[-1] < losses[0]
    assert float(h.scaler.get_scale()) >= 256.0 and h.amp_skipped_steps() <= 8


# ------------------------------------------------------------------------------------------------------- inference
def test_frame_schedule_equals_round_schedule():
    """test_gpu_baseline_configs.test_frame_schedule_equals_round_schedule_fp32_nets on a one-channel model."""
    from enerf_amd import frame, scene
    model = _model(1, bound=3, seed=2).eval()
    model.encoder.embeddings.data.uniform_(-1, 1)
    scene.install_occupancy(model)
    g = torch.Generator(device=DEV).manual_seed(4)
    (ro, rd), _ = scene.training_batch(2, 20000, DEV, generator=g)
    ro, rd = ro[0].contiguous(), rd[0].contiguous()
    bg = torch.rand(1, device=DEV)
    with torch.no_grad():
        d1, i1 = frame.render_frame(model, ro, rd, bg)
        d0, i0 = frame.render_rounds(model, ro, rd, bg)
        out = model.render(ro[None], rd[None], staged=False, bg_color=bg, perturb=False)
    assert i1.shape == i0.shape == (20000, 1)
    assert float((i1 - i0).abs().max()) < 2e-6 and float(((i1 - i0).abs() > 0).float().mean()) < 2e-3
    dd = (d1 - d0).abs()
    assert float(dd[torch.isfinite(dd)].max()) < 2e-6
    assert torch.equal(out["image"].view(-1, 1), i1)
    assert float(i1.std()) > 0.01


def test_one_channel_model_equals_three_channel_model_with_its_row_three_times():
    """A C = 1 model against a C = 3 model whose last colour layer is the C = 1 row three times, in the exact-fp32
    arithmetic mode: train and eval images agree per channel to 1e-5 (the bound tests/test_gpu_stratified.py holds two
    routes into the same networks to), and under a loss that weights the channels equally the C = 1 last-layer gradient
    is the sum of the three rows' (bound: the fused node's against the op-by-op route, 2e-4 of the largest entry)."""
    from enerf_amd import scene
    m1, m3 = _model(1), _model(3)
    with torch.no_grad():
        for (n, p1), (_, p3) in zip(m1.named_parameters(), m3.named_parameters()):
            if p1.shape == p3.shape:
                p3.copy_(p1)
            else:
                assert n == "color_net.2.weight" and p1.shape == (1, 64)
                p3.copy_(p1.expand(3, -1))
    for m in (m1, m3):
        m.encoder.embeddings.data.uniform_(-0.5, 0.5)
        scene.install_occupancy(m)
    m3.encoder.embeddings.data.copy_(m1.encoder.embeddings.data)
    g = torch.Generator(device=DEV).manual_seed(5)
    (ro, rd), _ = scene.training_batch(0, 3000, DEV, generator=g)
    gi = torch.randn(1, 3000, 1, device=DEV)
    with _mlp_precision(0):
        m1.train(), m3.train()
        o1 = m1.render(ro, rd, staged=False, bg_color=0.25, perturb=False)
        o3 = m3.render(ro, rd, staged=False, bg_color=0.25, perturb=False)
        (o1["image"] * gi).sum().backward()
        (o3["image"] * (gi / 3)).sum().backward()
        m1.eval(), m3.eval()
        with torch.no_grad():
            e1 = m1.render(ro, rd, staged=False, bg_color=0.25, perturb=False)
            e3 = m3.render(ro, rd, staged=False, bg_color=0.25, perturb=False)
    assert o1["image"].shape == (1, 3000, 1) and o3["image"].shape == (1, 3000, 3)
    for a, b in ((o1, o3), (e1, e3)):
        assert float((b["image"] - a["image"]).abs().max()) <= 1e-5            # every channel against the one
        assert float((b["depth"] - a["depth"]).abs().max()) <= 1e-5
        assert float(a["image"].std()) > 0.01
    g1, g3 = m1.color_net[2].weight.grad, m3.color_net[2].weight.grad
    assert float(g1.abs().max()) > 0
    assert float((g3.sum(0, keepdim=True) - g1).abs().max()) <= 2e-4 * float(g1.abs().max()) + 1e-9
    # and what lies below the last layer sees the same gradient
    ge1, ge3 = m1.encoder.embeddings.grad, m3.encoder.embeddings.grad
    assert float((ge3 - ge1).abs().max()) <= 2e-4 * float(ge1.abs().max()) + 1e-9


def test_harness_evaluate_returns_the_psnr_of_the_models_renders():
    """TrainHarness.evaluate on two 16 x 12 views of a one-channel marching model: the PSNR per view is the one torch
    computes from model.render's image (fp64 mean of squares; 1e-6 dB is 2e-7 of the mean: a few fp32 roundings)."""
    from enerf_amd import scene
    from enerf_amd.trainer import TrainHarness
    model = _model(1)
    model.encoder.embeddings.data.uniform_(-0.5, 0.5)
    h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
    step = 40
    H, W = scene.H // step, scene.W // step
    assert (W, H) == (16, 12)
    j, i = torch.meshgrid(torch.arange(H, device=DEV) * step, torch.arange(W, device=DEV) * step, indexing="ij")
    inds = (j * scene.W + i).reshape(-1)
    g = torch.Generator().manual_seed(11)
    views = []
    for k in range(2):
        ro, rd = scene.pixel_rays(scene.pose(5 * k), inds, DEV)
        views.append({"rays_o": ro, "rays_d": rd, "images": torch.rand(1, H, W, 1, generator=g), "H": H, "W": W})
    opt = ap.Namespace(event_only=False, out_dim_color=1, color_space="srgb", render_kwargs={})
    r = h.evaluate(views, opt)
    model.eval()
    want = []
    with torch.no_grad():
        for v in views:
            img = model.render(v["rays_o"], v["rays_d"], staged=True, bg_color=1, perturb=False)["image"]
            assert img.shape[-1] == 1
            mse = ((img.reshape(H, W, 1).double() - v["images"][0].to(DEV).double()) ** 2).mean()
            want.append(float(-10 * torch.log10(mse)))
    np.testing.assert_allclose(r["psnr"], want, rtol=0, atol=1e-6)
    assert np.std(want) > 0 or want[0] != want[1]
