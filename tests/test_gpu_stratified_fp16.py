"""The stratified sampler's fp16 regime (enerf_amd/stratified.py with mlp_precision 3): its
rounding points read back from the route's own buffers, the same regime restated by the PyTorch statement under autocast,
training through TrainHarness(fp16=True) against the autocast route, loss scaling, a CUDA-graph capture, the fallbacks
and checkpoints."""
import contextlib
import types

import numpy as np
import pytest
import torch

from util import det_fill_

pytestmark = pytest.mark.gpu
DEV = "cuda"


@contextlib.contextmanager
def route(on):
    from enerf_amd import stratified
    prev = stratified.ENABLED
    stratified.ENABLED = on
    try:
        yield
    finally:
        stratified.ENABLED = prev


@contextlib.contextmanager
def keep_last():
    from enerf_amd import stratified
    stratified.KEEP_LAST = True
    try:
        yield stratified
    finally:
        stratified.KEEP_LAST = False
        stratified.last = None


@contextlib.contextmanager
def fp16_regime(model):
    """Evaluation / a bare render in the regime: the model's own mlp_precision, as the documentation says."""
    model.mlp_precision = 3
    try:
        yield
    finally:
        model.__dict__.pop("mlp_precision", None)


def _model(C, bound, seed):
    """Deterministic weights small enough that the rays are neither empty nor saturated at their first sample."""
    from enerf_amd.network import NeRFNetwork
    torch.manual_seed(seed)
    model = NeRFNetwork(encoding="hashgrid", bound=bound, cuda_ray=False, out_dim_color=C)
    det_fill_(list(model.parameters()), seed, -0.5, 0.5)
    return model.to(DEV)


def _hit_rays(n, seed, bound):
    """n rays from outside the box towards points inside it."""
    g = np.random.default_rng(seed)
    v = g.normal(size=(n, 3))
    o = (bound + 1.5) * v / np.linalg.norm(v, axis=1, keepdims=True)
    d = g.uniform(-0.75 * bound, 0.75 * bound, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    f = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV)  # noqa: E731
    return f(o), f(d)


def _h16(x):
    return x.contiguous().view(torch.int16)


def _i32(x):
    return x.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------ 1. rounding
@pytest.mark.parametrize("C", [1, 3])
def test_rounding_points_exact(C):
    from enerf_amd import shencoder
    N, T = 2048, 128
    model = _model(C, 2, 5).train()
    ro, rd = _hit_rays(N, 7, 2)
    with keep_last() as strat, fp16_regime(model):
        calls = strat.stats["calls"]
        out = model.render(ro, rd, staged=False, bg_color=None, perturb=True, num_steps=T, upsample_steps=0,
                           out_dim_color=C)
        assert strat.stats["calls"] == calls + 1
        last = strat.last
    assert out["image"].dtype == torch.float32 and torch.isfinite(out["image"]).all()
    count = last["count"].long()
    total = int(last["incl"][-1])
    assert total == int(count.sum()) and total > N, f"{total} masked samples"
    cin, rgb, h16, sigma = last["cin"][:total], last["rgb"], last["h16"], last["sigma"]
    assert cin.dtype == torch.float16 and cin.shape[1] == 32
    # SH columns: the library's half SH encoder on the half-rounded directions, bit for bit
    sh = shencoder.sh_encode(rd.half(), 4)
    assert sh.dtype == torch.float16
    ray = torch.repeat_interleave(torch.arange(N, device=DEV), count)
    assert torch.equal(_h16(cin[:, 16:32]), _h16(sh[ray]))
    # geo_feat columns: fp16 values (the sigma net's outputs rounded at mode 3), those of the masked samples in order
    mask = (last["w"] > 1e-4).reshape(-1)
    geo = h16[mask][:, 1:16]
    assert torch.equal(_i32(geo), _i32(geo.half().float()))
    assert torch.equal(_h16(cin[:, 1:16]), _h16(geo.half()))
    assert torch.equal(_h16(cin[:, :1]), torch.zeros_like(_h16(cin[:, :1])))
    # sigma = trunc_exp of the fp16 h0 in fp32 (activation.py: torch.exp of x.float(); no clamp below 15 either way)
    h0 = h16[:, 0]
    assert torch.equal(_i32(h0), _i32(h0.half().float()))
    assert float(h0.max()) < 15.0
    assert torch.equal(_i32(sigma), _i32(torch.exp(torch.clamp(h0, max=15.0))))
    assert rgb.dtype == torch.float16


# ------------------------------------------------------------------------------------------------------ 2. restated
def _no_half_table(monkeypatch):
    """The statement's only rounding point the regime leaves out: the grid wrapper's half copy of the table."""
    from enerf_amd import gridencoder
    class _Torch(types.ModuleType):
        def __getattr__(self, name):
            return getattr(torch, name)

    proxy = _Torch("torch")
    proxy.is_autocast_enabled = lambda *a, **k: False
    monkeypatch.setattr(gridencoder, "torch", proxy)


def _run(model, ro, rd, bg, T, native, monkeypatch):
    from enerf_amd import stratified
    model.zero_grad(set_to_none=True)
    calls = stratified.stats["calls"]
    torch.manual_seed(4)                                   # the same jitter on both arms
    if native:
        with fp16_regime(model):
            out = model.render(ro, rd, staged=False, bg_color=bg, perturb=True, num_steps=T, upsample_steps=0,
                               out_dim_color=model.out_dim_color)
            ((out["image"] ** 2).sum() + out["depth"].sum()).backward()
    else:
        with monkeypatch.context() as mp:
            _no_half_table(mp)
            with torch.autocast("cuda", dtype=torch.float16):
                out = model.render(ro, rd, staged=False, bg_color=bg, perturb=True, num_steps=T, upsample_steps=0,
                                   out_dim_color=model.out_dim_color)
                loss = (out["image"].float() ** 2).sum() + out["depth"].float().sum()
            loss.backward()
    assert stratified.stats["calls"] == calls + (1 if native else 0)
    grads = {n: (p.grad.detach().float().clone() if p.grad is not None else torch.zeros_like(p)) for n, p in
             model.named_parameters()}
    return out["image"].detach().float(), out["depth"].detach().float(), grads


@pytest.mark.parametrize("bound", [2, 3])
@pytest.mark.parametrize("C", [1, 3])
def test_against_the_regime_restated_by_the_statement(C, bound, monkeypatch):
    """Native fp16 vs the statement under autocast with an fp32 table, identical weights, rays, jitter and per-ray
    background.  Both round at the same points; they differ in the order of the fp32 accumulations (MFMA tiles vs the
    GEMM library), which moves a rounded fp16 value by one ulp now and then.
    Observed on an MI355X (max over the four cases): image 1.05e-4 abs, depth 5.4e-6 abs, worst parameter gradient
    9.6e-4 relative L2 (the hash table's; the MLP weights' stay near 2.5e-4).  Bars: just under 4x those."""
    _restated(C, bound, 128, monkeypatch)


@pytest.mark.parametrize("T", [1100])
@pytest.mark.parametrize("bound", [2, 3])
@pytest.mark.parametrize("C", [1, 3])
def test_against_the_regime_restated_by_the_statement_beyond_one_pass(C, bound, T, monkeypatch):
    """The same comparison at more than one scan pass per ray (64 lanes x 8 samples = 512), same bars."""
    _restated(C, bound, T, monkeypatch)


def _restated(C, bound, T, monkeypatch):
    N = 4096
    model = _model(C, bound, 9).train()
    ro, rd = _hit_rays(N, 13 + bound, bound)
    bg = torch.rand(N, C, device=DEV)
    img_n, dep_n, g_n = _run(model, ro, rd, bg, T, True, monkeypatch)
    img_s, dep_s, g_s = _run(model, ro, rd, bg, T, False, monkeypatch)
    e_img = (img_n - img_s).abs().max().item()
    e_dep = (dep_n - dep_s).abs().max().item()
    rel = {n: ((g_n[n] - g_s[n]).norm() / g_s[n].norm().clamp_min(1e-30)).item() for n in g_s}
    print(f"\nC={C} bound={bound}: image {e_img:.3e}, depth {e_dep:.3e}, grads " +
          ", ".join(f"{n} {v:.3e}" for n, v in rel.items()))
    assert e_img <= 4e-4, e_img
    assert e_dep <= 2e-5, e_dep
    for n, v in rel.items():
        assert g_s[n].norm() > 0, n
        assert v <= 3.8e-3, (n, v)


# ------------------------------------------------------------------------------------------------------ 3. training
def _teacher(ro, rd):
    """the analytic colour where the ray meets the 0.6-sphere, white where it misses"""
    from enerf_amd import scene
    b_ = (ro * rd).sum(-1)
    disc = b_ ** 2 - ((ro * ro).sum(-1) - 0.36)
    hit = disc > 0
    t = -b_ - torch.sqrt(disc.clamp(min=0))
    p = ro + rd * t.unsqueeze(-1)
    return torch.where(hit.unsqueeze(-1), scene.analytic_color(p).clamp(0, 1), torch.ones_like(p))


def _rgb_batches(n, n_rays, seed=11):
    from enerf_amd import scene
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for b in range(n):
        (ro, rd), _ = scene.training_batch(b, n_rays, DEV, generator=g)
        out.append((ro, rd, _teacher(ro, rd)))
    return out


RGB_KW = dict(num_steps=128, upsample_steps=0, out_dim_color=3)


def _rgb_harness(fp16, seed=0, **model_kw):
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    torch.manual_seed(seed)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=False, out_dim_color=3, **model_kw).to(DEV)
    return TrainHarness(model, lr=1e-2, fp16=fp16)


def _train_rgb(h, batches, steps):
    torch.manual_seed(1)
    return np.array([float(h.step_rgb(*batches[i % len(batches)], **RGB_KW)) for i in range(steps)])


def _event_batch(n, seed):
    """n pixels of pose k seen again 1 degree further on; polarities from the analytic scene's lin-log luma change
    (real-valued, as tools/psnr_ab_events.py makes them): a batch the event loss can learn."""
    from enerf_amd import scene
    from enerf_amd.events import lin_log, rgb_to_luma
    g = torch.Generator().manual_seed(seed)
    inds = torch.randint(0, scene.H * scene.W, (n,), generator=g).to(DEV)
    k = (seed * 7) % 32
    (o1, d1) = scene.pixel_rays(scene.pose(k), inds, DEV)
    (o2, d2) = scene.pixel_rays(scene.pose(k + 1.0 / (360.0 / 32)), inds, DEV)
    ll = lambda o, d: lin_log(rgb_to_luma(_teacher(o, d), esim=True) * 255, linlog_thres=20)  # noqa: E731
    pols = ((ll(o2, d2) - ll(o1, d1)) / 0.2).reshape(1, n).contiguous()
    return {"images": torch.zeros(1, n, 1, device=DEV), "rays_evs_o1": o1, "rays_evs_d1": d1, "rays_evs_o2": o2,
            "rays_evs_d2": d2, "pols": pols}


def _train_events(fp16, steps=20, n=4096):
    from enerf_amd.events import EventOptions
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=False, out_dim_color=1).to(DEV)
    h = TrainHarness(model, lr=1e-2, fp16=fp16)
    opt = EventOptions(out_dim_color=1, use_luma=False, linlog=True, C_thres=0.2, event_only=True,
                       render_kwargs={"num_steps": 512, "upsample_steps": 0})
    batches = [_event_batch(n, 100 + i) for i in range(4)]          # (cycled: the first and last four see the same)
    torch.manual_seed(1)
    losses = np.array([float(h.step_events(batches[i % 4], opt)) for i in range(steps)])
    return h, losses


def _check_against_autocast(native, auto, h):
    assert np.isfinite(native).all() and np.isfinite(auto).all()
    assert abs(native[0] - auto[0]) <= 0.02 * abs(auto[0]), (native[0], auto[0])
    assert np.mean(native[-4:]) < np.mean(native[:4])
    assert float(h.scaler.get_scale()) >= 1024.0
    assert "mlp_precision" not in h.model.__dict__


def test_rgb_training_against_what_fp16_true_ran_before():
    from enerf_amd import stratified
    batches = _rgb_batches(4, 4096)
    h = _rgb_harness(True)
    assert h.strat_f16 and not h.fp16 and not h.amp_f16
    calls = stratified.stats["calls"]
    native = _train_rgb(h, batches, 48)
    assert stratified.stats["calls"] == calls + 48
    ha = _rgb_harness("autocast")
    assert ha.fp16 and not ha.strat_f16
    auto = _train_rgb(ha, batches, 48)
    assert stratified.stats["calls"] == calls + 48
    _check_against_autocast(native, auto, h)


def test_event_training_against_what_fp16_true_ran_before():
    from enerf_amd import stratified
    calls = stratified.stats["calls"]
    h, native = _train_events(True)
    assert h.strat_f16
    assert stratified.stats["calls"] == calls + 40
    ha, auto = _train_events("autocast")
    assert stratified.stats["calls"] == calls + 40
    _check_against_autocast(native, auto, h)


# ------------------------------------------------------------------------------------------------------ 4. scaling
def test_loss_scaling_skips_non_finite_steps_and_backs_the_scale_off():
    """Non-finite gradients reach the parameters' .grad unchanged: GradScaler's unscale_ finds them, the step is
    skipped, the scale halves; from a scale that fits on, the run trains."""
    batches = _rgb_batches(4, 4096)
    h = _rgb_harness(True)
    h.scaler._lazy_init_scale_growth_tracker(torch.device(DEV))
    h.scaler._scale.fill_(2.0 ** 40)
    before = {n: p.detach().clone() for n, p in h.model.named_parameters()}
    torch.manual_seed(1)
    loss0 = float(h.step_rgb(*batches[0], **RGB_KW))
    assert np.isfinite(loss0)
    assert float(h.scaler.get_scale()) == 2.0 ** 39
    for n, p in h.model.named_parameters():
        assert torch.equal(p.detach(), before[n]), n
    losses = [float(h.step_rgb(*batches[i % 4], **RGB_KW)) for i in range(1, 80)]
    scale = float(h.scaler.get_scale())
    assert scale < 2.0 ** 39
    assert any(not torch.equal(p.detach(), before[n]) for n, p in h.model.named_parameters())
    assert np.isfinite(losses).all() and np.mean(losses[-8:]) < 0.8 * np.mean(losses[:8])


# ------------------------------------------------------------------------------------------------------ 5. graph
def test_forward_backward_captured_in_a_cuda_graph():
    from enerf_amd import _lib, stratified
    N, T, C = 2048, 128, 3
    model = _model(C, 2, 21).train()
    ro, rd = _hit_rays(N, 22, 2)
    bg = torch.rand(N, C, device=DEV)
    params = list(model.parameters())

    def step():
        out = model.render(ro, rd, staged=False, bg_color=bg, perturb=False, num_steps=T, upsample_steps=0,
                           out_dim_color=C)
        loss = (out["image"] ** 2).sum() + out["depth"].sum()
        loss.backward()
        return loss.detach()

    with fp16_regime(model):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                for p in params:
                    p.grad = None
                eager = step()
            eager_grads = [p.grad.clone() for p in params]
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gen = _lib.lib().enerf_workspace_generation()
        calls = stratified.stats["calls"]
        for p in params:
            p.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_loss = step()
        assert stratified.stats["calls"] == calls + 1
        for p in params:
            p.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert _lib.lib().enerf_workspace_generation() == gen
    assert torch.equal(static_loss, eager)
    for p, ge in zip(params, eager_grads):
        # (the hash table's gradient is summed by atomics: its order, and so its last bit, is not fixed)
        err = (p.grad - ge).abs().max().item()
        assert err <= 1e-5 * ge.abs().max().item(), err


# ------------------------------------------------------------------------------------------------------ 6. fallbacks
def test_background_model_takes_the_autocast_route():
    from enerf_amd import stratified
    batches = _rgb_batches(2, 2048)
    h = _rgb_harness(True, bg_radius=4.0)
    assert h.strat_f16
    calls = stratified.stats["calls"]
    losses = _train_rgb(h, batches, 12)
    assert stratified.stats["calls"] == calls
    assert np.isfinite(losses).all() and np.mean(losses[-3:]) < np.mean(losses[:3])
    assert "mlp_precision" not in h.model.__dict__


def test_full_checkpoint_restores_the_scale(tmp_path):
    from enerf_amd.checkpoint import load_checkpoint
    batches = _rgb_batches(2, 2048)
    h = _rgb_harness(True)
    h.scaler._lazy_init_scale_growth_tracker(torch.device(DEV))
    h.scaler._scale.fill_(2.0 ** 20)
    _train_rgb(h, batches, 4)
    scale = float(h.scaler.get_scale())
    path = str(tmp_path / "ck.pth")
    h.save_checkpoint(path, full=True)
    h2 = _rgb_harness(True, seed=5)
    assert float(h2.scaler.get_scale()) != scale
    load_checkpoint(h2, path)
    assert float(h2.scaler.get_scale()) == scale
    loss = float(h2.step_rgb(*batches[0], **RGB_KW))
    assert np.isfinite(loss)


def test_default_precision_keeps_the_fp32_forms():
    from enerf_amd import stratified
    model = _model(3, 2, 31).train()
    ro, rd = _hit_rays(1024, 32, 2)
    with keep_last() as strat:
        model.render(ro, rd, staged=False, bg_color=None, perturb=False, num_steps=64, upsample_steps=0,
                     out_dim_color=3)
        assert strat.last["cin"].dtype == torch.float32 and strat.last["rgb"].dtype == torch.float32
