"""A background model (bg_radius > 0) on the native routes: the marching route's training node and whole-frame evaluation,
the stratified fp32 node, a dozen harness steps -- each against the route it takes with background.ENABLED = False, which
is the route every background model took before."""
import argparse as ap
import contextlib

import pytest
import torch

from test_gpu_gray_marching import _batches, _counting
from test_gpu_stratified import _close_rel, _empty_rays, _hit_rays, _mask_flips, mlp_precision
from util import assert_close, det_fill_

pytestmark = pytest.mark.gpu
DEV = "cuda"
BG_RADIUS = 3.0


@contextlib.contextmanager
def _switch(module, name, value):
    prev = getattr(module, name)
    setattr(module, name, value)
    try:
        yield
    finally:
        setattr(module, name, prev)


def _marching_model(C, seed=0, **kw):
    from enerf_amd import scene
    from enerf_amd.network import NeRFNetwork
    torch.manual_seed(seed)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=C, bg_radius=BG_RADIUS, **kw).to(DEV)
    model.encoder.embeddings.data.uniform_(-0.5, 0.5)
    model.encoder_bg.embeddings.data.uniform_(-0.5, 0.5)
    scene.install_occupancy(model)
    return model


def _decided(model, ro, rd):
    """-> (the rays whose 64 hidden pre-activations all lie clear of zero by more than fp32 round-off, how many were dropped):
    background_ref.forward's `undecided`, from the kernel's own input rows.  On the others the kernel's FMA chain and torch's
    matrix product may take different ReLU branches.  The image does not feel that (relu is continuous), but one flipped
    unit moves bg_net.0.weight's and the table's gradient by a whole ray's share -- measured: 2 such rays of 3000 with view
    directions off, 15 entries of grad_W0 off by up to 1.2 % -- which says nothing about either route.
    tests/nerf_mlp_ref.make_batch rejects its knife-edge rows for the same reason."""
    import background_ref as R
    from enerf_amd import background
    enc = model.encoder_bg
    trace = torch.full((ro.shape[0], 2 + 16 + 2 * enc.num_levels), float("nan"), device=DEV)
    W0, W1 = model.bg_net[0].weight.detach().contiguous(), model.bg_net[1].weight.detach().contiguous()
    background.forward_raw(ro, rd, model.bg_radius, background._geometry(enc), not model.disable_view_direction,
                           enc.embeddings.detach().contiguous(), enc.offsets, W0, W1, trace=trace)
    undecided = R.forward(trace[:, 2:].cpu().numpy(), W0.cpu().numpy(), W1.cpu().numpy())["undecided"]
    R.assert_decided(undecided)
    keep = torch.from_numpy(~undecided).to(DEV)
    return ro[keep].contiguous(), rd[keep].contiguous(), int(undecided.sum())


@pytest.mark.parametrize("C,mean_count,view_dirs", [(3, -1, True), (1, 40000, True), (3, 40000, False)])
def test_marching_training_render_matches_train_ops(C, mean_count, view_dirs):
    """run_cuda's training branch: _FusedRenderTrain with the native background against _train_ops with the statement,
    from identical state -- the bars of test_gpu_training.test_fused_render_node_matches_op_by_op_route.  Image, depth and
    counters on all 3000 rays; the gradients on the rays left by _decided (at most 3 dropped)."""
    from enerf_amd import background, fused_render, scene
    model = _marching_model(C, disable_view_direction=not view_dirs).train()
    g = torch.Generator(device=DEV).manual_seed(5)
    (ro_all, rd_all), _ = scene.training_batch(0, 3000, DEV, generator=g)
    ro_all, rd_all = ro_all.reshape(-1, 3).contiguous(), rd_all.reshape(-1, 3).clone()
    rd_all[::3] = -rd_all[::3]
    gi_all = torch.randn(3000, C, device=DEV, generator=g)
    fused_calls = []

    def run(native, ro, rd, gi):
        model.zero_grad()
        model.local_step = 0
        model.step_counter.zero_()
        model.mean_count = mean_count
        calls = background.stats["calls"]
        with _switch(background, "ENABLED", native), _counting(fused_render, "render_train", fused_calls):
            out = model.render(ro, rd, staged=False, bg_color=None, perturb=True)
            (out["image"].reshape(-1, C) * gi).sum().backward()
        assert background.stats["calls"] == calls + (1 if native else 0)
        return (out["image"].detach().reshape(-1, C), out["depth"].detach().reshape(-1), model.step_counter[0].clone(),
                {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})

    # (view directions off: the fused node does not serve the network itself, the native background then feeds _train_ops)
    taken = 1 if view_dirs else 0
    im1, dp1, c1, _ = run(True, ro_all, rd_all, gi_all)
    assert len(fused_calls) == taken                              # the fused node is taken ...
    im0, dp0, c0, _ = run(False, ro_all, rd_all, gi_all)
    assert len(fused_calls) == taken                              # ... and, switched off, the parent's route (_train_ops)
    assert torch.equal(c1, c0)
    # a good share of the rays miss the occupied cells (every third looks away): their pixels are background alone
    with torch.no_grad():
        bg = model.background_from_rays(ro_all, rd_all)
    missed = float(((im0 - bg).abs().amax(-1) < 1e-6).float().mean())
    assert 0.3 < missed < 0.9, missed
    assert float((im1 - im0).abs().max()) < 2e-5
    assert float((dp1 - dp0).abs().max()) < 2e-5
    # the gradients, without the rays whose ReLU branch fp32 round-off decides
    ro, rd, dropped = _decided(model, ro_all, rd_all)
    print(f"rays with an undecided ReLU branch, left out of the gradient comparison: {dropped} of 3000")
    assert dropped <= 3
    gi = gi_all[:ro.shape[0]].contiguous()
    g1, g0 = run(True, ro, rd, gi)[3], run(False, ro, rd, gi)[3]
    assert set(g1) == set(g0) and {"encoder_bg.embeddings", "bg_net.0.weight", "bg_net.1.weight"} <= set(g1)
    for n in g0:
        assert float((g1[n] - g0[n]).abs().max()) <= 2e-4 * float(g0[n].abs().max()) + 1e-9, n
    assert float(g0["encoder_bg.embeddings"].abs().max()) > 0 and float(g0["bg_net.0.weight"].abs().max()) > 0


def test_marching_evaluation_takes_the_whole_frame_pass():
    """Evaluation: render_frame with the per-ray background of the forward kernel, against render_rounds with the statement
    -- the bars of test_gpu_baseline_configs.test_frame_schedule_equals_round_schedule_fp32_nets."""
    from enerf_amd import background, frame, scene
    model = _marching_model(3, seed=2).eval()
    g = torch.Generator(device=DEV).manual_seed(4)
    (ro, rd), _ = scene.training_batch(2, 20000, DEV, generator=g)
    frames, rounds = [], []
    with torch.no_grad(), _counting(frame, "render_frame", frames), _counting(frame, "render_rounds", rounds):
        calls = background.stats["calls"]
        out1 = model.render(ro, rd, staged=False, bg_color=None, perturb=False)
        assert (len(frames), len(rounds)) == (1, 0) and background.stats["calls"] == calls + 1
        with _switch(background, "ENABLED", False):
            out0 = model.render(ro, rd, staged=False, bg_color=None, perturb=False)
        assert (len(frames), len(rounds)) == (1, 1) and background.stats["calls"] == calls + 1
    i1, i0 = out1["image"].view(-1, 3), out0["image"].view(-1, 3)
    # (the two backgrounds differ by fp32 round-off of the MLP, below 2e-6 on values in (0, 1): the bound on the images)
    assert float((i1 - i0).abs().max()) < 2e-6
    dd = (out1["depth"] - out0["depth"]).abs()
    assert float(dd[torch.isfinite(dd)].max()) < 2e-6
    assert float(i1.std()) > 0.01


def _stratified_scene(C, seed=3):
    """test_gpu_stratified._scene with a background model."""
    from enerf_amd.network import NeRFNetwork
    torch.manual_seed(seed)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=False, out_dim_color=C, bg_radius=4.0)
    det_fill_(list(model.parameters()), seed)
    with torch.no_grad():
        emb = model.encoder.embeddings
        n0 = int(model.encoder.offsets[1])
        emb.mul_(0.01)
        rows = torch.arange(n0)
        emb[:n0] = torch.where(rows >= 2048, 1.0, -1.0).unsqueeze(-1).expand(n0, 2)
        w0 = model.sigma_net[0].weight
        s = w0[:, 0] + w0[:, 1]
        model.sigma_net[1].weight[0] = torch.where(s > 0, 1.0, -1.0)
        model.bg_net[0].weight.mul_(0.2)
        model.bg_net[1].weight.mul_(0.2)
    return model


@pytest.mark.parametrize("C", [1, 3])
def test_stratified_fp32_route_against_the_statement(C):
    """The comparison of test_gpu_stratified._on_vs_off, with the model's own background on either side."""
    from enerf_amd import background, stratified
    N, T = 4096, 512
    model = _stratified_scene(C).to(DEV).train()
    o1, d1 = _hit_rays(N - 512, 11)
    o2, d2 = _empty_rays(512, 12)
    ro = torch.cat([o1, o2]).to(DEV)[None]
    rd = torch.cat([d1, d2]).to(DEV)[None]

    def arm(native):
        model.zero_grad(set_to_none=True)
        calls, bg_calls = stratified.stats["calls"], background.stats["calls"]
        stratified.KEEP_LAST = True
        try:
            with _switch(background, "ENABLED", native), mlp_precision(0):
                out = model.render(ro, rd, staged=False, bg_color=None, perturb=False, num_steps=T, upsample_steps=0,
                                   out_dim_color=C)
                ((out["image"] ** 2).sum() + out["depth"].sum()).backward()
        finally:
            stratified.KEEP_LAST = False
        assert stratified.stats["calls"] == calls + (1 if native else 0)
        assert background.stats["calls"] == bg_calls + (1 if native else 0)
        grads = {n: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for n, p in
                 model.named_parameters()}
        return out["image"].detach(), out["depth"].detach(), grads, (stratified.last if native else None)

    img1, dep1, gr1, last = arm(True)
    img0, dep0, gr0, _ = arm(False)
    flip = _mask_flips(model, ro, rd, T, last["w"])
    assert int(flip.sum().item()) <= 4
    keep = ~flip
    assert_close(img1[0][keep], img0[0][keep], rtol=0, atol=1e-5)
    assert_close(dep1[0][keep], dep0[0][keep], rtol=0, atol=1e-5)
    assert_close(img1, img0, rtol=0, atol=5e-4)
    assert_close(dep1, dep0, rtol=0, atol=1e-5)
    for n in gr0:
        _close_rel(gr1[n], gr0[n], 1e-4, n)
    for n in ("encoder_bg.embeddings", "bg_net.0.weight", "bg_net.1.weight"):
        assert float(gr0[n].abs().max()) > 0, n


def test_a_dozen_frame_steps_train_the_background():
    from enerf_amd import background
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3, bg_radius=BG_RADIUS).to(DEV)
    h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
    data = _batches(4, 2048, 3)
    batches = [{"rays_o": ro.view(1, -1, 3), "rays_d": rd.view(1, -1, 3), "images": tg.view(1, -1, 3)} for ro, rd, tg in data]
    opt = ap.Namespace(out_dim_color=3, color_space="srgb", render_kwargs={})
    before = {n: p.detach().clone() for n, p in model.named_parameters() if n.startswith(("encoder_bg", "bg_net"))}
    calls = background.stats["calls"]
    losses = [float(h.step_frames(batches[i % 4], opt)) for i in range(12)]
    assert background.stats["calls"] == calls + 12
    assert all(l == l for l in losses) and sum(losses[-3:]) < sum(losses[:3]), losses
    for n, p in model.named_parameters():
        if n in before:
            assert not torch.equal(p.detach(), before[n]), n


def test_switched_off_everything_runs_as_before():
    """background.ENABLED = False: the statement's launch chain, _train_ops, render_rounds -- and no native call."""
    from enerf_amd import background, frame, fused_render, scene
    model = _marching_model(3).train()
    g = torch.Generator(device=DEV).manual_seed(5)
    (ro, rd), _ = scene.training_batch(0, 1024, DEV, generator=g)
    fused, frames, rounds = [], [], []
    calls = background.stats["calls"]
    with _switch(background, "ENABLED", False), _counting(fused_render, "render_train", fused), \
            _counting(frame, "render_frame", frames), _counting(frame, "render_rounds", rounds):
        assert not background.supported(model, ro.view(-1, 3), rd.view(-1, 3))
        model.render(ro, rd, staged=False, perturb=True)["image"].sum().backward()
        with torch.no_grad():
            model.eval().render(ro, rd, staged=False, perturb=False)
    assert (len(fused), len(frames), len(rounds)) == (0, 0, 1) and background.stats["calls"] == calls
    assert model.encoder_bg.embeddings.grad is not None
