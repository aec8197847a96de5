"""End-to-end behaviour of the HIP path under optimisation: the loss goes down, replicas of a step are deterministic in
their integer state, and the rendered image agrees with the CPU oracle route in PSNR terms."""
import contextlib
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _batches(n, n_rays, bound, seed=11):
    from enerf_amd import scene
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for b in range(n):
        (ro, rd), _ = scene.training_batch(b, n_rays, DEV, generator=g)
        # target: analytic colour of the point where the ray meets the 0.6-sphere (smooth, learnable)
        b_ = (ro * rd).sum(-1)
        disc = b_ ** 2 - ((ro * ro).sum(-1) - 0.36)
        hit = disc > 0
        t = -b_ - torch.sqrt(disc.clamp(min=0))
        p = ro + rd * t.unsqueeze(-1)
        # rays that miss the sphere should come out as the (white) background
        tgt = torch.where(hit.unsqueeze(-1), scene.analytic_color(p).clamp(0, 1), torch.ones_like(p))
        out.append((ro, rd, tgt))
    return out


@pytest.mark.parametrize("net", ["linear", "ff"])
def test_training_reduces_loss(net):
    from enerf_amd.trainer import TrainHarness
    if net == "ff":
        from enerf_amd.network_ff import NeRFNetwork
    else:
        from enerf_amd.network import NeRFNetwork
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
    h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
    data = _batches(8, 2048, 2)
    losses = []
    for i in range(160):
        ro, rd, tgt = data[i % len(data)]
        losses.append(float(h.step_rgb(ro, rd, tgt).detach()))
    first, last = np.mean(losses[:8]), np.mean(losses[-8:])
    assert np.isfinite(losses).all()
    assert last < 0.5 * first, (first, last)
    assert model.mean_count > 0 and model.iter_density == math.ceil(160 / 16)


@pytest.mark.parametrize("bg", ["none", "scalar", "tensor"])
@pytest.mark.parametrize("mean_count", [-1, 40000])
def test_fused_render_node_matches_op_by_op_route(monkeypatch, bg, mean_count):
    """enerf_amd.fused_render (one autograd node for near_far -> march -> network -> composite -> background blend)
    against run_cuda's op-by-op training branch: same sample counters, image, depth and parameter gradients; with
    the sample budget unknown (mean_count <= 0, first 16 steps) and fixed (later steps, with overflow drop rule)."""
    from enerf_amd import fused_network, fused_render, scene
    from enerf_amd.network import NeRFNetwork
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
    model.encoder.embeddings.data.uniform_(-0.5, 0.5)
    scene.install_occupancy(model)
    model.train()
    g = torch.Generator(device=DEV).manual_seed(5)
    (ro, rd), _ = scene.training_batch(0, 3000, DEV, generator=g)
    gi = torch.randn(3000, 3, device=DEV)
    bg_color = {"none": None, "scalar": 0.25, "tensor": torch.rand(1, 1, 3, device=DEV)}[bg]
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
        out = model.render(ro.view(1, -1, 3) if bg == "tensor" else ro, rd.view(1, -1, 3) if bg == "tensor" else rd,
                           staged=False, bg_color=bg_color, perturb=True)
        (out["image"].reshape(-1, 3) * gi).sum().backward()
        return (out["image"].detach().reshape(-1, 3), out["depth"].detach().reshape(-1), model.step_counter[0].clone(),
                {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})

    im1, dp1, c1, g1 = run(True)
    assert len(calls) == 1
    im0, dp0, c0, g0 = run(False)
    assert len(calls) == 1
    assert torch.equal(c1, c0)                                   # samples / rays counted: bit-exact
    assert float((im1 - im0).abs().max()) < 2e-5
    assert float((dp1 - dp0).abs().max()) < 2e-5
    assert set(g1) == set(g0)
    for n in g0:
        assert float((g1[n] - g0[n]).abs().max()) <= 2e-4 * float(g0[n].abs().max()) + 1e-9, n


def test_manual_mse_step_matches_autograd_step(monkeypatch):
    """TrainHarness.manual_mse: the RGB step runs fused_render.train_step_mse (closed-form MSE gradient inside the
    composite backward, no autograd).  Same loss trajectory, counters and final weights as the autograd-driven step."""
    from enerf_amd import fused_render
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 2048, 2)
    calls = []
    orig, orig_native = fused_render.train_step_mse, fused_render.train_step_native
    monkeypatch.setattr(fused_render, "train_step_mse", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    # (once the sample budget exists the same launches are issued by the library itself: enerf_train_step_mse)
    monkeypatch.setattr(fused_render, "train_step_native", lambda *a, **k: (calls.append(1), orig_native(*a, **k))[1])
    runs = []
    for manual in (False, True):
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        h.manual_mse = manual
        losses = [h.step_rgb(*data[i % len(data)]).clone() for i in range(40)]
        runs.append((torch.stack(losses).cpu(), model.step_counter.clone().cpu(),
                     {n: p.detach().clone() for n, p in model.named_parameters()}))
        assert len(calls) == (40 if manual else 0)            # from the first step on: no sample budget needed
    (l0, c0, p0), (l1, c1, p1) = runs
    assert torch.equal(c0, c1)
    # Adam with eps = 1e-15 turns rounding-level gradient differences on rarely-hit table rows into lr-sized steps:
    # compare the weights in the mean, the trajectory through the losses
    for n in p0:
        assert float((p0[n] - p1[n]).abs().mean()) <= 1e-3 * float(p0[n].abs().mean()), n
    rel = ((l0 - l1).abs() / l0.abs().clamp(min=1e-9))
    # the first steps agree to rounding; after that the two runs drift apart at the rate the atomics' summation order
    # allows (the same route run twice does too: 0.6e-4 ... 1.04e-4 at step 40 from run to run)
    assert float(rel[:10].max()) < 5e-6, rel.tolist()
    assert float(rel.max()) < 3e-4, rel.tolist()


def test_graph_replay_matches_eager_steps():
    """TrainHarness(use_graphs=True): render + loss + backward replayed as a HIP graph once the sample budget is known.
    Same budgets, same inputs -> the loss trajectory and the sample counters are those of the eager harness."""
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 2048, 2)
    runs = []
    for graphs in (False, True):
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
        model.sample_budget_quantum = 8192                    # the graph harness rounds the budget up; match it
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic", use_graphs=graphs)
        losses = [h.step_rgb(*data[i % len(data)]).clone() for i in range(40)]
        runs.append((torch.stack(losses).cpu(), model.step_counter.clone().cpu(), len(h._graphs)))
    (l0, c0, n0), (l1, c1, n1) = runs
    assert n0 == 0 and n1 >= 1
    assert torch.equal(c0, c1)
    assert float(((l0 - l1).abs() / l0.abs().clamp(min=1e-9)).max()) < 1e-4


@pytest.mark.parametrize("manual", [True, False])
def test_prefetched_march_gives_the_same_steps(monkeypatch, manual):
    """The parameter-independent stage of the NEXT render (near_far + march) is issued early: on a side stream once the
    forward is queued (closed-form MSE step), or right after the gradient collectives are launched (autograd step, with
    a stand-in averager here).  Either way the prefetching harness must reproduce the plain one: same sample counters,
    same loss trajectory, across update_extra_state boundaries."""
    from enerf_amd import fused_render
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    streams = []
    orig = fused_render.prefetch_march
    monkeypatch.setattr(fused_render, "prefetch_march",
                        lambda *a, **k: (streams.append(k.get("stream")), orig(*a, **k))[1])

    class NoComm:
        def start(self): pass
        def finish(self): pass

    data = _batches(4, 2048, 2)
    runs = []
    for prefetch in (False, True):
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        h.avg = NoComm()
        h.prefetch = prefetch
        h.manual_mse = manual
        losses, slots = [], []
        for i in range(52):
            nxt = data[(i + 1) % len(data)]
            losses.append(h.step_rgb(*data[i % len(data)], next_rays=(nxt[0], nxt[1])).clone())
            slots.append(int(model.step_counter[model.rendered_counter_slot, 0]))
        runs.append((torch.stack(losses).cpu(), slots, model.mean_count))
    (l0, s0, m0), (l1, s1, m1) = runs
    assert len(streams) >= 30 and all((st is not None) == manual for st in streams)
    assert s0 == s1 and m0 == m1
    # (the grid backward's float atomics land in a different order from run to run; 52 Adam steps amplify that)
    assert float(((l0 - l1).abs() / l0.abs().clamp(min=1e-9)).max()) < 5e-4


def test_step_is_deterministic_in_integer_state():
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    res = []
    for _ in range(2):
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
        h = TrainHarness(model, occupancy="synthetic")
        data = _batches(2, 1024, 2)
        h.step_rgb(*data[0])
        res.append((model.step_counter.clone(), model.density_bitfield.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_render_psnr_vs_cpu_oracle_route(monkeypatch):
    """64x48 frame: HIP inference loop vs the same model through the CPU oracle backend: PSNR >= 70 dB."""
    import enerf_amd.raymarching as rmod, enerf_amd.gridencoder as gmod, enerf_amd.shencoder as smod
    from oracle import backend as ob
    from enerf_amd.network import NeRFNetwork
    from enerf_amd import scene
    torch.manual_seed(0)
    gpu = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV).eval()
    gpu.encoder.embeddings.data.uniform_(-0.5, 0.5)
    scene.install_occupancy(gpu)
    state = {k: v.detach().cpu().clone() for k, v in gpu.state_dict().items()}
    ys, xs = torch.meshgrid(torch.arange(0, 480, 10), torch.arange(0, 640, 10), indexing="ij")
    inds = (ys * 640 + xs).reshape(-1)
    ro, rd = scene.pixel_rays(scene.pose(5), inds.to(DEV), DEV)
    with torch.no_grad():
        img_gpu = gpu.render(ro, rd, staged=False, bg_color=None, perturb=False)["image"].cpu()
    with monkeypatch.context() as mp:
        mp.setattr(rmod, "_backend", ob.raymarching_backend); mp.setattr(rmod, "_DEVICE", "cpu")
        mp.setattr(gmod, "_backend", ob.gridencoder_backend); mp.setattr(smod, "_backend", ob.shencoder_backend)
        cpu = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).eval()
        cpu.load_state_dict(state)
        with torch.no_grad():
            img_cpu = cpu.render(ro.cpu(), rd.cpu(), staged=False, bg_color=None, perturb=False)["image"]
    mse = float(((img_gpu - img_cpu) ** 2).mean())
    psnr = 10 * math.log10(1.0 / max(mse, 1e-20))
    print(f"PSNR(HIP, CPU oracle) = {psnr:.1f} dB over {inds.numel()} pixels")
    assert psnr >= 70.0


def _dp_worker(rank, world, port, chunks, out, comm_dtype=None):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from enerf_amd.network import NeRFNetwork
        from enerf_amd.trainer import TrainHarness
        torch.cuda.set_device(0)
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic", world=world)
        h.comm_chunks = chunks
        h.comm_dtype = comm_dtype
        data = _batches(4, 1024, 2, seed=10 + rank)          # every rank renders its own rays
        losses = []
        for i in range(36):
            nxt = data[(i + 1) % len(data)]
            losses.append(float(h.step_rgb(*data[i % len(data)], next_rays=(nxt[0], nxt[1]))))
        torch.cuda.synchronize()
        out[(chunks if comm_dtype is None else "bf16", rank)] = (losses, {n: p.detach().cpu()
                                                                            for n, p in model.named_parameters()})
    finally:
        dist.destroy_process_group()


def test_data_parallel_chunked_allreduce_adam_pipeline_matches_bucket_path():
    """Two ranks (gloo, both on this GPU): the closed-form step's data-parallel tail -- hash-table gradient all-reduced in
    pieces with Adam applied piece by piece, MLP gradients as one flat buffer -- gives the replicas the same weights as
    the two-bucket GradAverager + one optimizer step, and keeps the replicas identical."""
    import socket
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    for chunks in (0, 4):
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        mp.spawn(_dp_worker, args=(2, port, chunks, out), nprocs=2, join=True)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_dp_worker, args=(2, port, 4, out, torch.bfloat16), nprocs=2, join=True)
    # opt-in 16-bit wire format for the table gradient: replicas still identical, same training within bf16 rounding
    p0, p1 = out[("bf16", 0)][1], out[("bf16", 1)][1]
    assert all(torch.equal(p0[n], p1[n]) for n in p0)
    lc = np.array(out[("bf16", 0)][0])
    assert np.abs(lc - np.array(out[(4, 0)][0])).max() <= 0.05 * np.abs(lc).max()
    for chunks in (0, 4):
        p0, p1 = out[(chunks, 0)][1], out[(chunks, 1)][1]
        for n in p0:
            assert torch.equal(p0[n], p1[n]), (chunks, n)                       # replicas stay identical
    la, lb = np.array(out[(0, 0)][0]), np.array(out[(4, 0)][0])
    assert np.abs(la - lb).max() <= 1e-4 * np.abs(la).max()
    for n, a in out[(0, 0)][1].items():
        b = out[(4, 0)][1][n]
        assert float((a - b).abs().mean()) <= 1e-3 * float(a.abs().mean()), n


def test_one_reduce_launch_for_both_networks_is_bit_identical(monkeypatch):
    """nerf_backward defers the colour net's weight-gradient reduction to the sigma net's reduce launch
    (enerf_mlp32_defer_reduce): same sums in the same order as two launches, so every gradient is bit-identical."""
    from enerf_amd import _lib, fused_network as fn
    from enerf_amd.network import NeRFNetwork
    torch.manual_seed(3)
    net = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
    B = 40000
    x = (torch.rand(B, 3, device=DEV) * 2 - 1) * 1.9
    d = torch.nn.functional.normalize(torch.randn(B, 3, device=DEV), dim=-1)
    params = fn.network_params(net)
    g_sigma = torch.randn(B, device=DEV)
    g_rgb = torch.randn(B, 3, device=DEV)

    def grads(defer):
        if not defer:
            monkeypatch.setattr(_lib.lib(), "enerf_mlp32_defer_reduce", lambda on: 0)
        with torch.no_grad():
            _, _, sv = fn.nerf_forward(x, d, fn.network_cfg(net), True, params[0], net.encoder.offsets, *params[1:])
            g_emb, dw = fn.nerf_backward(sv, g_sigma.clone(), g_rgb.clone(), raw=True)
        torch.cuda.synchronize()
        monkeypatch.undo()
        return g_emb, dw
    (ea, wa), (eb, wb) = grads(True), grads(False)
    assert torch.equal(wa, wb) and bool(wa.abs().sum() > 0)
    assert float((ea - eb).abs().max()) <= 1e-6 * float(ea.abs().max())      # (coarse levels: float atomics)


def _rccl_worker(rank, world, port, out):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=rank, world_size=world)
    try:
        from enerf_amd.network import NeRFNetwork
        from enerf_amd.trainer import TrainHarness
        data = _batches(4, 1024, 2, seed=10)
        for tag, dp, dtype in (("single", 1, None), ("rccl", 2, None), ("rccl16", 2, torch.bfloat16),
                               ("rccl_sharded", 2, None)):
            torch.manual_seed(0)
            model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
            h = TrainHarness(model, lr=1e-2, occupancy="synthetic", world=dp)     # dp = 2: the data-parallel tail runs
            h.comm_dtype = dtype
            if tag == "rccl_sharded":      # reduce_scatter_tensor -> Adam on the slice -> in-place all_gather_into_tensor
                h.comm_mode = "sharded"
            losses = []
            for i in range(36):
                nxt = data[(i + 1) % len(data)]
                losses.append(float(h.step_rgb(*data[i % len(data)], next_rays=(nxt[0], nxt[1]))))
            torch.cuda.synchronize()
            out[tag] = (losses, {n: p.detach().cpu() for n, p in model.named_parameters()})
    finally:
        dist.destroy_process_group()


def test_data_parallel_tail_over_rccl_single_rank():
    """The data-parallel tail on the real backend (RCCL, `ReduceOp.AVG`, async collectives on RCCL's stream, chunked
    Adam) with a world of one rank -- all this box offers: averaging over one rank is the identity, so the run must
    reproduce the single-process step (to the run-to-run noise of the coarse levels' float atomics); the 16-bit wire
    format must stay close to it."""
    import socket
    import torch.multiprocessing as mp
    out = mp.Manager().dict()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_rccl_worker, args=(1, port, out), nprocs=1, join=True)
    (la, pa), (lb, pb), (lc, pc) = out["single"], out["rccl"], out["rccl16"]
    la, lb = np.array(la), np.array(lb)
    print("max rel loss difference single vs RCCL tail:", np.abs(la - lb).max() / np.abs(la).max())
    assert np.abs(la - lb).max() <= 1e-4 * np.abs(la).max()       # (float atomics on the coarsest levels: not bitwise)
    for n, a in pa.items():
        assert float((a - pb[n]).abs().mean()) <= 1e-3 * float(a.abs().mean()), n
    assert np.abs(np.array(lc) - np.array(la)).max() <= 0.05 * np.abs(np.array(la)).max()
    ld, pd = out["rccl_sharded"]
    assert np.abs(la - np.array(ld)).max() <= 1e-4 * np.abs(la).max()
    for n, a in pa.items():
        assert float((a - pd[n]).abs().mean()) <= 1e-3 * float(a.abs().mean()), n


def _tune_worker(rank, world, port, out):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from enerf_amd.network import NeRFNetwork
        from enerf_amd.trainer import TrainHarness
        torch.cuda.set_device(0)
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic", world=world)
        data = _batches(4, 1024, 2, seed=10 + rank)

        def step(i):
            nxt = data[(i + 1) % len(data)]
            return h.step_rgb(*data[i % len(data)], next_rays=(nxt[0], nxt[1]))
        timings = h.tune_comm(step, candidates=(1, 3, 8), window=4)
        probe = h.probe_comm_dtype(step, torch.bfloat16, window=3)
        assert probe > 0 and h.comm_dtype is None
        loss = float(step(100))
        torch.cuda.synchronize()
        out[rank] = (timings, h.comm_chunks, h.global_step, loss,
                     {n: p.detach().cpu() for n, p in model.named_parameters()})
    finally:
        dist.destroy_process_group()


def test_comm_tuning_agrees_across_ranks():
    """tune_comm: every candidate is timed over the same number of steps, all ranks see the same timings (MAX
    all-reduce) and therefore choose the same cut; the replicas stay identical through the changes of cut (3 pieces:
    a cut that does not divide the table)."""
    import socket
    import torch.multiprocessing as mp
    out = mp.Manager().dict()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_tune_worker, args=(2, port, out), nprocs=2, join=True)
    (t0, c0, g0, l0, p0), (t1, c1, g1, l1, p1) = out[0], out[1]
    assert set(t0) == {1, 3, 8} and t0 == t1 and all(v > 0 for v in t0.values())
    assert c0 == c1 == min(t0, key=t0.get)
    # warm-up + 3 cuts, 2 windows of the sharded tail, 3 march placements (windows of 4), then 3 + 1 steps
    assert g0 == g1 == 4 * 4 + 2 * 4 + 3 * 4 + 3 + 1 and math.isfinite(l0)
    assert all(torch.equal(p0[n], p1[n]) for n in p0)


def test_comm_tuning_is_a_noop_on_one_rank():
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
    h = TrainHarness(model, occupancy="synthetic")
    assert h.tune_comm(lambda i: None) == {} and h.comm_chunks == 4 and h.global_step == 0


def test_event_step_with_closed_render_backward_matches_autograd_step(monkeypatch):
    """step_events: the two renders run without autograd, the event loss alone goes through it and hands its gradient
    to the renders' closed backward.  Same loss trajectory, counters and (in the mean) weights as the autograd step."""
    from enerf_amd import events
    from enerf_amd.events import EventOptions
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 2048, 2)
    opt = EventOptions(C_thres=0.2, use_luma=True, linlog=True, event_only=True)
    calls = []
    orig = events.train_step_events_manual
    monkeypatch.setattr(events, "train_step_events_manual", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    # (steady-state steps of the closed-form route go through the one-call step, enerf_train_step_events)
    from enerf_amd import fused_render
    orig_native = fused_render.train_step_events_native
    monkeypatch.setattr(fused_render, "train_step_events_native",
                        lambda *a, **k: (calls.append(1), orig_native(*a, **k))[1])
    runs = []
    for manual in (False, True):
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        h.manual_mse = manual
        losses = []
        torch.manual_seed(3)                                   # the step draws a random background colour
        def batch(i):
            ro, rd, tg = data[i % len(data)]
            ro2, rd2, _ = data[(i + 1) % len(data)]
            return {"images": tg.view(1, -1, 3), "rays_evs_o1": ro.view(1, -1, 3), "rays_evs_d1": rd.view(1, -1, 3),
                    "rays_evs_o2": ro2.view(1, -1, 3), "rays_evs_d2": rd2.view(1, -1, 3),
                    "pols": torch.sign(tg[..., 0] - 0.5).view(1, -1)}

        for i in range(40):      # the closed-form run also marches the next step's two ray sets early (side stream)
            losses.append(h.step_events(batch(i), opt, next_data=batch(i + 1) if manual else None).clone())
        runs.append((torch.stack(losses).cpu(), model.step_counter.clone().cpu(),
                     {n: p.detach().clone() for n, p in model.named_parameters()}))
        assert len(calls) == (40 if manual else 0)
    (l0, c0, p0), (l1, c1, p1) = runs
    assert torch.equal(c0, c1)
    assert float(((l0 - l1).abs() / l0.abs().clamp(min=1e-9)).max()) < 2e-4
    # (40 Adam steps with eps = 1e-15 amplify the routes' rounding differences: the table ends 0.9e-3 .. 1.3e-3 apart in
    # the mean, depending on the build's summation order inside the compositing scans; the loss curves agree to 5e-6)
    for n in p0:
        assert float((p0[n] - p1[n]).abs().mean()) <= 2e-3 * float(p0[n].abs().mean()), n


def test_event_step_with_negative_event_sampling_closed_form_matches_autograd(monkeypatch):
    """--negative_event_sampling: the step makes FOUR training renders (event pair + no-event pair, nerf/utils.py:482-565).
    The closed-form route (all four without autograd, record lists of all four flushed once into the tile Adam) against
    the autograd route: same counters, first losses to rounding, trajectory and weights as the two-render test; and the
    no-event term is really in the loss (a run with the term gated off differs)."""
    from enerf_amd import events
    from enerf_amd.events import EventOptions
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 2048, 2)
    calls = []
    orig = events.train_step_events_manual
    monkeypatch.setattr(events, "train_step_events_manual", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])

    def batch(i):
        ro, rd, tg = data[i % len(data)]
        ro2, rd2, _ = data[(i + 1) % len(data)]
        ro3, rd3, _ = data[(i + 2) % len(data)]
        ro4, rd4, _ = data[(i + 3) % len(data)]
        v = lambda x, n: x.view(1, -1, 3)[:, :n].contiguous()
        return {"images": tg.view(1, -1, 3), "rays_evs_o1": v(ro, 2048), "rays_evs_d1": v(rd, 2048),
                "rays_evs_o2": v(ro2, 2048), "rays_evs_d2": v(rd2, 2048), "pols": torch.sign(tg[..., 0] - 0.5).view(1, -1),
                "rays_no_evs_o1": v(ro3, 1024), "rays_no_evs_d1": v(rd3, 1024), "rays_no_evs_o2": v(ro4, 1024),
                "rays_no_evs_d2": v(rd4, 1024)}

    def run(manual, opt, steps=24):
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        h.manual_mse = manual
        torch.manual_seed(3)
        losses = [h.step_events(batch(i), opt).clone() for i in range(steps)]
        return (torch.stack(losses).cpu(), model.step_counter.clone().cpu(),
                {n: p.detach().clone() for n, p in model.named_parameters()})

    on = dict(C_thres=0.05, use_luma=True, linlog=True, event_only=True, negative_event_sampling=True, w_no_ev=5.0,
              epoch=2, epoch_start_noEvLoss=0)
    l0, c0, p0 = run(False, EventOptions(**on))
    assert not calls
    l1, c1, p1 = run(True, EventOptions(**on))
    assert len(calls) == 24
    assert torch.equal(c0, c1)                                   # four renders per step on both routes, same samples
    rel = (l0 - l1).abs() / l0.abs().clamp(min=1e-9)
    assert float(rel[:4].max()) < 1e-5 and float(rel.max()) < 3e-4, rel.tolist()
    for n in p0:
        assert float((p0[n] - p1[n]).abs().mean()) <= 2e-3 * float(p0[n].abs().mean()), n
    l2, c2, _ = run(True, EventOptions(**dict(on, epoch=0)))     # gated off: two renders per step, a different loss
    assert float((l2[0] - l1[0]).abs()) > 1e-4 * float(l1[0].abs())


def test_early_sample_budget_equals_the_update_kernels_own(monkeypatch):
    """TrainHarness.early_budget: update_extra_state's sample budget is read behind the window's last march (side stream)
    before the update is queued, and the update's own read-back is never waited for.  The value must be the one the
    update kernel forms from the same ring (checked here against the read-back, update by update), the route must really
    be taken in the steady state, and mean_density resolves to the grid's mean when somebody asks."""
    from enerf_amd import density_update, fused_render
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 2048, 2)
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
    h = TrainHarness(model, lr=1e-2, occupancy="learned")
    assert h.early_budget
    seen = []
    orig_end, orig_early = density_update.update_end, fused_render.early_mean_count

    def end(model_, handle, early=None):
        orig_end(model_, handle, early)
        done, host, _stats, total_step = handle[:4]
        done.synchronize()
        mean, counted = host.tolist()
        seen.append((early, total_step, int(counted / total_step) if total_step else None, int(model_.mean_count), mean))

    monkeypatch.setattr(density_update, "update_end", end)
    for i in range(70):
        ro, rd, tg = data[i % len(data)]
        nxt = data[(i + 1) % len(data)]
        h.step_rgb(ro, rd, tg, next_rays=(nxt[0], nxt[1]))
    torch.cuda.synchronize()
    assert len(seen) == 5                                        # updates at steps 0, 16, 32, 48, 64
    assert seen[0][0] == (None, 0)                               # nothing marched yet: no wait, no budget
    early_used = 0
    for early, total_step, device_count, host_count, mean in seen[1:]:
        assert total_step == 16 and host_count == device_count  # whichever route: the budget is the update kernel's
        if early is not None:
            assert early == (device_count, 16)
            early_used += 1
    assert early_used >= 3                                       # every update whose last march ran on the side stream
    want = float(torch.mean(model.density_grid.clamp(min=0)))
    assert abs(model.mean_density - want) <= 1e-6 * max(1.0, abs(want)) and model._pending_density_stats is None
    # switched off: the old route, same budgets
    torch.manual_seed(0)
    model2 = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
    h2 = TrainHarness(model2, lr=1e-2, occupancy="learned")
    h2.early_budget = False
    seen2, seen[:] = seen[:], []
    for i in range(20):
        ro, rd, tg = data[i % len(data)]
        nxt = data[(i + 1) % len(data)]
        h2.step_rgb(ro, rd, tg, next_rays=(nxt[0], nxt[1]))
    assert [s[0] for s in seen] == [None, None] and seen[1][3] == seen2[1][3]   # step 16: the cold window's counts agree


def test_cold_window_one_call_step_equals_the_python_driven_cold_step(monkeypatch):
    """Before the first sample budget (the reference's first 16 steps: nothing may be dropped) the one-call step reserves
    rows from an earlier render's count (fused_render.cold_capacity) and checks the count that comes back.  Against the
    Python-driven cold step: the same samples per step (counters bit-exact), the same losses to rounding; and with the
    reservation forced too small every stage is repaired (write pass repeated at the exact size) to the same result."""
    from enerf_amd import fused_render
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 2048, 2)
    native_calls = []
    orig = fused_render.train_step_native
    monkeypatch.setattr(fused_render, "train_step_native", lambda *a, **k: (native_calls.append(1), orig(*a, **k))[1])

    def run(cold_native, capacity=None, steps=15):
        monkeypatch.setattr(fused_render, "COLD_NATIVE", cold_native)
        if capacity is not None:
            monkeypatch.setattr(fused_render, "cold_capacity", capacity)
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        del native_calls[:]
        losses = []
        for i in range(steps):
            ro, rd, tg = data[i % len(data)]
            nxt = data[(i + 1) % len(data)]
            losses.append(h.step_rgb(ro, rd, tg, next_rays=(nxt[0], nxt[1])).clone())
        assert model.mean_count == 0                                   # still the cold window
        return (torch.stack(losses).cpu(), model.step_counter.clone().cpu(), len(native_calls),
                {n: p.detach().clone() for n, p in model.named_parameters()})

    l0, c0, n0, p0 = run(False)
    assert n0 == 0
    l1, c1, n1, p1 = run(True)
    assert n1 == 14                                                    # every step but the first
    assert torch.equal(c0, c1)                                         # same samples, same ring slots
    rel = (l0 - l1).abs() / l0.abs().clamp(min=1e-9)
    assert float(rel[:3].max()) < 5e-6 and float(rel.max()) < 3e-4, rel.tolist()
    for n in p0:
        assert float((p0[n] - p1[n]).abs().mean()) <= 2e-3 * float(p0[n].abs().mean()), n
    # reservation always too small: every stage overflows and is repaired
    l2, c2, n2, p2 = run(True, capacity=lambda rows, N, max_steps, floor=0: max(128, (rows // 2) // 128 * 128))
    assert n2 == 14 and torch.equal(c0, c2)
    rel = (l0 - l2).abs() / l0.abs().clamp(min=1e-9)
    assert float(rel[:3].max()) < 5e-6 and float(rel.max()) < 3e-4, rel.tolist()


def test_long_run_with_learned_occupancy_converges():
    """600 steps with the occupancy grid maintained by update_extra_state itself (not the analytic one): through the 16
    full sweeps and into the partial-update regime, with the closed-form step, the side-stream march and the device-side
    density update all active.  The loss must keep falling, the grid must neither die nor fill up, and a held-out view
    must come out close to the analytic render of the scene."""
    from enerf_amd import scene
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
    h = TrainHarness(model, lr=1e-2, occupancy="learned", update_interval=16)
    h.update_interval = 2                     # 16 full sweeps + 284 partial updates in 600 steps
    data = _batches(16, 4096, 2, seed=5)
    losses = []
    for i in range(600):
        nxt = data[(i + 1) % len(data)]
        losses.append(h.step_rgb(*data[i % len(data)], next_rays=(nxt[0], nxt[1])).clone())
    losses = torch.stack(losses).cpu().numpy()
    assert np.isfinite(losses).all()
    assert losses[-50:].mean() < 0.25 * losses[:10].mean(), (losses[:10].mean(), losses[-50:].mean())
    # no drift once the partial updates take over (per-step losses are spiky: compare medians, with slack)
    assert np.median(losses[-100:]) < 2.0 * np.median(losses[200:300])
    assert model.iter_density == 300 and model.mean_count > 0
    occ = float((model.density_grid > min(model.mean_density, model.density_thresh)).float().mean())
    assert 0.0005 < occ < 0.6, occ                                             # neither dead nor everything occupied
    ro, rd, tgt = _batches(1, 8192, 2, seed=77)[0]
    model.eval()
    with torch.no_grad():
        img = model.render(ro, rd, staged=False, bg_color=None, perturb=False)["image"].reshape(-1, 3)
    mse = float(((img - tgt) ** 2).mean())
    assert -10 * math.log10(mse) > 18.0, mse                                   # PSNR of a held-out batch of pixels


def test_fused_table_adam_step_matches_dense_gradient_step():
    """TrainHarness.fuse_table_adam (one GPU: the table gradient never becomes a dense tensor -- the optimizer's pass
    sums each tile's records in LDS) against the same closed-form step with the dense gradient + fused Adam kernel:
    same loss trajectory and counters over 40 steps, across update_extra_state boundaries and the cold window."""
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 4096, 2)
    runs = []
    for fuse in (False, True):
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        h.fuse_table_adam = fuse
        losses = []
        for i in range(40):
            nxt = data[(i + 1) % len(data)]
            losses.append(h.step_rgb(*data[i % len(data)], next_rays=(nxt[0], nxt[1])).clone())
        runs.append((torch.stack(losses).cpu(), model.step_counter.clone().cpu(),
                     {n: p.detach().clone() for n, p in model.named_parameters()}))
    (l0, c0, p0), (l1, c1, p1) = runs
    assert torch.equal(c0, c1)
    assert float(((l0 - l1).abs() / l0.abs().clamp(min=1e-9)).max()) < 5e-4
    for n in p0:
        assert float((p0[n] - p1[n]).abs().mean()) <= 1e-3 * float(p0[n].abs().mean()), n
    assert float(l1[-4:].mean()) < 0.7 * float(l1[:4].mean())


@pytest.mark.parametrize("route", ["bf16", "autocast", "f16"])
def test_fp16_training_variant(route):
    """Mixed precision, the harness's two switches:
    "autocast" = TrainHarness(fp16=True), the shipped configs' `fp16 = True` as the reference runs it
    (nerf/utils.py:964-975: autocast(float16) + GradScaler): half hash table and half table gradient through the grid
    kernels (gridencoder/grid.py:38-39,72: the 588 B/point case), half SH, fp32 marching / compositing; the scaler must
    not see overflows after its first steps;
    "bf16" = TrainHarness(amp="bf16"), this library's own regime -- the closed-form step with the networks on bf16
    operands (mlp32 precision 2), fp32 table, no loss scaling; the model's arithmetic is restored after each step;
    "f16" = TrainHarness(fp16=True) on a model the fused path serves: the SAME regime as "autocast" on the closed-form
    step -- fp16 operands (mlp32 precision 3), the GradScaler's protocol on the device, on the scaler's own tensors.
    Either way the loss must fall, the sample counters must be those of the fp32 run (marching does not depend on the
    networks), and the first step's loss must agree with the fp32 step's to 16-bit precision."""
    import functools
    from enerf_amd import fused_render
    from enerf_amd.backends import _gridencoder as ge
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 4096, 2)
    runs = []
    for fp16 in (False, {"bf16": "bf16", "autocast": "autocast", "f16": True}[route]):
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic", fp16=fp16 if fp16 in (True, "autocast") else False,
                         amp="bf16" if fp16 == "bf16" else None)
        seen, closed = [], []
        orig, orig_step = ge.grid_encode_forward, fused_render.train_step_mse
        # (functools.wraps: gridencoder._supports_layout reads the backend function's signature)
        ge.grid_encode_forward = functools.wraps(orig)(lambda *a, **k: (seen.append(a[1].dtype), orig(*a, **k))[1])
        orig_native = fused_render.train_step_native          # (steady-state steps: the same launches from one C call)
        fused_render.train_step_mse = lambda *a, **k: (closed.append(1), orig_step(*a, **k))[1]
        fused_render.train_step_native = lambda *a, **k: (closed.append(1), orig_native(*a, **k))[1]
        try:
            losses = [float(h.step_rgb(*data[i % len(data)])) for i in range(48)]
        finally:
            ge.grid_encode_forward, fused_render.train_step_mse = orig, orig_step
            fused_render.train_step_native = orig_native
        runs.append((losses, model.step_counter.clone().cpu(), set(seen), h, len(closed)))
    (l32, c32, d32, _, n32), (l16, c16, d16, h16, n16) = runs
    assert d32 == {torch.float32} and n32 == 48
    if route == "autocast":
        assert torch.float16 in d16 and n16 == 0                     # training renders used the half table (the density
        assert float(h16.scaler.get_scale()) >= 1024.0               # sweep of update_extra_state stays fp32); no run of
    elif route == "f16":                                             # overflow-halvings
        assert h16.amp_f16 and not h16.fp16 and d16 == {torch.float32} and n16 == 48        # every step closed-form
        assert h16.scaler.is_enabled() and float(h16.scaler.get_scale()) >= 1024.0
        assert h16.scaler.state_dict()["scale"] == float(h16.scaler.get_scale())
        assert h16.amp_skipped_steps() <= 6 and "mlp_precision" not in h16.model.__dict__
    else:
        assert d16 == {torch.float32} and n16 == 48 and h16.amp_bf16
        assert "mlp_precision" not in h16.model.__dict__             # (scoped to the harness's steps, not left on the model)
        assert not h16.scaler.is_enabled() and h16.scaler.state_dict() == {}
    assert torch.equal(c32, c16)
    assert np.isfinite(l16).all() and abs(l16[0] - l32[0]) <= 0.02 * abs(l32[0])
    assert np.mean(l16[-8:]) < 0.6 * np.mean(l16[:8])


def test_fp16_closed_form_skips_non_finite_steps_and_backs_the_scale_off():
    """The GradScaler protocol on the device (enerf_amp_begin / enerf_amp_end): with a loss scale far too large the
    activation gradients leave fp16's range, the weight-gradient reduce launch flags it, the optimizer launch leaves every
    parameter and moment as it was, the scale is halved and the step is counted as skipped -- step after step until the
    scale fits, from where on the run trains; the optimizer state written to a checkpoint counts applied steps only."""
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    from enerf_amd.checkpoint import checkpoint_dict
    data = _batches(4, 4096, 2)
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
    h = TrainHarness(model, lr=1e-2, occupancy="synthetic", fp16=True)
    assert h.amp_f16
    h.scaler._scale.fill_(2.0 ** 40)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    loss0 = float(h.step_rgb(*data[0]))
    torch.cuda.synchronize()
    assert np.isfinite(loss0)                                        # (the reported loss is not scaled)
    assert h.amp_skipped_steps() == 1 and float(h.scaler.get_scale()) == 2.0 ** 39
    for n, p in model.named_parameters():
        assert torch.equal(p.detach(), before[n]), n                  # nothing moved
    st = h.opt.state[model.encoder.embeddings]
    assert float(st["exp_avg"].abs().max()) == 0.0 and float(st["exp_avg_sq"].abs().max()) == 0.0
    losses = [float(h.step_rgb(*data[i % 4])) for i in range(1, 80)]
    skipped = h.amp_skipped_steps()
    assert 10 <= skipped <= 40 and float(h.scaler.get_scale()) == 2.0 ** (40 - skipped)
    assert any(not torch.equal(p.detach(), before[n]) for n, p in model.named_parameters())
    assert np.isfinite(losses).all() and np.mean(losses[-8:]) < 0.7 * np.mean(losses[:8])
    ck = checkpoint_dict(h, full=True)
    steps = {int(v["step"]) for v in ck["optimizer"]["state"].values()}
    assert steps == {80 - skipped} and ck["scaler"]["scale"] == 2.0 ** (40 - skipped)


def test_fp16_closed_form_event_step_runs_under_the_scaler():
    from enerf_amd.events import EventOptions
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    from test_gpu_baseline_configs import _event_batch
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
    h = TrainHarness(model, lr=1e-2, occupancy="synthetic", fp16=True)
    opt = EventOptions(C_thres=0.2, use_luma=True, linlog=True, event_only=True)
    data = _event_batch(4096, DEV)
    losses = [float(h.step_events(data, opt)) for _ in range(40)]
    assert h.amp_f16 and np.isfinite(losses).all() and losses[-1] < losses[0]
    assert float(h.scaler.get_scale()) >= 256.0 and h.amp_skipped_steps() <= 8


def test_padding_rows_of_the_sample_budget_are_skipped_without_changing_anything(monkeypatch):
    """fused_render.SKIP_PADDING_ROWS: the MLP kernels take the march's device-side count and leave the budget's
    unfilled rows alone (forward: not computed; backward: zero input gradient).  Image, loss and every gradient must
    equal the run that computes all rows, with a budget well above and one below the batch's real sample count."""
    from enerf_amd import fused_network, fused_render
    from enerf_amd.network import NeRFNetwork
    from enerf_amd import scene
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV).train()
    model.encoder.embeddings.data.uniform_(-0.5, 0.5)
    scene.install_occupancy(model)
    (ro, rd, tgt), = _batches(1, 4096, 2)
    for budget in (180000, 100000):
        outs = []
        for skip in (True, False):
            monkeypatch.setattr(fused_render, "SKIP_PADDING_ROWS", skip)
            model.mean_count = budget
            model.local_step = 0
            for p in model.parameters():
                p.grad = None
            loss = torch.zeros((), device=DEV)
            image, grads = fused_render.train_step_mse(model, ro, rd, tgt, 1, True, loss_out=loss)
            torch.cuda.synchronize()
            names = ["emb", "ws0", "ws1", "wc0", "wc1", "wc2"]
            g = {n: (model.encoder.embeddings.grad if t is None else t).clone() for n, t in zip(names, grads)}
            outs.append((image.clone(), float(loss), g, int(model.step_counter[0, 0])))
            model.encoder.embeddings.grad = None
        (i1, l1, g1, c1), (i0, l0, g0, c0) = outs
        assert c1 == c0 and (c1 < budget) == (budget == 180000)
        assert torch.equal(i1, i0) and abs(l1 - l0) <= 1e-6 * abs(l0)       # (the loss is summed with float atomics)
        for n in g0:
            assert float((g1[n] - g0[n]).abs().max()) <= 1e-6 * float(g0[n].abs().max()) + 1e-12, (budget, n)


@pytest.mark.parametrize("use_luma,linlog", [(True, True), (False, True), (True, False), (False, False)])
def test_fused_event_loss_matches_autograd(use_luma, linlog):
    """enerf_event_loss_fwd_bwd (one launch) against events.event_loss + torch.autograd on the same images: loss, delta
    and both image gradients, all four (use_luma, linlog) variants of nerf/utils.py:499-516, intensities on both sides
    of the lin-log threshold (20 / 255) and of log_thres."""
    from enerf_amd.events import EventOptions, event_loss, event_loss_with_grads
    g = torch.Generator(device=DEV).manual_seed(3)
    n = 4096
    a = torch.rand(1, n, 3, device=DEV, generator=g) ** 3           # plenty of values below 20 / 255
    b = (a + 0.05 * torch.randn(1, n, 3, device=DEV, generator=g)).clamp(1e-4, 1.0)
    a = a.clamp(1e-4, 1.0)
    a[0, :7] = 1e-12                                                  # below log_thres * / 255 (log branch: clamped)
    pols = torch.randint(-3, 4, (1, n), device=DEV, generator=g).float()
    opt = EventOptions(C_thres=0.2, use_luma=use_luma, linlog=linlog, event_only=True)
    loss, delta, g1, g2 = event_loss_with_grads(a, b, pols, opt)
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref_loss, ref_delta = event_loss(ar, br, pols, opt)
    r1, r2 = torch.autograd.grad(ref_loss, [ar, br], allow_unused=True)
    r1 = torch.zeros_like(a) if r1 is None else r1
    r2 = torch.zeros_like(b) if r2 is None else r2
    assert delta.shape == ref_delta.shape
    assert float((delta - ref_delta).abs().max()) <= 1e-6 * max(float(ref_delta.abs().max()), 1.0)
    assert abs(float(loss) - float(ref_loss)) <= 2e-6 * abs(float(ref_loss)) + 1e-12
    for got, want in ((g1, r1), (g2, r2)):
        assert torch.isfinite(got).all()
        assert float((got - want).abs().max()) <= 2e-6 * float(want.abs().max()) + 1e-12


def test_update_step_count_pass_queued_before_the_read_back_changes_nothing():
    """TrainHarness.overlap_update: on steps that start with update_extra_state the render's near/far + count pass are
    queued before the update's 16-byte read-back is waited for (density_update.update_begin / premarch_count /
    update_end) and the write pass follows with the budget.  Same launches in the same order on the device as the plain
    sequence.  With learned occupancy (the bitfield really changes): the first window -- update at step 0 from the
    initial weights, 16 renders against its bitfield -- must give identical counters and the identical first budget;
    later windows see weights that differ in the last bits from run to run (the smallest table levels are summed with
    atomics), so the bitfield may differ in a few threshold cells: losses, parameters and bitfield agree to that."""
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 4096, 2)
    runs = []
    for overlap in (False, True):
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
        h = TrainHarness(model, lr=1e-2, occupancy="learned")
        h.overlap_update = overlap
        losses, budgets, first_window = [], [], None
        for i in range(40):
            nxt = data[(i + 1) % len(data)]
            losses.append(h.step_rgb(*data[i % len(data)], next_rays=(nxt[0], nxt[1])).clone())
            budgets.append(int(model.mean_count))
            if i == 15:
                first_window = (model.step_counter.clone().cpu(), model.density_bitfield.clone(), int(model.local_step))
        runs.append((torch.stack(losses).cpu(), first_window, budgets, model.density_bitfield.clone(),
                     {n: p.detach().clone() for n, p in model.named_parameters()}, int(model.local_step)))
    (l0, w0, b0, f0, p0, s0), (l1, w1, b1, f1, p1, s1) = runs
    assert torch.equal(w0[0], w1[0]) and torch.equal(w0[1], w1[1]) and w0[2] == w1[2] == 16
    assert b0[:17] == b1[:17] and b0[16] > 0 and s0 == s1
    assert all(abs(x - y) <= 0.02 * x for x, y in zip(b0[17:], b1[17:]))
    assert float((f0 != f1).float().mean()) < 2e-3
    assert float(((l0 - l1).abs() / l0.abs().clamp(min=1e-9)).max()) < 2e-2
    for n in p0:
        assert float((p0[n] - p1[n]).abs().mean()) <= 2e-2 * float(p0[n].abs().mean()), n


@pytest.mark.parametrize("net", ["linear", "ff"])
def test_native_step_call_equals_the_python_driven_step(net):
    """enerf_train_step_mse (csrc/train_step.hip: the steady-state closed-form step as ONE library call, the next batch's
    march included) issues the same entry points in the same order as the Python-driven step: same sample counters, same
    loss values, same weights (to the float atomics of the table's smallest levels), for both network families."""
    from enerf_amd import fused_render
    from enerf_amd.trainer import TrainHarness
    if net == "ff":
        from enerf_amd.network_ff import NeRFNetwork
    else:
        from enerf_amd.network import NeRFNetwork
    data = _batches(4, 4096, 2)
    runs = {}
    for native in (True, False):
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        h.native_step = native
        calls = []
        orig = fused_render.train_step_native
        fused_render.train_step_native = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        try:
            losses, counters = [], []
            for i in range(40):
                nxt = data[(i + 1) % 4]
                losses.append(float(h.step_rgb(*data[i % 4], next_rays=(nxt[0], nxt[1]))))
                counters.append(model.step_counter[model.rendered_counter_slot].cpu().clone())
        finally:
            fused_render.train_step_native = orig
        torch.cuda.synchronize()
        runs[native] = (losses, torch.stack(counters), {n: p.detach().clone() for n, p in model.named_parameters()},
                        len(calls), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    (la, ca, pa, na, ga), (lb, cb, pb, nb, gb) = runs[True], runs[False]
    # every step but the first: the cold window (steps 0..15, no sample budget: rows reserved from an earlier render's
    # count) and the steady state; steps 16 and 32 start with update_extra_state and are native from the render on
    assert na == 39 and nb == 0
    assert torch.equal(ca, cb)
    assert np.abs(np.array(la) - np.array(lb)).max() <= 1e-5 * np.abs(lb).max()
    for n, a in pa.items():
        assert float((a - pb[n]).abs().mean()) <= 1e-4 * float(pb[n].abs().mean()) + 1e-9, n
    assert set(ga) == set(gb)


def test_native_event_step_call_equals_the_python_driven_event_step():
    """enerf_train_step_events (csrc/train_step.hip: the steady-state event-only step -- two renders, the event loss, both
    backwards, one optimizer pass, the next step's two marches -- as ONE library call) issues the same entry points in the
    same order as events.train_step_events_manual + FusedAdam.step_grid_table: same sample counters, same losses, same
    weights (to the float atomics of the table's smallest levels)."""
    from enerf_amd import fused_render
    from enerf_amd.events import EventOptions
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 4096, 2)
    opt = EventOptions(C_thres=0.2, use_luma=True, linlog=True, event_only=True)

    def batch(i):
        ro, rd, tg = data[i % len(data)]
        ro2, rd2, _ = data[(i + 1) % len(data)]
        return {"images": tg.view(1, -1, 3), "rays_evs_o1": ro.view(1, -1, 3), "rays_evs_d1": rd.view(1, -1, 3),
                "rays_evs_o2": ro2.view(1, -1, 3), "rays_evs_d2": rd2.view(1, -1, 3),
                "pols": torch.sign(tg[..., 0] - 0.5).view(1, -1)}
    runs = {}
    for native in (True, False):
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        h.native_step = native
        calls = []
        orig = fused_render.train_step_events_native

        def counted(m_, *a, **k):
            out = orig(m_, *a, **k)
            calls.append(int(m_._native_events_ctx["a"].flags))
            return out
        fused_render.train_step_events_native = counted
        try:
            torch.manual_seed(3)                               # the step draws a random background colour
            losses = [h.step_events(batch(i), opt, next_data=batch(i + 1)).clone() for i in range(40)]
        finally:
            fused_render.train_step_events_native = orig
        if native:
            # both renders' samples as ONE batch of 2 M rows (flags bit 1) whenever the two stages were marched together by
            # the previous call: every steady step except the ones right after an update_extra_state
            assert sum(1 for f in calls if f & 2) >= len(calls) - 4 and len(calls) >= 24
        torch.cuda.synchronize()
        runs[native] = (torch.stack(losses).cpu(), model.step_counter.clone().cpu(),
                        {n: p.detach().clone() for n, p in model.named_parameters()}, len(calls),
                        {n for n, p in model.named_parameters() if p.grad is not None})
    # the one-call step with the renders kept apart (the layout before the merge) still agrees with both
    fused_render.MERGE_EVENT_RENDERS = False
    try:
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        torch.manual_seed(3)
        lc = torch.stack([h.step_events(batch(i), opt, next_data=batch(i + 1)).clone() for i in range(40)]).cpu()
        assert int(model._native_events_ctx["a"].flags) == 0
    finally:
        fused_render.MERGE_EVENT_RENDERS = True
    assert float(((lc - runs[False][0]).abs() / runs[False][0].abs().clamp(min=1e-9)).max()) <= 1e-5
    (la, ca, pa, na, ga), (lb, cb, pb, nb, gb) = runs[True], runs[False]
    # (8 steps without a sample budget -- two renders per step fill the 16-slot ring -- then every step is steady)
    assert na >= 24 and nb == 0
    assert torch.equal(ca, cb)
    assert float(((la - lb).abs() / lb.abs().clamp(min=1e-9)).max()) <= 1e-5
    for n, a in pa.items():
        assert float((a - pb[n]).abs().mean()) <= 1e-4 * float(pb[n].abs().mean()) + 1e-9, n
    assert ga == gb


def test_fragments_built_inside_the_grid_forward_equal_their_own_launch():
    """enerf_train_step_mse has the fused MLP's operand fragments built by sixteen extra workgroups of its grid forward's
    launch (csrc/common.h SplitJob, from csrc/nerf_mlp.hip's table of sources) instead of k_nerf_frags: the 90 112 bytes
    must be the same, bit for bit, for the weights every step starts with; and a run with the carried build switched off
    (enerf_debug_carry_frags) sees the same counters and losses."""
    from enerf_amd import _lib as L, fused_network as fnet, fused_render
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    lib = L.lib()
    data = _batches(4, 4096, 2)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    runs = {}
    for carry in (1, 0):
        prev = lib.enerf_debug_carry_frags(carry)
        try:
            torch.manual_seed(0)
            model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
            h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
            weights = fnet.network_params(model)[1:]
            checked = []
            orig = fused_render.train_step_native

            def spy(*a, **k):
                before = [w.detach().clone() for w in weights]
                out = orig(*a, **k)
                if not carry or len(checked) >= 6:
                    return out
                carried = torch.empty(44 * 2048, dtype=torch.uint8, device=DEV)
                L.check(lib.enerf_debug_nerf_frags_copy(carried.data_ptr(), stream()), "frags_copy")
                # the same from k_nerf_frags: a forward over 32 rows with the step's starting weights, nothing vouched for
                seg_s, seg_c = fnet._weight_segments("linear", before)
                B = 32
                feats = torch.zeros(16, B, 2, device=DEV)
                dirs = torch.zeros(B, 3, device=DEV)
                dirs[:, 2] = 1
                sigma, rgb = torch.empty(B, device=DEV), torch.empty(B, 3, device=DEV)
                L.check(lib.enerf_nerf_mlp_forward(feats.data_ptr(), dirs.data_ptr(), seg_s, seg_c,
                                                   fnet._ARCH["linear"]["w0c"], B, 3, sigma.data_ptr(), rgb.data_ptr(), 0,
                                                   stream()), "nerf_mlp_forward")
                own = torch.empty_like(carried)
                L.check(lib.enerf_debug_nerf_frags_copy(own.data_ptr(), stream()), "frags_copy")
                checked.append(bool(torch.equal(carried, own)) and bool(carried.any()))
                return out
            fused_render.train_step_native = spy
            try:
                losses, counters = [], []
                for i in range(24):
                    nxt = data[(i + 1) % 4]
                    losses.append(float(h.step_rgb(*data[i % 4], next_rays=(nxt[0], nxt[1]))))
                    counters.append(model.step_counter[model.rendered_counter_slot].cpu().clone())
            finally:
                fused_render.train_step_native = orig
            torch.cuda.synchronize()
            runs[carry] = (losses, torch.stack(counters), checked)
        finally:
            lib.enerf_debug_carry_frags(prev)
    assert len(runs[1][2]) == 6 and all(runs[1][2]), runs[1][2]
    assert torch.equal(runs[1][1], runs[0][1])
    assert np.abs(np.array(runs[1][0]) - np.array(runs[0][0])).max() <= 1e-5 * np.abs(runs[0][0]).max()


def test_weight_gradients_summed_by_the_optimizer_launch_equal_the_reduce_launch():
    """enerf_train_step_mse leaves the fused MLP backward's per-workgroup weight-gradient sums to k_grid_tile_adam's small-
    tensor section (csrc/common.h PartialSums) instead of launching k_mlp32_reduce_w2: same counters, same losses, the
    same gradients in p.grad and the same weights, to the order of the fp32 sums (enerf_debug_fold_reduce switches back)."""
    from enerf_amd import _lib as L
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    lib = L.lib()
    data = _batches(4, 4096, 2)
    runs = {}
    for fold in (1, 0):
        prev = lib.enerf_debug_fold_reduce(fold)
        try:
            torch.manual_seed(0)
            model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
            h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
            losses, counters = [], []
            for i in range(24):
                nxt = data[(i + 1) % 4]
                losses.append(float(h.step_rgb(*data[i % 4], next_rays=(nxt[0], nxt[1]))))
                counters.append(model.step_counter[model.rendered_counter_slot].cpu().clone())
            torch.cuda.synchronize()
            named = {n: p for n, p in model.named_parameters() if "encoder" not in n}
            runs[fold] = (losses, torch.stack(counters), {n: p.detach().clone() for n, p in named.items()},
                          {n: p.grad.detach().clone() for n, p in named.items()})
        finally:
            lib.enerf_debug_fold_reduce(prev)
    (la, ca, pa, ga), (lb, cb, pb, gb) = runs[1], runs[0]
    assert torch.equal(ca, cb)
    assert np.abs(np.array(la) - np.array(lb)).max() <= 1e-5 * np.abs(lb).max()
    assert len(ga) == 5
    for n in ga:
        assert float(gb[n].abs().max()) > 0
        assert float((ga[n] - gb[n]).abs().max()) <= 2e-4 * float(gb[n].abs().max()), n
        assert float((pa[n] - pb[n]).abs().mean()) <= 1e-4 * float(pb[n].abs().mean()) + 1e-9, n


@contextlib.contextmanager
def _carried_reports():
    """Wraps fused_render._call -> the list of what every one-call step answered: bit 0 of its struct's `report`."""
    from enerf_amd import fused_render
    orig, seen = fused_render._call, []

    def wrapped(*a):
        seen.append(orig(*a))
        return seen[-1]

    fused_render._call = wrapped
    try:
        yield seen
    finally:
        fused_render._call = orig


@pytest.mark.parametrize("n_rays,bound,steps", [(4096, 2, 40), (1000, 3, 36), (16384, 2, 36), (64, 2, 36)])
def test_march_carried_by_the_optimizer_launch_equals_the_side_stream_march(n_rays, bound, steps):
    """csrc/train_step.hip: in the steady state the next batch's march rides in the table optimizer's launch (count pass) and
    one launch behind it (scan + write) instead of a second stream.  Same rays table, same counter, same samples -- bit for
    bit -- hence the same training run: 40 steps with the carried march against 40 with the side-stream march, sample
    counters bit-exact, losses and parameters to the last bits the table's float atomics leave open.
    Every call says in its struct's `report` (bit 0) whether its next march rode that way: summed over the calls, the debug
    counter's difference."""
    from enerf_amd import _lib
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    lib = _lib.lib()
    data = _batches(4, n_rays, bound)
    runs = {}
    prev = lib.enerf_debug_carry_count(-1)
    try:
        for carried in (1, 0):
            lib.enerf_debug_carry_count(carried)
            taken0 = lib.enerf_debug_carry_count(-2)
            torch.manual_seed(0)
            model = NeRFNetwork(encoding="hashgrid", bound=bound, cuda_ray=True, out_dim_color=3).to(DEV)
            h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
            losses, counters = [], []
            with _carried_reports() as reports:
                for i in range(steps):
                    nxt = data[(i + 1) % 4]
                    losses.append(h.step_rgb(*data[i % 4], next_rays=(nxt[0], nxt[1])).detach().clone())
                    counters.append(model.step_counter[model.rendered_counter_slot].clone())
            torch.cuda.synchronize()
            runs[carried] = (torch.stack(losses).cpu(), torch.stack(counters).cpu(),
                             {n: p.detach().clone() for n, p in model.named_parameters()},
                             lib.enerf_debug_carry_count(-2) - taken0, sum(reports))
    finally:
        lib.enerf_debug_carry_count(prev)
    (la, ca, pa, na, ra), (lb, cb, pb, nb, rb) = runs[1], runs[0]
    # (the steady-state steps that have a successor to march: the cold window mirrors its count and keeps the side stream)
    assert na >= steps // 2 - 2 and nb == 0, (na, nb)
    assert ra == na and rb == 0, (ra, na, rb)
    assert torch.equal(ca, cb)
    # (the table's smallest levels are scattered with float atomics, whose order moves last bits from run to run: the bars
    #  are those of the native-call test above)
    #  (small batches scatter EVERY level with atomics: 7e-7 of a 0.06 loss between two runs of the 64-ray case)
    assert float((la - lb).abs().max()) <= (1e-5 if n_rays >= 4096 else 5e-5) * float(lb.abs().max())
    for n, a in pa.items():
        assert float((a - pb[n]).abs().mean()) <= 1e-4 * float(pb[n].abs().mean()) + 1e-9, n


def test_event_marches_carried_by_the_optimizer_launch_equal_the_side_stream_marches():
    """The event-only step's TWO next marches ride in its optimizer launch as two count jobs (the second logs into a chunk log
    of its own, WS_MARCH2) and are scanned + written by two launches behind it: same counters as with the side-stream marches,
    losses and parameters to the last bits the table's float atomics leave open."""
    from enerf_amd import _lib
    from enerf_amd.events import EventOptions
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    lib = _lib.lib()
    data = _batches(4, 4096, 2)
    opt = EventOptions(C_thres=0.2, use_luma=True, linlog=True, event_only=True)

    def batch(i):
        ro, rd, tg = data[i % len(data)]
        ro2, rd2, _ = data[(i + 1) % len(data)]
        return {"images": tg.view(1, -1, 3), "rays_evs_o1": ro.view(1, -1, 3), "rays_evs_d1": rd.view(1, -1, 3),
                "rays_evs_o2": ro2.view(1, -1, 3), "rays_evs_d2": rd2.view(1, -1, 3),
                "pols": torch.sign(tg[..., 0] - 0.5).view(1, -1)}
    runs = {}
    prev = lib.enerf_debug_carry_count(-1)
    try:
        for carried in (1, 0):
            lib.enerf_debug_carry_count(carried)
            taken0 = lib.enerf_debug_carry_count(-2)
            torch.manual_seed(0)
            model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
            h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
            torch.manual_seed(3)                               # the step draws a random background colour
            with _carried_reports() as reports:
                losses = [h.step_events(batch(i), opt, next_data=batch(i + 1)).clone() for i in range(40)]
            torch.cuda.synchronize()
            runs[carried] = (torch.stack(losses).cpu(), model.step_counter.clone().cpu(),
                             {n: p.detach().clone() for n, p in model.named_parameters()},
                             lib.enerf_debug_carry_count(-2) - taken0, sum(reports))
    finally:
        lib.enerf_debug_carry_count(prev)
    (la, ca, pa, na, ra), (lb, cb, pb, nb, rb) = runs[1], runs[0]
    assert na >= 20 and nb == 0, (na, nb)
    assert ra == na and rb == 0, (ra, na, rb)      # (`report` bit 0 of every call, summed: the debug counter's difference)
    assert torch.equal(ca, cb)
    assert float(((la - lb).abs() / lb.abs().clamp(min=1e-9)).max()) <= 1e-5
    for n, a in pa.items():
        assert float((a - pb[n]).abs().mean()) <= 1e-4 * float(pb[n].abs().mean()) + 1e-9, n


@pytest.mark.parametrize("n_rays", [64, 4096])
def test_count_jobs_the_optimizer_launch_did_not_take_are_counted_by_their_own_launch(n_rays):
    """csrc/train_step.hip optimizer(): under loss scaling (enerf_amp_begin: TrainHarness(fp16=True), whose steady-state
    steps are the one-call step) the table optimizer's launch is the form that carries nothing, so the next march's count
    job, prepared for it, runs as a launch of its own (march_carry_count_now) in front of the scan + write.  The marched
    batches are those of the side-stream march: samples depend on the rays and the fixed occupancy only, so the per-step
    sample counters of 12 steps are equal bit for bit.  (The harness reaches the carried march by itself once a sample
    budget exists: the 12 steps follow the cold window and its update_extra_state, 17 steps that are not compared.)"""
    from enerf_amd import _lib
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    lib = _lib.lib()
    data = _batches(4, n_rays, 2)
    runs = {}
    prev = lib.enerf_debug_carry_count(-1)
    try:
        for carried in (1, 0):
            lib.enerf_debug_carry_count(carried)
            torch.manual_seed(0)
            model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
            h = TrainHarness(model, lr=1e-2, occupancy="synthetic", fp16=True)
            assert h.amp_f16
            counters = []
            for i in range(17 + 12):      # (the cold window and its update_extra_state, then 12 steady-state steps)
                nxt = data[(i + 1) % 4]
                h.step_rgb(*data[i % 4], next_rays=(nxt[0], nxt[1]))
                counters.append(model.step_counter[model.rendered_counter_slot].clone())
                if i == 16:
                    taken0 = lib.enerf_debug_carry_count(-2)
            torch.cuda.synchronize()
            runs[carried] = (torch.stack(counters[17:]).cpu(), lib.enerf_debug_carry_count(-2) - taken0)
    finally:
        lib.enerf_debug_carry_count(prev)
    (ca, na), (cb, nb) = runs[1], runs[0]
    assert na > 0 and nb == 0, (na, nb)
    assert int(ca.sum()) > 0 and torch.equal(ca, cb)


def test_model_with_a_staged_ring_copy_deep_copies_and_saves():
    """What the fused routes cache on the module is not model state (renderer._TRANSIENT): with stage_ring_copy's event and
    pinned buffer staged on it -- the window's last step, marches riding on the training stream -- the model still deep-copies
    and pickles, and the copy holds none of it."""
    import copy
    import io
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 4096, 2)
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
    h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
    for i in range(48):
        nxt = data[(i + 1) % 4]
        h.step_rgb(*data[i % 4], next_rays=(nxt[0], nxt[1]))
        if "_ring_copy" in model.__dict__:
            break
    assert "_ring_copy" in model.__dict__ and "_ring_host" in model.__dict__ and "_native_ctx" in model.__dict__
    twin = copy.deepcopy(model)
    torch.save(model, io.BytesIO())
    assert not any(k in twin.__dict__ for k in model._TRANSIENT)
    assert not any(k in model.__getstate__() for k in model._TRANSIENT)
    for (n, p), (n2, p2) in zip(model.named_parameters(), twin.named_parameters()):
        assert n == n2 and torch.equal(p, p2)


def _seven_steps(model, h, data, around_native=None):
    """Step 0 (Python-driven: the cold window's first) and six one-call steps -> (losses, counters); `around_native`
    wraps every call of fused_render.train_step_native."""
    from enerf_amd import fused_render
    calls = []
    orig = fused_render.train_step_native

    def native(*a, **k):
        calls.append(1)
        return orig(*a, **k) if around_native is None else around_native(orig, *a, **k)

    fused_render.train_step_native = native
    try:
        losses, counters = [], []
        for i in range(7):
            nxt = data[(i + 1) % 4]
            losses.append(float(h.step_rgb(*data[i % 4], next_rays=(nxt[0], nxt[1]))))
            counters.append(model.step_counter[model.rendered_counter_slot].cpu().clone())
    finally:
        fused_render.train_step_native = orig
    torch.cuda.synchronize()
    assert len(calls) == (6 if h.native_step else 0)
    return np.array(losses), torch.stack(counters)


def test_process_wide_row_count_does_not_reach_the_one_call_step():
    """The one-call step's MLP launches take their rows from the call's own `counter` field and not from
    enerf_mlp32_valid_rows: a count of 32 rows set process-wide in front of every one-call step changes neither the samples
    nor the losses.  (Skipped rows are left unwritten in the step's own scratch: a step that honoured the setting would
    train on stale values.)
    With `counter` NULL every row of the budget counts (a caller that wants that AND a step sets flags bit 2 instead:
    test_skip_padding_rows_switch_is_honoured_by_the_one_call_step).  Both one-call steps' compositing needs the counter and refuses such a call (so no step can be trained that
    way, on any commit); what the forward has written by then shows the rows its launches took: sigma and rgb of ALL rows,
    bit for bit what the same call writes with no process-wide count set.  (Before the MLP calls took their rows as an
    argument, a NULL counter left the launches to the process's setting: 32 rows written, the rest stale.)"""
    import ctypes
    from enerf_amd import _lib as L
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    lib = L.lib()
    data = _batches(4, 1024, 2)
    t = torch.full((1,), 32, dtype=torch.int32, device=DEV)
    runs = []
    for armed in (False, True):
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")

        def around(orig, *a, **k):
            if armed:
                lib.enerf_mlp32_valid_rows(t.data_ptr())
            return orig(*a, **k)

        try:
            runs.append(_seven_steps(model, h, data, around))
        finally:
            lib.enerf_mlp32_valid_rows(None)
    (la, ca), (lb, cb) = runs
    assert torch.equal(ca, cb)
    assert np.abs(la - lb).max() <= 1e-5 * np.abs(la).max(), (la, lb)
    # the last call's arguments once more (buffers and batch are alive), without a counter and without a next march
    a, bufs = model._native_ctx["a"], model._native_ctx["t"]
    a.loss = a.counter = a.next_rays_o = None
    outs = []
    for armed in (False, True):
        bufs["sigma"].fill_(-7.0)
        bufs["rgb"].fill_(-7.0)
        if armed:
            lib.enerf_mlp32_valid_rows(t.data_ptr())
        try:
            rc = lib.enerf_train_step_mse(ctypes.byref(a))
        finally:
            lib.enerf_mlp32_valid_rows(None)
        assert rc == -1 and b"counter" in lib.enerf_last_error()                # ENERF_E_BADARG, from the compositing
        torch.cuda.synchronize()
        outs.append((bufs["sigma"].clone(), bufs["rgb"].clone()))
    for x, y in zip(*outs):                  # (sigma = exp(.) and rgb = sigmoid(.) are never negative: every row was written)
        assert bool((x != -7.0).all()) and torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_one_call_step_runs_in_its_own_arithmetic_mode():
    """enerf_train_step_args.mlp_precision (here 0: the fp32 MFMA kernels, one launch per net) is the mode of the step's own
    MLP launches, handed to them as an argument: the one-call steps equal the Python-driven ones, which set the mode around
    their launches, and the process's enerf_mlp32_precision reads the same before and after every one-call step."""
    from enerf_amd import _lib as L
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 1024, 2)
    modes = []

    def around(orig, *a, **k):
        before = L.lib().enerf_mlp32_precision(-1)
        out = orig(*a, **k)
        modes.append((before, L.lib().enerf_mlp32_precision(-1)))
        return out

    runs = []
    for native in (True, False):
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
        model.mlp_precision = 0
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        h.native_step = native
        runs.append(_seven_steps(model, h, data, around))
    (la, ca), (lb, cb) = runs
    assert len(modes) == 6 and all(before == after == modes[0][0] != 0 for before, after in modes), modes
    assert torch.equal(ca, cb)
    assert np.abs(la - lb).max() <= 1e-5 * np.abs(lb).max(), (la, lb)


def test_one_call_step_refused_in_the_middle_leaves_nothing_armed():
    """enerf_train_step_mse takes what modifies its MLP launches (valid-row counts, the arithmetic mode, the side stream's
    signal, the two nets' shared reduce launch) and its next march (near / far, the count mirror) as arguments of the
    library's internal entry points.  A step that is refused half-way -- here the next batch's march with
    max_steps = 0, which enerf_march_rays_train_ex rejects by argument validation, after the forward and the MLP backward
    have been issued on the step's rows -- must leave nothing behind: the Python-driven steps that follow on the same model
    see the same samples and losses as on a model that never made the failing call."""
    import ctypes
    from enerf_amd import _lib as L
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 4096, 2)
    runs = []
    for fail in (True, False):
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        for i in range(20):
            nxt = data[(i + 1) % 4]
            h.step_rgb(*data[i % 4], next_rays=(nxt[0], nxt[1]))
        if fail:
            # the last call's arguments once more (its buffers are the context's, its batch is data[3]: all alive), with a
            # next march the library refuses; nothing is launched for that march, so the stage already marched stays intact
            a = model._native_ctx["a"]
            assert a.next_rays_o and a.counter
            a.loss, a.max_steps = None, 0
            rc = L.lib().enerf_train_step_mse(ctypes.byref(a))
            assert rc == -1 and b"max_steps=0" in L.lib().enerf_last_error()          # ENERF_E_BADARG
            a.max_steps = 1024
        h.native_step = False
        losses, counters = [], []
        for i in range(20, 26):
            nxt = data[(i + 1) % 4]
            losses.append(float(h.step_rgb(*data[i % 4], next_rays=(nxt[0], nxt[1]))))
            counters.append(model.step_counter[model.rendered_counter_slot].cpu().clone())
        torch.cuda.synchronize()
        runs.append((np.array(losses), torch.stack(counters)))
    (la, ca), (lb, cb) = runs
    assert torch.equal(ca, cb)
    # (two runs of the same steps agree to the order of the float atomics of the table's smallest levels: the bound the
    #  tests above put on the same pair of routes)
    assert np.abs(la - lb).max() <= 1e-5 * np.abs(lb).max(), (la, lb)


def test_one_call_step_leaves_a_public_mirror_request_alone():
    """enerf_train_step_args.next_count_host is the count mirror of the step's own next march; a request armed with
    enerf_march_mirror_count is for the next PUBLIC march and the step neither takes nor clears it.  The cold window's last
    call once more (its buffers and batch are alive, its next march keeps the side stream: march_flags bit 4) with A armed
    and next_count_host = B: B receives the device counter's two words, A stays untouched, and the public count pass that
    follows writes A -- the request survived the step -- and disarms it."""
    import ctypes
    from enerf_amd import _lib as L
    from enerf_amd.backends import _raymarching as rb
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    lib = L.lib()
    data = _batches(4, 1024, 2)
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
    h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
    _seven_steps(model, h, data)
    a = model._native_ctx["a"]
    assert a.next_rays_o and a.march_flags & 16
    (stage,) = model._premarched.values()                      # the stage the call marched into, and marches into again
    assert stage["counter"].data_ptr() == a.next_counter
    ro, rd = (x.contiguous().view(-1, 3) for x in data[7 % 4][:2])
    assert ro.data_ptr() == a.next_rays_o
    A = torch.full((2,), -1, dtype=torch.int32).pin_memory()
    B = torch.full((2,), -1, dtype=torch.int32).pin_memory()
    rays = torch.empty(1024, 3, dtype=torch.int32, device=DEV)
    counter = torch.zeros(2, dtype=torch.int32, device=DEV)

    def public_count():
        rb.march_rays_train_count(ro, rd, model.density_bitfield, model.bound, 0.0, 1024, 1024, model.cascade,
                                  model.grid_size, stage["nears"], stage["fars"], rays, counter, True, 8)
        torch.cuda.synchronize()

    a.loss = None
    try:
        assert lib.enerf_march_mirror_count(A.data_ptr()) == 0
        a.next_count_host = B.data_ptr()
        assert lib.enerf_train_step_mse(ctypes.byref(a)) == 0, lib.enerf_last_error()
        torch.cuda.synchronize()
        assert a.report & 1 == 0
        assert B.tolist() == stage["counter"].cpu().tolist() and B[0] > 0 and B[1] == 1024
        assert A.tolist() == [-1, -1]
        public_count()
        assert A.tolist() == counter.cpu().tolist() == B.tolist()
        A.fill_(-1)
        public_count()                                         # ... exactly once: nothing is armed any more
        assert A.tolist() == [-1, -1]
    finally:
        lib.enerf_march_mirror_count(None)


def test_skip_padding_rows_switch_is_honoured_by_the_one_call_step(monkeypatch):
    """fused_render.SKIP_PADDING_ROWS off (ENERF_SKIP_PADDING_ROWS=0) on the one-call step: flags bit 2 makes the grid and
    MLP launches take every row of the budget while the compositing keeps the counter it requires.  Rows past the counter
    get zero gradient from the compositing backward, so the steps are those of the default -- counters bit-equal, losses to
    the order of the table's float atomics (the bar the neighbouring tests put on two runs of the same steps)."""
    from enerf_amd import fused_render
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 1024, 2)
    runs, flags = [], []
    for skip in (False, True):
        monkeypatch.setattr(fused_render, "SKIP_PADDING_ROWS", skip)
        torch.manual_seed(0)
        model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        runs.append(_seven_steps(model, h, data))              # (asserts the six native calls)
        flags.append(model._native_ctx["a"].flags)
    (la, ca), (lb, cb) = runs
    assert flags[0] & 4 and not flags[1] & 4, flags
    assert torch.equal(ca, cb)
    print("losses with every row / with the padding skipped:", la, lb)
    assert np.abs(la - lb).max() <= 1e-5 * np.abs(lb).max(), (la, lb)
