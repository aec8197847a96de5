"""The frame batch on the device (enerf_amd/frame_sampler.py, csrc/frame_batch.hip): the three
kernels against the reference fixture and the module's statements, FrameSampler.batch from a generator,
TrainHarness.step_frames in fp32 and in the stratified route's fp16 regime, and the frame term of the event step."""
import copy
import functools

import numpy as np
import pytest
import torch

from util import golden, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = {"s30x50": (30, 50), "s48x64": (48, 64), "s480x640": (480, 640)}
VIEW, NFIX = 2, 257
RAYS_D_BAR = 2e-6      # ~three fp32 roundings on a unit vector, then a 3-term dot product with entries <= 1


def _dev(a):
    return t(a).to(DEV)


# ------------------------------------------------------------------------------------------------------ 1. rays
@pytest.mark.parametrize("tag", list(CASES))
def test_frame_batch_against_the_fixture_and_the_statement(tag):
    from enerf_amd.frame_sampler import FrameSampler, rays_fp64, rays_statement
    g = golden("ref_frame_batch")
    H, W = CASES[tag]
    poses, intr = g[f"{tag}_poses"], g[f"{tag}_intrinsics"]
    gen = torch.Generator().manual_seed(H)
    worst = 0.0
    for Ci in (None, 1, 3, 4):
        images = None if Ci is None else torch.rand(3, H, W, Ci, generator=gen).to(DEV)
        for index in (0, 2):
            for n in (1, 33, NFIX, 4096):
                s = FrameSampler(_dev(poses), intr, H, W, images=images, num_rays=n)
                N = min(n, H * W)
                fixture = n == NFIX and index == VIEW
                inds = t(g[f"{tag}_u_inds"])[0] if fixture else torch.randint(0, H * W, [N], generator=gen)
                if n == 33:
                    inds[:2] = torch.tensor([0, H * W - 1])             # the first and the last pixel
                b = s.batch([index], draws={"inds": inds.to(DEV)})
                assert b["rays_o"].shape == b["rays_d"].shape == (1, N, 3) and b["inds"].shape == (1, N)
                assert torch.equal(b["inds"][0].cpu(), inds)
                assert torch.equal(b["rays_o"][0].cpu(), t(poses)[index, :3, 3].expand(N, 3))
                err = np.abs(b["rays_d"][0].double().cpu().numpy() - rays_fp64(poses, index, intr, W, inds.numpy())).max()
                worst = max(worst, err)
                assert err <= RAYS_D_BAR, (Ci, index, n, err)
                _, rd, _ = rays_statement(t(poses), index, intr, H, W, inds)
                assert (b["rays_d"][0].cpu() - rd).abs().max() <= RAYS_D_BAR
                if Ci is None:
                    assert "images" not in b
                else:
                    assert torch.equal(b["images"][0], images[index].reshape(H * W, Ci)[inds.to(DEV)])
                if fixture:
                    assert np.array_equal(b["rays_o"].cpu().numpy(), g[f"{tag}_u_rays_o"])
                    assert np.abs(b["rays_d"].cpu().numpy() - g[f"{tag}_u_rays_d"]).max() <= 2 * RAYS_D_BAR
    print(f"\n{tag}: rays_d vs fp64, worst {worst:.3e}")


def test_full_frame():
    from enerf_amd.frame_sampler import FrameSampler, rays_fp64
    g = golden("ref_frame_batch")
    H, W = CASES["s30x50"]
    images = torch.rand(3, H, W, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    s = FrameSampler(_dev(g["s30x50_poses"]), g["s30x50_intrinsics"], H, W, images=images, num_rays=-1)
    b = s.batch(2)
    assert b["rays_d"].shape == (1, H * W, 3) and b["images"].shape == (1, H, W, 3) and torch.equal(b["images"][0], images[2])
    ref = rays_fp64(g["s30x50_poses"], 2, g["s30x50_intrinsics"], W, np.arange(H * W))
    assert np.abs(b["rays_d"][0].double().cpu().numpy() - ref).max() <= RAYS_D_BAR
    assert torch.equal(b["rays_o"][0].cpu(), t(g["s30x50_poses"])[2, :3, 3].expand(H * W, 3))


# ------------------------------------------------------------------------------------------------------ 2. selection
@functools.lru_cache(maxsize=None)
def _selection_inputs(kind):
    """(weights, e, u_row, u_col) on the CPU and, computed once, the statement's full order."""
    from enerf_amd.frame_sampler import CELLS, select_statement
    gen = torch.Generator().manual_seed({"ones": 1, "log_uniform": 2, "zeros": 3, "ties": 4}[kind])
    e = torch.empty(CELLS).exponential_(generator=gen)
    if kind == "ones":
        w = torch.ones(CELLS)                                           # every key decided by e
    elif kind == "log_uniform":
        w = 10.0 ** (-30.0 * torch.rand(CELLS, generator=gen))          # 1e-30 .. 1
    else:
        w = torch.rand(CELLS, generator=gen) ** 3 + 1e-3
    if kind == "zeros":
        w[torch.randperm(CELLS, generator=gen)[:5000]] = 0
    if kind == "ties":
        tie = torch.randperm(CELLS, generator=gen)[:64]
        w[tie], e[tie] = 0.75, 0.125                                    # 64 exactly equal (weight, e) pairs, a large key
    u_row, u_col = torch.rand(CELLS, generator=gen), torch.rand(CELLS, generator=gen)
    return w, e, u_row, u_col, select_statement(w, e, CELLS)


def _tied_run(w, order):
    """Where the 64 tied cells (weight 0.75) sit in `order`: (first rank, the cells in that order)."""
    ranks = (w[order] == 0.75).nonzero()[:, 0]
    return int(ranks[0]), order[ranks].tolist()


@pytest.mark.parametrize("kind", ["ones", "log_uniform", "zeros", "ties"])
def test_error_map_sample_against_the_statement(kind):
    from enerf_amd.frame_sampler import CELLS, error_map_sample, pixels_statement
    w, e, u_row, u_col, order = _selection_inputs(kind)
    if kind == "ties":
        # the test's own premise: the tied cells (key 6) sit together in the statement's order, by cell index, behind
        # the cells with e < w / 6 and within the first 4096: N = 4096 and N = 16384 below contain the whole run
        start, cells = _tied_run(w, order)
        assert len(cells) == 64 and cells == sorted(cells) and order[start:start + 64].tolist() == cells
        assert 1 <= start and start + 64 <= 4096
    for k, N in enumerate((1, 33, 4096, CELLS)):
        H, W = list(CASES.values())[(k + len(kind)) % 3]
        coarse, inds = error_map_sample(w.to(DEV), e.to(DEV), u_row[:N].to(DEV).contiguous(),
                                        u_col[:N].to(DEV).contiguous(), H, W)
        assert coarse.dtype == inds.dtype == torch.int64 and coarse.shape == inds.shape == (N,)
        assert torch.equal(coarse.cpu(), order[:N]), (kind, N)
        assert torch.equal(inds.cpu(), pixels_statement(order[:N], u_row[:N], u_col[:N], H, W)), (kind, N)
        if N == CELLS:
            assert torch.equal(coarse.sort().values.cpu(), torch.arange(CELLS))
        if kind == "zeros":
            n_pos = CELLS - 5000
            assert bool((w[coarse.cpu()[:n_pos]] > 0).all()) and bool((w[coarse.cpu()[n_pos:]] == 0).all())


@pytest.mark.parametrize("tag", list(CASES))
def test_pixel_mapping_against_the_fixture(tag):
    from enerf_amd.frame_sampler import FrameSampler, rays_fp64
    g = golden("ref_frame_batch")
    H, W = CASES[tag]
    s = FrameSampler(_dev(g[f"{tag}_poses"]), g[f"{tag}_intrinsics"], H, W, num_rays=NFIX, error_map=True)
    b = s.batch([VIEW], draws={k: _dev(g[f"{tag}_e_{k}"]) for k in ("inds_coarse", "u_row", "u_col")})
    assert np.array_equal(b["inds"].cpu().numpy(), g[f"{tag}_e_inds"])
    assert np.array_equal(b["inds_coarse"].cpu().numpy(), g[f"{tag}_e_inds_coarse"]) and b["index"] == [VIEW]
    assert np.array_equal(b["rays_o"].cpu().numpy(), g[f"{tag}_e_rays_o"])
    ref = rays_fp64(g[f"{tag}_poses"], VIEW, g[f"{tag}_intrinsics"], W, g[f"{tag}_e_inds"][0])
    assert np.abs(b["rays_d"][0].double().cpu().numpy() - ref).max() <= RAYS_D_BAR


# ------------------------------------------------------------------------------------------------------ 3. write-back
@pytest.mark.parametrize("N", [1, 4096, 128 * 128])
def test_error_map_update_is_the_torch_statement_bit_for_bit(N):
    from enerf_amd.frame_sampler import CELLS, FrameSampler
    g = golden("ref_frame_batch")
    gen = torch.Generator().manual_seed(N)
    s = FrameSampler(_dev(g["s48x64_poses"]), g["s48x64_intrinsics"], 48, 64, error_map=True)
    s.error_map.copy_(torch.rand(3, CELLS, generator=gen))
    before = s.error_map.clone()
    coarse = torch.randperm(CELLS, generator=gen)[:N].to(DEV)
    err = torch.rand(1, N, generator=gen).to(DEV)
    s.update_error([1], coarse[None], err)
    want = before.clone()
    want[1].scatter_(0, coarse, 0.1 * before[1].gather(0, coarse) + 0.9 * err[0])
    assert torch.equal(s.error_map.view(torch.int32), want.view(torch.int32))
    untouched = torch.ones(CELLS, dtype=torch.bool, device=DEV)
    untouched[coarse] = False
    assert torch.equal(s.error_map[1][untouched], before[1][untouched]) and int(untouched.sum()) == CELLS - N


def test_write_back_reproduces_the_reference():
    from enerf_amd.frame_sampler import FrameSampler
    g = golden("ref_frame_batch")
    s = FrameSampler(_dev(g["s48x64_poses"]), g["s48x64_intrinsics"], 48, 64, error_map=True)
    s.error_map[VIEW] = _dev(g["wb_old"])
    s.update_error([VIEW], _dev(g["wb_inds_coarse"]), _dev(g["wb_error"]))
    assert np.array_equal(s.error_map[VIEW].cpu().numpy(), g["wb_new"]) and bool((s.error_map[:VIEW] == 1).all())


# ------------------------------------------------------------------------------------------------------ 4. generator
@functools.lru_cache(maxsize=None)
def _scene_sampler_inputs():
    """Four views of the analytic scene at its own 640 x 480: poses and grey images [4, 480, 640, 1] on the device."""
    from enerf_amd import scene
    from enerf_amd.events import rgb_to_luma
    from test_gpu_stratified_fp16 import _teacher
    poses = torch.stack([scene.pose(k) for k in (0, 7, 14, 21)]).to(DEV)
    inds = torch.arange(scene.H * scene.W, device=DEV)
    images = torch.stack([rgb_to_luma(_teacher(*scene.pixel_rays(p, inds, DEV)), esim=True)[0] for p in poses.cpu()])
    return poses, images.reshape(4, scene.H, scene.W, 1).contiguous()


def _scene_sampler(num_rays=1024, error_map=False):
    from enerf_amd import scene
    from enerf_amd.frame_sampler import FrameSampler
    poses, images = _scene_sampler_inputs()
    return FrameSampler(poses, scene.INTRINSICS, scene.H, scene.W, images=images, num_rays=num_rays, error_map=error_map)


@pytest.mark.parametrize("error_map", [False, True])
def test_batch_from_a_generator(error_map):
    from enerf_amd import events, scene
    s = _scene_sampler(4096, error_map)
    if error_map:
        s.error_map.copy_(torch.rand(4, 128 * 128, generator=torch.Generator().manual_seed(2)) + 0.01)
    a = s.batch([3], generator=torch.Generator(device=DEV).manual_seed(5))
    b = s.batch([3], generator=torch.Generator(device=DEV).manual_seed(5))
    c = s.batch([3], generator=torch.Generator(device=DEV).manual_seed(6))
    keys = ["rays_o", "rays_d", "images", "inds"] + (["inds_coarse"] if error_map else [])
    assert set(keys) <= set(a)
    for k in keys:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["inds"], c["inds"])
    inds = a["inds"][0]
    assert int(inds.min()) >= 0 and int(inds.max()) < scene.H * scene.W
    if error_map:
        assert len(set(a["inds_coarse"][0].tolist())) == 4096
    ref = events.get_rays(s.poses[3:4], scene.INTRINSICS, scene.H, scene.W, 4096, inds=inds)
    assert torch.equal(a["rays_o"], ref["rays_o"])
    assert (a["rays_d"] - ref["rays_d"]).abs().max() <= 2 * RAYS_D_BAR            # (each within the bar of fp64)
    assert torch.equal(a["images"][0], s.images[3].reshape(-1, 1)[inds])


# ------------------------------------------------------------------------------------------------------ 5. step_frames
KW = {"num_steps": 64, "upsample_steps": 0}


def _harness(fp16=False, seed=0):
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    torch.manual_seed(seed)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=False, out_dim_color=1).to(DEV)
    return TrainHarness(model, lr=1e-2, fp16=fp16)


def _opt(**kw):
    from enerf_amd.events import EventOptions
    return EventOptions(out_dim_color=1, use_luma=False, linlog=True, C_thres=0.2, render_kwargs=dict(KW), **kw)


def test_step_frames_fp32_first_loss_and_error_map_training():
    from enerf_amd import stratified
    s = _scene_sampler(1024, error_map=True)
    h = _harness()
    twin = copy.deepcopy(h.model).train()
    gen = torch.Generator(device=DEV).manual_seed(3)
    batch = s.batch([0], generator=gen)
    calls = stratified.stats["calls"]
    torch.manual_seed(1)
    losses = [float(h.step_frames(batch, _opt(), sampler=s))]
    assert stratified.stats["calls"] == calls + 1
    # Trainer.train_step, written out (nerf/utils.py:575-636)
    torch.manual_seed(1)
    bg = torch.rand_like(batch["images"])
    pred = twin.render(batch["rays_o"], batch["rays_d"], staged=False, bg_color=bg, perturb=True, out_dim_color=1,
                       **KW)["image"]
    want = float(((pred.detach() - batch["images"]) ** 2).mean(-1).mean())
    assert abs(losses[0] - want) <= 1e-6 * abs(want), (losses[0], want)
    sampled = {v: set() for v in range(4)}
    sampled[0] |= set(batch["inds_coarse"][0].tolist())
    for i in range(1, 48):
        batch = s.batch([i % 4], generator=gen)
        sampled[i % 4] |= set(batch["inds_coarse"][0].tolist())
        losses.append(float(h.step_frames(batch, _opt(), sampler=s)))
    print(f"\nfirst 4 {np.mean(losses[:4]):.5f}, last 4 {np.mean(losses[-4:]):.5f}")
    assert np.isfinite(losses).all() and np.mean(losses[-4:]) < np.mean(losses[:4])
    changed = (s.error_map != 1).cpu()
    for v in range(4):
        assert set(changed[v].nonzero()[:, 0].tolist()) <= sampled[v]
        assert int(changed[v].sum()) >= 0.99 * len(sampled[v])      # (an error of exactly 1 would leave a cell at 1)


def _frame_batches(n):
    s = _scene_sampler(1024)
    gen = torch.Generator(device=DEV).manual_seed(11)
    return [s.batch([i % 4], generator=gen) for i in range(n)]


def test_step_frames_in_the_native_fp16_regime_against_autocast():
    from enerf_amd import stratified
    from test_gpu_stratified_fp16 import _check_against_autocast
    batches = _frame_batches(4)

    def train(fp16):
        h = _harness(fp16)
        torch.manual_seed(1)
        return h, np.array([float(h.step_frames(batches[i % 4], _opt())) for i in range(48)])
    calls = stratified.stats["calls"]
    h, native = train(True)
    assert h.strat_f16 and not h.fp16
    assert stratified.stats["calls"] == calls + 48
    ha, auto = train("autocast")
    assert ha.fp16 and not ha.strat_f16
    assert stratified.stats["calls"] == calls + 48
    print(f"\nnative {native[0]:.5f} -> {native[-4:].mean():.5f}, autocast {auto[0]:.5f} -> {auto[-4:].mean():.5f}")
    _check_against_autocast(native, auto, h)


def _train_events_and_frames(fp16, event_only, steps=24):
    from test_gpu_stratified_fp16 import _event_batch
    frames = _frame_batches(4)
    batches = [{**_event_batch(1024, 100 + i), **{k: frames[i][k] for k in ("rays_o", "rays_d", "images")}}
               for i in range(4)]
    h = _harness(fp16)
    opt = _opt(event_only=event_only)
    torch.manual_seed(1)
    return h, np.array([float(h.step_events(batches[i % 4], opt)) for i in range(steps)])


def test_event_step_with_a_frame_term_in_the_native_fp16_regime():
    from enerf_amd import stratified
    from test_gpu_stratified_fp16 import _check_against_autocast
    calls = stratified.stats["calls"]
    h, native = _train_events_and_frames(True, False)
    assert h.strat_f16
    assert stratified.stats["calls"] == calls + 3 * 24
    ha, auto = _train_events_and_frames("autocast", False)
    assert stratified.stats["calls"] == calls + 3 * 24
    print(f"\nnative {native[0]:.5f} -> {native[-4:].mean():.5f}, autocast {auto[0]:.5f} -> {auto[-4:].mean():.5f}")
    _check_against_autocast(native, auto, h)
    # event-only, no negative sampling: as before, the two event renders
    calls = stratified.stats["calls"]
    h, losses = _train_events_and_frames(True, True, steps=4)
    assert stratified.stats["calls"] == calls + 2 * 4 and np.isfinite(losses).all()
