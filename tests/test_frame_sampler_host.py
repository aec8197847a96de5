"""enerf_amd/frame_sampler.py on the CPU: its statements of the three kernels of csrc/frame_batch.hip against the fixture
minted from the reference's own get_rays / Trainer.train_step (tests/refcheck/mint_frame_batch_golden.py ->
tests/golden/ref_frame_batch.npz), the selection statement as a sampler, and TrainHarness.step_frames on a CPU model
against the written-out statement of Trainer.train_step (nerf/utils.py:575-636)."""
import copy

import numpy as np
import pytest
import torch

from util import det_fill_, golden, t

CASES = {"s30x50": (30, 50), "s48x64": (48, 64), "s480x640": (480, 640)}
VIEW, N = 2, 257
RAYS_D_BAR = 2e-6      # ~three fp32 roundings on a unit vector, then a 3-term dot product with entries <= 1


def _sampler(g, tag, error_map, **kw):
    from enerf_amd.frame_sampler import FrameSampler
    H, W = CASES[tag]
    s = FrameSampler(t(g[f"{tag}_poses"]), g[f"{tag}_intrinsics"], H, W, num_rays=N, error_map=error_map, **kw)
    if error_map:
        s.error_map[VIEW] = t(g[f"{tag}_error_map_row"])
    return s


def _check_rays(g, tag, kind, b):
    from enerf_amd.frame_sampler import rays_fp64
    H, W = CASES[tag]
    inds = g[f"{tag}_{kind}_inds"]
    assert np.array_equal(b["inds"].numpy(), inds)
    assert b["rays_o"].shape == (1, N, 3) and b["rays_d"].shape == (1, N, 3)
    assert np.array_equal(b["rays_o"].numpy(), g[f"{tag}_{kind}_rays_o"])
    ref = rays_fp64(g[f"{tag}_poses"], VIEW, g[f"{tag}_intrinsics"], W, inds[0])
    err = np.abs(b["rays_d"][0].double().numpy() - ref).max()
    err_ref = np.abs(g[f"{tag}_{kind}_rays_d"][0].astype(np.float64) - ref).max()
    print(f"\n{tag} {kind}: rays_d vs fp64 {err:.3e} (the reference's own {err_ref:.3e})")
    assert err_ref <= RAYS_D_BAR and err <= RAYS_D_BAR, (err, err_ref)
    assert (b["H"], b["W"]) == (H, W)


@pytest.mark.parametrize("tag", list(CASES))
def test_uniform_batch_reproduces_the_reference(tag):
    g = golden("ref_frame_batch")
    b = _sampler(g, tag, False).batch([VIEW], draws={"inds": t(g[f"{tag}_u_inds"])})
    assert "inds_coarse" not in b and "images" not in b
    _check_rays(g, tag, "u", b)


@pytest.mark.parametrize("tag", list(CASES))
def test_error_map_pixel_mapping_reproduces_the_reference(tag):
    g = golden("ref_frame_batch")
    H, W = CASES[tag]
    draws = {k: t(g[f"{tag}_e_{k}"]) for k in ("inds_coarse", "u_row", "u_col")}
    b = _sampler(g, tag, True).batch(torch.tensor([VIEW]), draws=draws)
    assert np.array_equal(b["inds_coarse"].numpy(), g[f"{tag}_e_inds_coarse"]) and b["index"] == [VIEW]
    _check_rays(g, tag, "e", b)
    if tag == "s30x50":                     # the case is there for these: several cells per pixel, the clamp hit
        inds = g[f"{tag}_e_inds"][0]
        assert len(np.unique(inds)) < N and (inds // W == H - 1).any() and (inds % W == W - 1).any()


def test_images_are_gathered_and_the_full_frame_is_a_view():
    from enerf_amd.frame_sampler import FrameSampler, rays_statement
    g = golden("ref_frame_batch")
    H, W = CASES["s30x50"]
    poses = t(g["s30x50_poses"])
    images = torch.rand(3, H, W, 4, generator=torch.Generator().manual_seed(3))
    s = FrameSampler(poses, g["s30x50_intrinsics"], H, W, images=images, num_rays=64)
    b = s.batch(1, generator=torch.Generator().manual_seed(5))
    inds = b["inds"][0]
    assert inds.shape == (64,) and int(inds.min()) >= 0 and int(inds.max()) < H * W
    assert torch.equal(b["images"], images[1].reshape(-1, 4)[inds][None])
    s.num_rays = -1
    full = s.batch(0)
    assert full["images"].shape == (1, H, W, 4) and torch.equal(full["images"][0], images[0])
    ro, rd, _ = rays_statement(poses, 0, g["s30x50_intrinsics"], H, W, torch.arange(H * W))
    assert torch.equal(full["rays_d"][0], rd) and torch.equal(full["rays_o"][0], ro) and "inds" not in full
    s.num_rays = 10 ** 9                    # N = min(num_rays, H W)
    assert s.batch(0)["inds"].shape == (1, H * W)


def test_refusals():
    from enerf_amd.frame_sampler import FrameSampler
    g = golden("ref_frame_batch")
    with pytest.raises(ValueError, match="one view per batch"):
        _sampler(g, "s48x64", False).batch([0, 1])
    s = FrameSampler(t(g["s480x640_poses"]), g["s480x640_intrinsics"], 480, 640, num_rays=16385, error_map=True)
    with pytest.raises(ValueError, match="without replacement"):
        s.batch(0)
    with pytest.raises(ValueError, match="view 3 of 3"):
        s.batch(3)


def test_error_map_write_back_reproduces_the_reference():
    from enerf_amd.frame_sampler import FrameSampler, update_statement
    g = golden("ref_frame_batch")
    new = update_statement(t(g["wb_old"]), t(g["wb_inds_coarse"])[0], t(g["wb_error"])[0])
    assert np.array_equal(new.numpy(), g["wb_new"])
    s = FrameSampler(t(g["s48x64_poses"]), g["s48x64_intrinsics"], 48, 64, error_map=True)
    assert s.error_map.shape == (3, 128 * 128) and bool((s.error_map == 1).all())
    s.error_map[VIEW] = t(g["wb_old"])
    s.update_error([VIEW], t(g["wb_inds_coarse"]), t(g["wb_error"]))
    assert np.array_equal(s.error_map[VIEW].numpy(), g["wb_new"]) and bool((s.error_map[:VIEW] == 1).all())


# ------------------------------------------------------------------------------------------------------ selection
def test_selection_draws_in_proportion_to_the_weights():
    """N = 1, four positive cells of weights 1 : 2 : 3 : 4: 40 000 seeded draws, Pearson's chi-square with 3 degrees of
    freedom at p > 0.001 (critical value 16.266).  The statement sorts along its last axis whatever its length: the 40 000
    draws run on a map of 128 cells (sorting 40 000 x 16384 keys takes half a minute), 2 000 more on the full map."""
    from enerf_amd.frame_sampler import CELLS, select_statement
    gen = torch.Generator().manual_seed(1234)
    for n_cells, cells, draws in ((128, [5, 31, 64, 127], 40000), (CELLS, [5, 4097, 9000, 16383], 2000)):
        w = torch.zeros(n_cells)
        w[cells] = torch.tensor([1.0, 2.0, 3.0, 4.0])
        e = torch.empty(draws, n_cells).exponential_(generator=gen)
        first = select_statement(w, e, 1)[:, 0]
        counts = np.array([int((first == c).sum()) for c in cells], np.float64)
        assert counts.sum() == draws, "a zero-weight cell was drawn before a positive one"
        expect = draws * np.array([0.1, 0.2, 0.3, 0.4])
        chi2 = float(((counts - expect) ** 2 / expect).sum())
        print(f"\n{n_cells} cells: counts {counts}, chi-square {chi2:.3f}")
        assert chi2 < 16.266, (counts, chi2)


def test_selection_order_permutation_zero_weights_and_ties():
    from enerf_amd.frame_sampler import CELLS, select_statement
    gen = torch.Generator().manual_seed(7)
    w = torch.rand(CELLS, generator=gen) ** 4
    zero = torch.randperm(CELLS, generator=gen)[:5000]
    w[zero] = 0
    e = torch.empty(CELLS).exponential_(generator=gen)
    tie = torch.randperm(CELLS, generator=gen)[:64]
    tie = tie[w[tie] > 0]
    w[tie], e[tie] = 0.5, 0.25                                    # exactly equal (weight, e) pairs
    e[int(tie[0]) + 1 if int(tie[0]) + 1 < CELLS else 0] = 0.0    # and one e == 0: key +inf for a positive weight
    order = select_statement(w, e, CELLS)
    assert np.array_equal(np.sort(order.numpy()), np.arange(CELLS))
    n_pos = int((w > 0).sum())
    assert bool((w[order[:n_pos]] > 0).all()) and bool((w[order[n_pos:]] == 0).all())
    with np.errstate(divide="ignore"):
        key = np.where(w.numpy() > 0, w.numpy() / e.numpy(), np.float32(0))
    want = np.lexsort((np.arange(CELLS), -key.astype(np.float64)))   # key descending, then the smaller cell
    assert np.array_equal(order.numpy(), want)
    assert np.array_equal(select_statement(w, e, 33).numpy(), want[:33])
    pos = {int(c): k for k, c in enumerate(order.tolist())}
    ranks = sorted(pos[int(c)] for c in tie)
    assert ranks == list(range(ranks[0], ranks[0] + len(tie)))     # the tied cells sit together ...
    assert [int(c) for c in order[ranks[0]:ranks[0] + len(tie)]] == sorted(int(c) for c in tie)   # ... by cell index


@pytest.mark.parametrize("kind", ["ones", "log_uniform", "zeros", "ties"])
def test_the_kernels_sorting_network_on_the_host(kind):
    """csrc/frame_batch.hip's network and pixel mapping, run thread by thread on the host by the library
    (enerf_debug_error_map_sample_host), against the statement: order included, for every N at once."""
    from enerf_amd import _lib as L
    from enerf_amd.frame_sampler import CELLS, pixels_statement, select_statement
    gen = torch.Generator().manual_seed(len(kind))
    e = torch.empty(CELLS).exponential_(generator=gen)
    w = {"ones": torch.ones(CELLS), "log_uniform": 10.0 ** (-30.0 * torch.rand(CELLS, generator=gen))}.get(
        kind, torch.rand(CELLS, generator=gen) ** 3 + 1e-3)
    if kind == "zeros":
        w[torch.randperm(CELLS, generator=gen)[:5000]] = 0
        e[int(w.argmax())] = 0.0                                  # key +inf
    if kind == "ties":
        tie = torch.randperm(CELLS, generator=gen)[:64]
        w[tie], e[tie] = 0.75, 0.125
    u_row, u_col = torch.rand(CELLS, generator=gen), torch.rand(CELLS, generator=gen)
    for H, W in CASES.values():
        coarse, inds = torch.empty(CELLS, dtype=torch.int64), torch.empty(CELLS, dtype=torch.int64)
        L.check(L.lib().enerf_debug_error_map_sample_host(w.data_ptr(), e.data_ptr(), u_row.data_ptr(), u_col.data_ptr(),
                                                          CELLS, H, W, coarse.data_ptr(), inds.data_ptr()), "host sample")
        want = select_statement(w, e, CELLS)
        assert torch.equal(coarse, want)
        assert torch.equal(inds, pixels_statement(want, u_row, u_col, H, W))


# ------------------------------------------------------------------------------------------------------ step_frames
def _cpu_model(seed):
    from enerf_amd.network import NeRFNetwork
    model = NeRFNetwork(encoding="frequency", encoding_dir="frequency", bound=3, cuda_ray=False, out_dim_color=1)
    det_fill_(list(model.parameters()), seed, -0.25, 0.25)
    return model


def test_step_frames_equals_the_written_out_train_step(cpu_oracle_backend):
    from enerf_amd import scene
    from enerf_amd.events import EventOptions
    from enerf_amd.frame_sampler import FrameSampler
    from enerf_amd.trainer import TrainHarness
    H, W, C = 48, 64, 1
    poses = torch.stack([scene.pose(k) for k in (0, 5, 11)])
    images = torch.rand(3, H, W, C + 1, generator=torch.Generator().manual_seed(2))      # (grey + alpha)
    sampler = FrameSampler(poses, (32.0, 32.0, 31.6, 24.3), H, W, images=images, num_rays=96, error_map=True)
    batch = sampler.batch([1], generator=torch.Generator().manual_seed(9))
    assert batch["images"].shape == (1, 96, C + 1)
    opt = EventOptions(out_dim_color=C, render_kwargs={"num_steps": 32, "upsample_steps": 0})
    model = _cpu_model(91)
    twin = copy.deepcopy(model).train()
    h = TrainHarness(model, lr=5e-3)
    before = sampler.error_map.clone()
    torch.manual_seed(500)
    loss = h.step_frames(batch, opt, sampler=sampler)
    assert h.global_step == 1
    # Trainer.train_step, written out (nerf/utils.py:575-636)
    torch.manual_seed(500)
    im = batch["images"]
    bg = torch.rand_like(im[..., :C])
    gt = im[..., :C] * im[..., C:] + bg * (1 - im[..., C:])
    pred = twin.render(batch["rays_o"], batch["rays_d"], staged=False, bg_color=bg, perturb=True, num_steps=32,
                       upsample_steps=0, out_dim_color=C)["image"]
    per_ray = torch.nn.MSELoss(reduction="none")(pred, gt).mean(-1)
    want = float(per_ray.detach().mean())
    assert abs(float(loss) - want) <= 1e-6 * abs(want), (float(loss), want)
    assert any(not torch.equal(p, q) for p, q in zip(model.parameters(), twin.parameters())), "no optimizer step"
    # the map: the EMA at inds_coarse of view 1, untouched everywhere else
    coarse = batch["inds_coarse"][0]
    assert len(set(coarse.tolist())) == 96
    changed = (sampler.error_map != before).nonzero()
    assert set(changed[:, 0].tolist()) == {1}
    assert sorted(changed[:, 1].tolist()) == sorted(coarse.tolist())
    ema = 0.1 * before[1].gather(0, coarse) + 0.9 * per_ray.detach()[0]
    assert torch.allclose(sampler.error_map[1, coarse], ema, rtol=1e-5, atol=0)
    # without a sampler (or an error map) the step is the same and writes nothing
    b2 = {k: v for k, v in batch.items() if k not in ("inds_coarse", "index")}
    assert torch.isfinite(h.step_frames(b2, opt)) and h.global_step == 2


def test_step_frames_linear_colour_space_leaves_the_batch_alone(cpu_oracle_backend):
    from enerf_amd.evaluate import srgb_to_linear
    from enerf_amd.events import EventOptions
    from enerf_amd.trainer import TrainHarness
    g = torch.Generator().manual_seed(4)
    o = torch.tensor([[0.0, 0.0, -4.5]]).expand(1, 32, 3).contiguous()
    d = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, 1.0]) + 0.2 * torch.rand(1, 32, 3, generator=g), dim=-1)
    images = torch.rand(1, 32, 1, generator=g)
    kept = images.clone()
    model = _cpu_model(17)
    twin = copy.deepcopy(model).train()
    h = TrainHarness(model, lr=5e-3)
    opt = EventOptions(out_dim_color=1, color_space="linear", render_kwargs={"num_steps": 16, "upsample_steps": 0})
    torch.manual_seed(3)
    loss = h.step_frames({"rays_o": o, "rays_d": d, "images": images}, opt)
    assert torch.equal(images, kept)
    torch.manual_seed(3)
    gt = srgb_to_linear(images)
    bg = torch.rand_like(gt)
    pred = twin.render(o, d, staged=False, bg_color=bg, perturb=True, num_steps=16, upsample_steps=0,
                       out_dim_color=1)["image"]
    want = float(((pred.detach() - gt) ** 2).mean(-1).mean())
    assert abs(float(loss) - want) <= 1e-6 * abs(want)
