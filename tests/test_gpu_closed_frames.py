"""TrainHarness.closed_frames: step_frames and step_events with event_only = 0 on the closed-form route (the frame term out
of the compositing launch, fused_render.train_step_frames / events.train_step_events_manual) against the autograd route
they leave -- the bars of test_gpu_gray_marching.test_event_step_with_closed_render_backward_matches_autograd_step, which
makes the same kind of comparison -- and, for the combined step, against what the reference's own Python computed
(tests/golden/ref_cuda_ray.npz, keys ev_*)."""
import argparse as ap

import numpy as np
import pytest
import torch

from test_gpu_gray_marching import DEV, _batches, _counting, _event_batch_of, _gray_options, _model
from test_gpu_cuda_ray_vs_reference_fixture import _bring_to_fixture_state, _grad_check
from util import golden

pytestmark = pytest.mark.gpu
STEPS = 40


def _compare(runs):
    (l0, c0, p0), (l1, c1, p1) = runs
    assert torch.equal(c0, c1)
    rel = float(((l0 - l1).abs() / l0.abs().clamp(min=1e-9)).max())
    print(f"losses: max rel diff {rel:.2e}")
    assert rel < 2e-4
    for n in p0:
        d, m = float((p0[n] - p1[n]).abs().mean()), float(p0[n].abs().mean())
        print(f"{n}: mean |diff| / mean |p| = {d / max(m, 1e-30):.2e}")
        assert d <= 2e-3 * m, n


def _state(model, losses):
    torch.cuda.synchronize()
    return (torch.stack(losses).cpu(), model.step_counter.clone().cpu(),
            {n: p.detach().clone() for n, p in model.named_parameters()})


@pytest.mark.parametrize("C", [1, 3])
def test_step_frames_closed_matches_autograd(C):
    """Alpha images on the step's per-pixel background, 40 steps from the same seeds on either route."""
    from enerf_amd import fused_render
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 2048, C)
    g = torch.Generator(device=DEV).manual_seed(5)
    batches = [{"rays_o": ro.view(1, -1, 3), "rays_d": rd.view(1, -1, 3),
                "images": torch.cat([tg, torch.rand(*tg.shape[:-1], 1, generator=g, device=DEV)], -1).view(1, -1, C + 1)}
               for ro, rd, tg in data]
    opt = ap.Namespace(out_dim_color=C, color_space="srgb", render_kwargs={})
    runs = []
    for closed in (False, True):
        model = _model(C)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        assert h.closed_frames is False
        h.closed_frames = closed
        autograd_calls, closed_calls = [], []
        torch.manual_seed(3)                                   # the step draws its background
        with _counting(fused_render, "render_train", autograd_calls), \
                _counting(fused_render, "train_step_frames", closed_calls):
            losses = [h.step_frames(batches[i % 4], opt).clone() for i in range(STEPS)]
        assert (len(autograd_calls), len(closed_calls)) == ((0, STEPS) if closed else (STEPS, 0))
        runs.append(_state(model, losses))
    assert float(runs[0][0][-1]) < float(runs[0][0][0])
    _compare(runs)


def test_background_model_keeps_step_frames_on_autograd():
    """bg_radius > 0: fused_render.supported refuses, the switch changes nothing."""
    from enerf_amd import fused_render
    from enerf_amd.trainer import TrainHarness
    model = _model(1)
    h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
    h.closed_frames = True
    (ro, rd, tg), = _batches(1, 2048, 1)
    assert h._frames_closed_ok(ro, rd, tg, torch.rand_like(tg), {"out_dim_color": 1})
    model.bg_radius = 1.0
    assert not h._frames_closed_ok(ro, rd, tg, 1, {"out_dim_color": 1})
    assert not fused_render.supported(model, ro, rd, 1, 0)


def test_error_map_receives_the_same_per_ray_error():
    """One step on each route from identical state: the same cells of the sampler's error map move, to the same values."""
    from enerf_amd import fused_render, scene
    from enerf_amd.frame_sampler import FrameSampler
    from enerf_amd.trainer import TrainHarness
    H, W = 48, 64
    poses = torch.stack([scene.pose(k) for k in (0, 5, 11)]).to(DEV)
    images = torch.rand(3, H, W, 2, generator=torch.Generator().manual_seed(2)).to(DEV)           # grey + alpha
    opt = ap.Namespace(out_dim_color=1, color_space="srgb", render_kwargs={})
    maps, losses = [], []
    for closed in (False, True):
        sampler = FrameSampler(poses, (32.0, 32.0, 31.6, 24.3), H, W, images=images, num_rays=2048, error_map=True)
        assert tuple(sampler.error_map.shape) == (3, 128 * 128)
        batch = sampler.batch([1], generator=torch.Generator(device=DEV).manual_seed(9))
        model = _model(1)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        h.closed_frames = closed
        torch.manual_seed(3)
        calls = []
        with _counting(fused_render, "train_step_frames", calls):
            losses.append(float(h.step_frames(batch, opt, sampler=sampler)))
        assert len(calls) == int(closed)
        maps.append(sampler.error_map.clone().cpu())
    a, b = maps
    assert torch.equal(a != 1, b != 1) and 0 < int((a != 1).sum()) <= 2048
    assert torch.equal(a[0], torch.ones_like(a[0])) and torch.equal(a[2], torch.ones_like(a[2]))
    rel = float(((a - b).abs() / a.abs()).max())
    print(f"error map: max rel diff {rel:.2e}; losses {losses}")
    assert rel <= 2e-4 and abs(losses[0] - losses[1]) <= 2e-4 * losses[0]


@pytest.mark.parametrize("no_events", [False, True])
def test_event_step_with_frames_closed_matches_autograd(monkeypatch, no_events):
    """event_only = 0, weight_loss_rgb = 0.5: three renders per step (five with negative_event_sampling); the event loss
    of the closed route is the device kernel's."""
    from enerf_amd import events, fused_render
    from enerf_amd.trainer import TrainHarness
    data = _batches(4, 2048, 1)
    extra = dict(C_thres=0.05, negative_event_sampling=True, w_no_ev=5.0, epoch=2, epoch_start_noEvLoss=0) if no_events else {}
    opt = _gray_options(event_only=False, weight_loss_rgb=0.5, **extra)

    def batch(i):
        b = _event_batch_of(data, i)
        ro, rd, tg = data[(i + 2) % 4]                        # the frame: another view's rays with its own pixels
        b.update(rays_o=ro.view(1, -1, 3), rays_d=rd.view(1, -1, 3), images=tg.view(1, -1, 1))
        if no_events:
            v = lambda x: x.view(1, -1, 3)[:, :1024].contiguous()
            (ro3, rd3, _), (ro4, rd4, _) = data[(i + 3) % 4], data[(i + 1) % 4]
            b.update(rays_no_evs_o1=v(ro3), rays_no_evs_d1=v(rd3), rays_no_evs_o2=v(ro4), rays_no_evs_d2=v(rd4))
        return b

    manual_calls, device_loss, raw_renders = [], [], []
    orig = events.train_step_events_manual
    monkeypatch.setattr(events, "train_step_events_manual", lambda *a, **k: (manual_calls.append(1), orig(*a, **k))[1])
    orig_loss = events.event_loss_with_grads
    monkeypatch.setattr(events, "event_loss_with_grads",
                        lambda a, b, *r: (device_loss.append(events._fused_images(a, b) and tuple(a.shape)),
                                          orig_loss(a, b, *r))[1])
    orig_raw = fused_render.render_train_raw
    monkeypatch.setattr(fused_render, "render_train_raw", lambda *a, **k: (raw_renders.append(1), orig_raw(*a, **k))[1])
    runs = []
    for closed in (False, True):
        model = _model(1)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        h.closed_frames = closed
        torch.manual_seed(3)
        # (the closed route marches the next step's event rays ahead -- not behind the last step: those marches would
        #  take counter slots of a step this comparison never runs)
        losses = [h.step_events(batch(i), opt, next_data=batch(i + 1) if closed and i + 1 < STEPS else None).clone()
                  for i in range(STEPS)]
        assert len(manual_calls) == (STEPS if closed else 0)
        runs.append(_state(model, losses))
    assert len(device_loss) == STEPS and set(device_loss) == {(1, 2048, 1)}
    assert len(raw_renders) == STEPS * (5 if no_events else 3)
    _compare(runs)


def test_closed_event_step_with_frames_reproduces_the_reference_python(monkeypatch, mlp32_mode):
    """The fixture's combined step (32 event pairs, 32 frame rays, event_only = 0; minted by the reference's
    train_step_events) on the closed route, after the fixture's two training renders: counters bit-exact, loss and both of
    its terms 2e-4, gradients at test_product_on_the_gpu_reproduces_the_reference_python's bars for this step."""
    from enerf_amd.events import EventOptions, train_step_events_manual
    z = golden("ref_cuda_ray")
    model = _bring_to_fixture_state(z, monkeypatch).cuda()
    o, d = torch.from_numpy(z["rays_o"]).to(DEV), torch.from_numpy(z["rays_d"]).to(DEV)
    for step, (perturb, force, gamma) in enumerate(((True, False, 0.0), (False, True, 1.0 / 256))):
        model.zero_grad()
        out = model.render(o, d, staged=False, bg_color=torch.full((3,), 0.25, device=DEV), perturb=perturb,
                           force_all_rays=force, dt_gamma=gamma, max_steps=256)
        ((out["image"] ** 2).sum() + 0.1 * out["depth"].sum()).backward()
    data = {k[3:]: torch.from_numpy(z[k]).to(DEV) for k in z.files if k.startswith("ev_") and k[3:] in
            ("images", "rays_evs_o1", "rays_evs_d1", "rays_evs_o2", "rays_evs_d2", "pols", "rays_o", "rays_d")}
    opt = EventOptions(use_luma=True, linlog=True, C_thres=0.2, event_only=False)
    model.zero_grad()
    torch.manual_seed(321)
    bg = torch.rand((1, 1, 3)).to(DEV)                              # the reference's host-side draw (nerf/utils.py:487)
    loss, delta, terms = train_step_events_manual(model, data, opt, bg_color=bg, return_terms=True)
    torch.cuda.synchronize()
    assert torch.equal(model.step_counter[:6].cpu(), torch.from_numpy(z["ev_step_counter"]))
    assert int(model.local_step) == int(z["ev_local_step"])
    print(f"loss {float(loss)} / {float(z['ev_loss'])}, evs {float(terms['loss_evs'])} / {float(z['ev_loss_evs'])}, "
          f"frames {float(terms['loss_frames'])} / {float(z['ev_loss_frames'])}")
    np.testing.assert_allclose(float(loss), float(z["ev_loss"]), rtol=2e-4)
    np.testing.assert_allclose(float(terms["loss_evs"]), float(z["ev_loss_evs"]), rtol=2e-4)
    np.testing.assert_allclose(float(terms["loss_frames"]), float(z["ev_loss_frames"]), rtol=2e-4)
    assert terms["loss_no_evs"] is None
    np.testing.assert_allclose(delta.detach().cpu().numpy(), z["ev_delta"], rtol=1e-3, atol=2e-4)
    _grad_check(model, z, "ev", tol=1.7e-2 if mlp32_mode == "split-bf16" else 1.5e-5)
