"""The normalised event loss (C_thres = -1: enerf_event_loss_fwd_bwd_c's k_event_loss_norm) and the no-event hinge
(enerf_no_event_loss_fwd_bwd_c), csrc/event_pairs.hip, against events.event_loss / events.no_event_loss in FLOAT64 under
autograd on the same inputs -- never against the code under test.  Inputs: tests/test_gpu_event_loss_channels._images.

Tolerance of the normalised loss.  The statement is ill-conditioned: its own fp32 evaluation (torch, same inputs) is off by
up to ~1e-5 of the gradient's maximum.  The kernel is held to 2e-6 * max|want| -- the bar k_event_loss is held to -- plus
twice the error of the fp32 torch statement against the same fp64 (the input's conditioning; the factor 2 for the
device's logf rounding differently from torch's).  The hinge is well conditioned: 2e-6 throughout, rays within 1e-5 of the
kink (where fp32 may land on its other side) left out of the gradient comparison, at most 1 % of a case's rays."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _images(n, C, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.rand(1, n, C, device=DEV, generator=g) ** 3           # plenty of values below 20 / 255
    b = (a + 0.05 * torch.randn(1, n, C, device=DEV, generator=g)).clamp(1e-4, 1.0)
    a = a.clamp(1e-4, 1.0)
    a[0, :min(7, n)] = 1e-12                                         # below log_thres / 255 (log branch: clamped)
    pols = torch.randint(-3, 4, (1, n), device=DEV, generator=g).float()
    return a, b, pols


def _options(C, luma, linlog, C_thres=-1, **kw):
    from enerf_amd.events import EventOptions
    return EventOptions(**dict(dict(out_dim_color=C, C_thres=C_thres, use_luma=luma, linlog=linlog, event_only=True), **kw))


def _statement(a, b, pols, opt, dtype):
    """events.event_loss + autograd in `dtype` -> (loss, delta, g1, g2) as float64 tensors."""
    from enerf_amd.events import event_loss
    ar, br = a.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)
    loss, delta = event_loss(ar, br, pols.to(dtype), opt)
    g1, g2 = torch.autograd.grad(loss, [ar, br], allow_unused=True)
    g1 = torch.zeros_like(ar) if g1 is None else g1
    g2 = torch.zeros_like(br) if g2 is None else g2
    return tuple(t.detach().double() for t in (loss, delta, g1, g2))


def _counted(monkeypatch, name, pick):
    """Counts the calls of library entry `name`: -> the list that receives pick(args) per call."""
    from enerf_amd import _lib as L
    lib, calls = L.lib(), []
    orig = getattr(lib, name)
    monkeypatch.setattr(lib, name, lambda *args: (calls.append(pick(args)), orig(*args))[1])
    return calls


def _check_normalised(monkeypatch, a, b, pols, opt, report=None):
    """The kernel on (a, b, pols) against the fp64 statement, with the module's tolerance; -> the largest ratio of error
    to tolerance seen."""
    from enerf_amd.events import event_loss_with_grads
    calls = _counted(monkeypatch, "enerf_event_loss_fwd_bwd_c", lambda args: (args[6], args[8], args[13]))
    loss, delta, g1, g2 = event_loss_with_grads(a, b, pols, opt)
    C = a.shape[-1]
    assert calls == [(-1, 20.0 if opt.event_only else 400.0, C)]     # the kernel ran: C_thres == -1, the weight, channels
    w_loss, w_delta, w1, w2 = _statement(a, b, pols, opt, torch.float64)
    s_loss, _, s1, s2 = _statement(a, b, pols, opt, torch.float32)
    assert delta.shape == w_delta.shape == (1, a.shape[1], 1 if opt.use_luma else C)
    assert float((delta.double() - w_delta).abs().max()) <= 1e-6 * max(float(w_delta.abs().max()), 1.0)
    worst = 0.0
    for what, got, want, stmt in (("loss", loss, w_loss, s_loss), ("g1", g1, w1, s1), ("g2", g2, w2, s2)):
        assert got.shape == want.shape and torch.isfinite(got).all(), what
        err = float((got.double() - want).abs().max())
        tol = 2e-6 * float(want.abs().max()) + 2.0 * float((stmt - want).abs().max())
        print(f"{what}: err {err:.3e} tol {tol:.3e} max|want| {float(want.abs().max()):.3e} "
              f"fp32 statement err {float((stmt - want).abs().max()):.3e}")
        assert err <= tol + 1e-30, (what, err, tol)
        if tol > 0:
            worst = max(worst, err / tol)
    return worst


# ------------------------------------------------------------------------------------------ 1. the normalised kernel
@pytest.mark.parametrize("n", [2, 1023, 1025])
@pytest.mark.parametrize("linlog", [True, False])
@pytest.mark.parametrize("C,luma", [(1, False), (2, False), (3, False), (3, True)])
def test_normalised_event_loss_matches_fp64_statement(monkeypatch, C, luma, linlog, n):
    a, b, pols = _images(n, C)
    _check_normalised(monkeypatch, a, b, pols, _options(C, luma, linlog))


def test_normalised_event_loss_with_frames_carries_the_weight_400(monkeypatch):
    a, b, pols = _images(1025, 3)
    _check_normalised(monkeypatch, a, b, pols, _options(3, True, True, event_only=False))


# ------------------------------------------------------------------------------------------ 2. degenerate inputs
@pytest.mark.parametrize("C,luma", [(1, False), (3, True)])
def test_equal_images_take_the_subgradient_of_the_norm_at_zero(monkeypatch, C, luma):
    a, _, pols = _images(1025, C)
    _check_normalised(monkeypatch, a, a.clone(), pols, _options(C, luma, True))


@pytest.mark.parametrize("C,luma", [(2, False), (3, True)])
def test_zero_polarities(monkeypatch, C, luma):
    a, b, pols = _images(1025, C)
    _check_normalised(monkeypatch, a, b, torch.zeros_like(pols), _options(C, luma, True))


def test_luma_without_linlog_has_zero_delta_and_exactly_zero_gradients(monkeypatch):
    from enerf_amd.events import event_loss_with_grads
    a, b, pols = _images(1025, 3)
    opt = _options(3, True, False)
    _check_normalised(monkeypatch, a, b, pols, opt)
    loss, delta, g1, g2 = event_loss_with_grads(a, b, pols, opt)
    assert not delta.any() and not g1.any() and not g2.any()
    assert abs(float(loss) - 20.0 / 1025) <= 2e-6 * 20.0 / 1025      # 20 * mean over the N rays of q^2, with |q|_2 = 1


def test_one_ray_cancels_to_nothing(monkeypatch):
    """N = 1: u = q = 1 up to 1e-9, the loss is ~1e-17 and fp32 cannot resolve it (fp32 torch cannot either): return
    code, finiteness and |loss| <= 1e-6 only.  The polarity is set positive, the sign of delta (b > a = 1e-12)."""
    from enerf_amd.events import event_loss_with_grads
    a, b, pols = _images(1, 1)
    pols[:] = 2.0
    opt = _options(1, False, True)
    calls = _counted(monkeypatch, "enerf_event_loss_fwd_bwd_c", lambda args: args[6])
    loss, delta, g1, g2 = event_loss_with_grads(a, b, pols, opt)     # (raises on a return code other than 0)
    assert calls == [-1] and float(delta) > 0
    assert abs(float(_statement(a, b, pols, opt, torch.float64)[0])) <= 1e-6
    assert all(bool(torch.isfinite(t).all()) for t in (loss, delta, g1, g2))
    assert abs(float(loss)) <= 1e-6


# ------------------------------------------------------------------------------------------ 3. the hinge
@functools.lru_cache(maxsize=None)
def _hinge_reference(n, C, luma, C_thres):
    from enerf_amd.events import lin_log, no_event_loss, rgb_to_luma
    a, b, _ = _images(n, C)
    opt = _options(C, luma, True, C_thres=C_thres, w_no_ev=5.0)
    ar, br = a.double().requires_grad_(True), b.double().requires_grad_(True)
    loss = no_event_loss(ar, br, opt)
    g1, g2 = torch.autograd.grad(loss, [ar, br])
    with torch.no_grad():
        la, lb = (rgb_to_luma(ar), rgb_to_luma(br)) if luma else (ar, br)
        excess = (lin_log(lb * 255) - lin_log(la * 255)).abs() - (C_thres if C_thres > 0 else 0.25)
    return a, b, opt, loss.detach(), g1, g2, excess


@pytest.mark.parametrize("n", [1, 1023, 1025])
@pytest.mark.parametrize("C_thres", [0.05, -1])
@pytest.mark.parametrize("C,luma", [(1, False), (2, False), (3, False), (3, True)])
def test_no_event_hinge_matches_fp64_statement(monkeypatch, C, luma, C_thres, n):
    from enerf_amd.events import no_event_loss_with_grads
    a, b, opt, want, w1, w2, excess = _hinge_reference(n, C, luma, C_thres)
    calls = _counted(monkeypatch, "enerf_no_event_loss_fwd_bwd_c", lambda args: (args[2], args[4], args[5], args[9]))
    loss, g1, g2 = no_event_loss_with_grads(a, b, opt)
    assert len(calls) == 1 and calls[0][0] == n and calls[0][2:] == (5.0, C)
    assert abs(calls[0][1] - (0.05 if C_thres > 0 else 0.25)) < 1e-7
    over = float((excess > 0).double().mean())
    print(f"over the threshold: {over:.3f}")
    if n >= 1023:
        assert 0.1 <= over <= 0.9                                    # a hinge that is neither all on nor all off
    assert abs(float(loss) - float(want)) <= 2e-6 * abs(float(want)) + 1e-12
    keep = (excess.abs() >= 1e-5).all(dim=-1, keepdim=True)          # rays clear of the kink, in every entry
    assert int((~keep).sum()) <= n // 100
    for got, ref in ((g1, w1), (g2, w2)):
        assert got.shape == ref.shape and torch.isfinite(got).all()
        err = float(((got.double() - ref) * keep).abs().max())
        print(f"err {err:.3e} max|want| {float(ref.abs().max()):.3e}")
        assert err <= 2e-6 * float(ref.abs().max()) + 1e-30


def test_hinge_gradient_is_zero_where_the_images_agree():
    from enerf_amd.events import no_event_loss_with_grads
    a, _, _ = _images(1025, 3)
    loss, g1, g2 = no_event_loss_with_grads(a, a.clone(), _options(3, False, True, C_thres=0.05, w_no_ev=5.0))
    assert float(loss) == 0.0 and not g1.any() and not g2.any()


# ------------------------------------------------------------------------------------------ 4. refusals
def test_both_entries_refuse_what_they_do_not_serve(monkeypatch):
    from enerf_amd import _lib as L
    from enerf_amd.events import event_loss_with_grads
    n = 64
    lib, s = L.lib(), L.stream_handle()
    a, b, pols = _images(n, 1)
    g1, g2, delta = torch.empty_like(a), torch.empty_like(b), torch.empty(1, n, 1, device=DEV)
    p = lambda t: t.data_ptr()

    def normalised(use_luma, channels, grad2=g2):
        return lib.enerf_event_loss_fwd_bwd_c(p(a), p(b), p(pols), n, use_luma, 1, -1.0, 1e-7, 20.0, p(g1),
                                              None if grad2 is None else p(grad2), p(delta), None, channels, s)

    def hinge(use_luma, channels, grad2=g2):
        return lib.enerf_no_event_loss_fwd_bwd_c(p(a), p(b), n, use_luma, 0.25, 5.0, p(g1),
                                                 None if grad2 is None else p(grad2), None, channels, s)

    for entry in (normalised, hinge):
        assert entry(0, 1) == 0                                      # (what is refused below is not refused wholesale)
        assert entry(1, 1) == -1 and "luma" in lib.enerf_last_error().decode()
        for bad in (0, 4):
            assert entry(0, bad) == -1 and "channels" in lib.enerf_last_error().decode()
        assert entry(0, 1, None) == -1 and "required" in lib.enerf_last_error().decode()
    assert lib.enerf_no_event_loss_fwd_bwd_c(p(a), p(b), 0, 0, 0.25, 5.0, None, None, None, 1, s) == 0   # N == 0
    torch.cuda.synchronize()
    # two batch entries: the norm is per entry, the kernel serves one -- Python keeps autograd
    calls = _counted(monkeypatch, "enerf_event_loss_fwd_bwd_c", lambda args: 1)
    a2, b2, pols2 = (torch.cat([t, t.flip(1)]) for t in (a, b, pols))
    opt = _options(1, False, True)
    loss, delta2, q1, q2 = event_loss_with_grads(a2, b2, pols2, opt)
    assert not calls and delta2.shape == (2, n, 1)
    w_loss, _, w1, _ = _statement(a2, b2, pols2, opt, torch.float32)
    assert float(loss) == float(w_loss) and torch.equal(q1.double(), w1)


# ------------------------------------------------------------------------------------------ 5. the manual route
@pytest.mark.parametrize("variant", ["normalised", "negative_event_sampling"])
def test_manual_route_runs_both_losses_in_the_library_and_matches_autograd(monkeypatch, variant):
    """The setup and bars of test_gpu_gray_marching.test_unfused_losses_run_on_the_manual_route_and_match_autograd; here
    the losses of the manual route are the library's."""
    from enerf_amd.trainer import TrainHarness
    from test_gpu_gray_marching import _batches, _event_batch_of, _gray_options, _model
    data = _batches(4, 2048, 1)

    def batch(i):
        b = _event_batch_of(data, i)
        if variant == "negative_event_sampling":
            v = lambda x: x.view(1, -1, 3)[:, :1024].contiguous()
            (ro3, rd3, _), (ro4, rd4, _) = data[(i + 2) % 4], data[(i + 3) % 4]
            b.update(rays_no_evs_o1=v(ro3), rays_no_evs_d1=v(rd3), rays_no_evs_o2=v(ro4), rays_no_evs_d2=v(rd4))
        return b

    if variant == "normalised":
        opt = _gray_options(C_thres=-1)
        calls = _counted(monkeypatch, "enerf_event_loss_fwd_bwd_c", lambda args: args[6])
        want_calls = [-1] * 24
    else:
        opt = _gray_options(C_thres=0.05, negative_event_sampling=True, w_no_ev=5.0, epoch=2, epoch_start_noEvLoss=0)
        calls = _counted(monkeypatch, "enerf_no_event_loss_fwd_bwd_c", lambda args: args[2])
        want_calls = [1024] * 24
    runs = []
    for manual in (False, True):
        model = _model(1)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        h.manual_mse = manual
        torch.manual_seed(3)
        losses = [h.step_events(batch(i), opt).clone() for i in range(24)]
        runs.append((torch.stack(losses).cpu(), model.step_counter.clone().cpu(),
                     {n: p.detach().clone() for n, p in model.named_parameters()}))
        assert calls == (want_calls if manual else [])
    (l0, c0, p0), (l1, c1, p1) = runs
    assert torch.equal(c0, c1)
    rel = (l0 - l1).abs() / l0.abs().clamp(min=1e-9)
    assert float(rel[:4].max()) < 1e-5 and float(rel.max()) < 3e-4, rel.tolist()
    for n in p0:
        assert float((p0[n] - p1[n]).abs().mean()) <= 2e-3 * float(p0[n].abs().mean()), n


# ------------------------------------------------------------------------------------------ 6. the one-call step
def test_one_call_event_step_serves_the_normalised_loss_on_request():
    """The setup and bars of test_gpu_gray_marching.test_native_event_step_call_equals_the_python_driven_event_step at
    C_thres = -1: with native_normalised the one-call step runs and equals the Python-driven step; by default it stays
    away."""
    from enerf_amd import fused_render
    from enerf_amd.trainer import TrainHarness
    from test_gpu_gray_marching import _batches, _counting, _event_batch_of, _gray_options, _model
    data = _batches(4, 4096, 1)
    opt = _gray_options(C_thres=-1)
    runs = {}
    for mode in ("requested", "python", "default"):
        model = _model(1)
        h = TrainHarness(model, lr=1e-2, occupancy="synthetic")
        assert h.native_normalised is False
        h.native_step = mode != "python"
        h.native_normalised = mode == "requested"
        calls = []
        with _counting(fused_render, "train_step_events_native", calls):
            torch.manual_seed(3)
            losses = [h.step_events(_event_batch_of(data, i), opt, next_data=_event_batch_of(data, i + 1)).clone()
                      for i in range(40)]
        torch.cuda.synchronize()
        runs[mode] = (torch.stack(losses).cpu(), model.step_counter.clone().cpu(),
                      {n: p.detach().clone() for n, p in model.named_parameters()}, len(calls))
    (la, ca, pa, na), (lb, cb, pb, nb) = runs["requested"], runs["python"]
    assert na >= 24 and nb == 0 and runs["default"][3] == 0
    assert torch.equal(ca, cb)
    assert float(((la - lb).abs() / lb.abs().clamp(min=1e-9)).max()) <= 1e-5
    for n, a in pa.items():
        assert float((a - pb[n]).abs().mean()) <= 1e-4 * float(pb[n].abs().mean()) + 1e-9, n
