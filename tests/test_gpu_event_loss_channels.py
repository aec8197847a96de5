"""The fused event loss (enerf_event_loss_fwd_bwd_c, csrc/event_pairs.hip) on images of 1 and 2 channels -- the shipped
grayscale settings: out_dim_color = 1, use_luma = 0 -- against events.event_loss under autograd, with the tolerances
test_gpu_training.test_fused_event_loss_matches_autograd holds the three-channel kernel to.  N = 1, 1023, 1025: one ray,
and either side of the kernel's 1024-thread stride."""
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


@pytest.mark.parametrize("n", [1, 1023, 1025])
@pytest.mark.parametrize("linlog", [True, False])
@pytest.mark.parametrize("C", [1, 2])
def test_fused_event_loss_of_narrow_images_matches_autograd(monkeypatch, C, linlog, n):
    from enerf_amd import _lib as L
    from enerf_amd.events import EventOptions, event_loss, event_loss_with_grads
    a, b, pols = _images(n, C)
    opt = EventOptions(out_dim_color=C, C_thres=0.2, use_luma=False, linlog=linlog, event_only=True)
    lib, calls = L.lib(), []
    orig = lib.enerf_event_loss_fwd_bwd_c
    monkeypatch.setattr(lib, "enerf_event_loss_fwd_bwd_c", lambda *args: (calls.append(args[-2]), orig(*args))[1])
    loss, delta, g1, g2 = event_loss_with_grads(a, b, pols, opt)
    assert calls == [C]                                              # the kernel ran, with this channel count
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref_loss, ref_delta = event_loss(ar, br, pols, opt)
    r1, r2 = torch.autograd.grad(ref_loss, [ar, br], allow_unused=True)
    r1 = torch.zeros_like(a) if r1 is None else r1
    r2 = torch.zeros_like(b) if r2 is None else r2
    assert delta.shape == ref_delta.shape == (1, n, C)
    assert float((delta - ref_delta).abs().max()) <= 1e-6 * max(float(ref_delta.abs().max()), 1.0)
    assert abs(float(loss) - float(ref_loss)) <= 2e-6 * abs(float(ref_loss)) + 1e-12
    for got, want in ((g1, r1), (g2, r2)):
        assert got.shape == want.shape and torch.isfinite(got).all()
        assert float((got - want).abs().max()) <= 2e-6 * float(want.abs().max()) + 1e-12


def test_luma_of_one_channel_is_refused_by_the_entry_point_and_python_takes_autograd(monkeypatch):
    from enerf_amd import _lib as L
    from enerf_amd.events import EventOptions, event_loss_with_grads
    n = 64
    a, b, pols = _images(n, 1)
    g1, g2, delta = torch.empty_like(a), torch.empty_like(b), torch.empty(1, n, 1, device=DEV)
    lib = L.lib()
    rc = lib.enerf_event_loss_fwd_bwd_c(a.data_ptr(), b.data_ptr(), pols.data_ptr(), n, 1, 1, 0.2, 1e-7, 1.0, g1.data_ptr(),
                                        g2.data_ptr(), delta.data_ptr(), None, 1, L.stream_handle())
    assert rc == -1 and "luma" in lib.enerf_last_error().decode()
    for bad in (0, 4):
        assert lib.enerf_event_loss_fwd_bwd_c(a.data_ptr(), b.data_ptr(), pols.data_ptr(), n, 0, 1, 0.2, 1e-7, 1.0,
                                              g1.data_ptr(), g2.data_ptr(), delta.data_ptr(), None, bad,
                                              L.stream_handle()) == -1
    # Python: luma on a one-channel image is not the kernel's business -- whatever event_loss does with it under autograd
    calls = []
    orig = lib.enerf_event_loss_fwd_bwd_c
    monkeypatch.setattr(lib, "enerf_event_loss_fwd_bwd_c", lambda *args: (calls.append(1), orig(*args))[1])
    opt = EventOptions(out_dim_color=1, C_thres=0.2, use_luma=True, linlog=True, event_only=True)
    try:
        event_loss_with_grads(a, b, pols, opt)
    except (RuntimeError, IndexError):                               # rgb_to_luma wants three channels
        pass
    assert not calls
