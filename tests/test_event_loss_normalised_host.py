"""Host-side checks of the normalised event loss and the no-event hinge in HIP (no GPU): the new entry point is declared,
bound and exported with the header still at ABI 13; off the device both *_with_grads functions are autograd of the torch
statements; the one-call step admits the normalised loss only on request."""
import ctypes
import inspect
import os
import re

import pytest
import torch


def test_no_event_entry_point_is_declared_bound_and_exported_at_abi_13():
    from enerf_amd import _lib
    name = "enerf_no_event_loss_fwd_bwd_c"
    assert _lib.header_abi_version() == 13
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "enerf_hip.h")).read()
    assert re.search(r"\bint %s\(" % name, header)
    u32, f32, vp = _lib._u32, _lib._f32, _lib._vp
    # image1, image2, N, use_luma, C_no, upstream, grad_image1, grad_image2, loss, channels, stream
    assert _lib.SIGNATURES[name] == [vp, vp, u32, u32, f32, f32, vp, vp, vp, u32, vp]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.lib().enerf_abi_version() == 13


def _cpu_images(n=257, C=3, seed=1):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(1, n, C, generator=g).clamp(1e-3, 1.0)
    b = (a + 0.05 * torch.randn(1, n, C, generator=g)).clamp(1e-3, 1.0)
    pols = torch.randint(-2, 3, (1, n), generator=g).float()
    return a, b, pols


@pytest.mark.parametrize("kw", [dict(C_thres=-1, use_luma=False, linlog=True, event_only=True),
                                dict(C_thres=-1, use_luma=True, linlog=True, event_only=False),
                                dict(C_thres=-1, use_luma=True, linlog=False, event_only=True),
                                dict(C_thres=0.2, use_luma=False, linlog=True, event_only=True)])
def test_event_loss_with_grads_on_cpu_tensors_is_autograd_of_the_statement(kw):
    from enerf_amd.events import EventOptions, event_loss, event_loss_with_grads
    a, b, pols = _cpu_images()
    opt = EventOptions(**kw)
    loss, delta, g1, g2 = event_loss_with_grads(a, b, pols, opt)
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref_loss, ref_delta = event_loss(ar, br, pols, opt)
    r1, r2 = torch.autograd.grad(ref_loss, [ar, br], allow_unused=True)
    assert torch.equal(delta, ref_delta.detach()) and float(loss) == float(ref_loss.detach())
    assert torch.equal(g1, torch.zeros_like(a) if r1 is None else r1)
    assert torch.equal(g2, torch.zeros_like(b) if r2 is None else r2)


@pytest.mark.parametrize("kw", [dict(C_thres=0.05, use_luma=True), dict(C_thres=-1, use_luma=False),
                                dict(C_thres=0.05, use_luma=False, out_dim_color=1)])
def test_no_event_loss_with_grads_on_cpu_tensors_is_autograd_of_the_statement(kw):
    from enerf_amd.events import EventOptions, no_event_loss, no_event_loss_with_grads
    a, b, _ = _cpu_images(C=kw.get("out_dim_color", 3))
    opt = EventOptions(w_no_ev=5.0, **kw)
    loss, g1, g2 = no_event_loss_with_grads(a, b, opt)
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = no_event_loss(ar, br, opt)
    r1, r2 = torch.autograd.grad(ref, [ar, br])
    assert float(loss) == float(ref) and not loss.requires_grad
    assert torch.equal(g1, r1) and torch.equal(g2, r2)
    assert float(g2.abs().max()) > 0                                 # a hinge that is somewhere active


def test_one_call_step_takes_the_normalised_loss_only_on_request():
    from enerf_amd import fused_render
    p = inspect.signature(fused_render.native_events_supported).parameters
    assert list(p)[:4] == ["model", "data", "loss_opt", "opt"] and p["normalised"].default is False
    from enerf_amd.trainer import TrainHarness
    src = inspect.getsource(TrainHarness.__init__)
    assert re.search(r"self\.native_normalised\s*=\s*False", src)
