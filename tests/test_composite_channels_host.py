"""Host-side checks of the channel-taking compositing interface (no GPU): the CPU oracle stays three-channel, so colours
of any other width are refused before they reach it; the header is at ABI 13 and every _c entry point is bound."""
import re
import os

import pytest
import torch

NEW = ["enerf_composite_rays_train_forward_c", "enerf_composite_rays_train_forward_blend_c",
       "enerf_composite_rays_train_backward_c", "enerf_composite_rays_train_backward_mse_c",
       "enerf_composite_rays_train_fwd_bwd_mse_c", "enerf_composite_rays_c", "enerf_composite_rays_frame_c",
       "enerf_event_loss_fwd_bwd_c"]


@pytest.mark.parametrize("C", [1, 2])
def test_cpu_colours_of_other_widths_never_reach_the_oracle(monkeypatch, C):
    from enerf_amd import raymarching
    reached = []
    monkeypatch.setattr(raymarching._backend, "composite_rays_train_forward", lambda *a: reached.append(a))
    monkeypatch.setattr(raymarching._backend, "composite_rays", lambda *a: reached.append(a))
    M, N = 12, 3
    rays = torch.tensor([[0, 0, 4], [1, 4, 4], [2, 8, 3]], dtype=torch.int32)
    with pytest.raises(ValueError, match=f"C = {C}"):
        raymarching.composite_rays_train(torch.rand(M), torch.rand(M, C), torch.rand(M, 2), rays)
    with pytest.raises(ValueError, match=f"C = {C}"):
        raymarching.composite_rays(N, 4, torch.arange(N, dtype=torch.int32), torch.zeros(N), torch.rand(M), torch.rand(M, C),
                                   torch.rand(M, 2), torch.zeros(N), torch.zeros(N), torch.zeros(N, C))
    assert not reached


def test_channel_counts_above_three_are_refused_everywhere():
    from enerf_amd import raymarching
    with pytest.raises(ValueError, match="C = 4"):
        raymarching.composite_rays_train(torch.rand(4), torch.rand(4, 4), torch.rand(4, 2),
                                         torch.tensor([[0, 0, 3]], dtype=torch.int32))


def test_header_is_at_abi_13_and_binds_the_channel_taking_entry_points():
    from enerf_amd import _lib
    assert _lib.header_abi_version() == 13
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "enerf_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\bint %s\(" % name, header), name
        # one argument more than the three-channel form: the channel count, in front of the stream
        base = _lib.SIGNATURES[name[:-2]]
        assert _lib.SIGNATURES[name] == base[:-1] + [_lib._u32] + base[-1:], name
