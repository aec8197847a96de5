"""Which renders the native stratified route (enerf_amd/stratified.py) turns down.  Host only: `refusals` names every
reason, so each out-of-scope case is checked on its own even with CPU rays."""
import pytest
import torch


def _linear(**kw):
    from enerf_amd.network import NeRFNetwork
    torch.manual_seed(0)
    return NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=False, **kw)


def _rays(n=8):
    o = torch.zeros(1, n, 3)
    o[..., 2] = -3.0
    d = torch.zeros(1, n, 3)
    d[..., 2] = 1.0
    return o, d


def test_cpu_rays_are_refused_and_nothing_else_is():
    from enerf_amd import stratified
    o, d = _rays()
    assert stratified.refusals(_linear(out_dim_color=3), o, d, 0, None, 3) == ["cpu"]
    assert not stratified.supported(_linear(out_dim_color=1), o, d, 0, None, 1)


@pytest.mark.parametrize("case", ["upsample_steps", "bg_radius", "autocast", "ffmlp", "out_dim_color",
                                  "disable_view_direction", "disabled"])
def test_out_of_scope_cases_are_refused(case, monkeypatch):
    from enerf_amd import stratified
    o, d = _rays()
    up, c = 0, 3
    if case == "upsample_steps":
        model, up, reason = _linear(out_dim_color=3), 8, "upsample_steps"
    elif case == "bg_radius":
        model, reason = _linear(out_dim_color=3, bg_radius=1.5), "bg_radius"
    elif case == "ffmlp":
        from enerf_amd.network_ff import NeRFNetwork as FF
        model, reason = FF(encoding="hashgrid", encoding_dir="sphere_harmonics", bound=2, cuda_ray=False), "network"
    elif case == "out_dim_color":
        model, c, reason = _linear(out_dim_color=4), 4, "out_dim_color"
    elif case == "disable_view_direction":
        model, reason = _linear(out_dim_color=3, disable_view_direction=True), "disable_view_direction"
    elif case == "disabled":
        model, reason = _linear(out_dim_color=3), "disabled"
        monkeypatch.setattr(stratified, "ENABLED", False)
    else:
        model, reason = _linear(out_dim_color=3), "autocast"
    if case == "autocast":
        with torch.autocast("cpu", dtype=torch.bfloat16):
            # (torch.is_autocast_enabled() is the CUDA flag: set it the way a CUDA autocast region does)
            prev = torch.is_autocast_enabled()
            torch.set_autocast_enabled(True)
            try:
                why = stratified.refusals(model, o, d, up, None, c)
            finally:
                torch.set_autocast_enabled(prev)
    else:
        why = stratified.refusals(model, o, d, up, None, c)
    assert reason in why, why


def test_background_forms():
    from enerf_amd import stratified
    o, _ = _rays(8)
    C = 3
    assert stratified._background_form(None, o, C) == "const"
    assert stratified._background_form(1, o, C) == "const"
    assert stratified._background_form(torch.rand(C), o, C) == "shared"
    assert stratified._background_form(torch.rand(1, 1, C), o, C) == "shared"
    assert stratified._background_form(torch.rand(8, C), o, C) == "per_ray"
    assert stratified._background_form(torch.rand(1, 8, C), o, C) == "per_ray"
    assert stratified._background_form(torch.rand(8), o, 1) is None                   # (would broadcast to [8, 8])
    assert stratified._background_form(torch.rand(C, requires_grad=True), o, C) is None
    assert stratified._background_form(torch.rand(C, dtype=torch.float64), o, C) is None
    assert stratified._background_form(torch.rand(4, C), o, C) is None


def test_cpu_render_keeps_the_statement(cpu_oracle_backend):
    from enerf_amd import stratified
    model = _linear(out_dim_color=3).eval()
    o, d = _rays(4)
    before = stratified.stats["calls"]
    with torch.no_grad():
        out = model.render(o, d, staged=False, num_steps=16, upsample_steps=0, bg_color=None, perturb=False,
                           out_dim_color=3)
    assert stratified.stats["calls"] == before
    assert out["image"].shape == (1, 4, 3) and out["depth"].shape == (1, 4)
