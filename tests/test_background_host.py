"""enerf_amd.background on the host: every refusal reason on its own, the CPU path of NeRFNetwork.background_from_rays, the
library's two entry points, and the answers of the public route predicates for a background model."""
import ctypes
import types

import pytest
import torch

from enerf_amd import _lib, background

RADIUS = 2.0


def _model(**kw):
    from enerf_amd.gridencoder import GridEncoder
    from enerf_amd.network import NeRFNetwork
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, bg_radius=RADIUS, out_dim_color=kw.pop("out_dim_color", 3), **kw)
    model.encoder_bg = GridEncoder(input_dim=2, num_levels=4, level_dim=2, base_resolution=16, log2_hashmap_size=10,
                                   desired_resolution=2048)                       # (a small table: the tests are about routing)
    return model


def _device_rays(**kw):
    """What `refusals` reads of a ray tensor, answering as fp32 rays on the parameters' device would (no GPU here)."""
    f = dict(is_cuda=True, dtype=torch.float32, requires_grad=False, device=torch.device("cpu"))
    f.update(kw)
    return types.SimpleNamespace(**f)


def test_a_default_background_model_is_served():
    rays = _device_rays()
    assert background.refusals(_model(), rays, rays) == []
    assert background.supported(_model(out_dim_color=1, disable_view_direction=True), rays, rays)


def _disabled(model, monkeypatch):
    monkeypatch.setattr(background, "ENABLED", False)


def _no_bg_net(model, monkeypatch):
    model.bg_net = None


def _encoder_3d(model, monkeypatch):
    from enerf_amd.gridencoder import GridEncoder
    model.encoder_bg = GridEncoder(input_dim=3, num_levels=4, level_dim=2, log2_hashmap_size=8, desired_resolution=64)


def _encoder_level_dim(model, monkeypatch):
    from enerf_amd.gridencoder import GridEncoder
    model.encoder_bg = GridEncoder(input_dim=2, num_levels=4, level_dim=4, log2_hashmap_size=8, desired_resolution=64)


def _encoder_dir(model, monkeypatch):
    from enerf_amd.shencoder import SHEncoder
    model.encoder_dir = SHEncoder(degree=3)


def _three_layers(model, monkeypatch):
    model.bg_net = torch.nn.ModuleList([torch.nn.Linear(24, 64, bias=False), torch.nn.Linear(64, 64, bias=False),
                                        torch.nn.Linear(64, 3, bias=False)])


def _hidden_32(model, monkeypatch):
    model.bg_net = torch.nn.ModuleList([torch.nn.Linear(24, 32, bias=False), torch.nn.Linear(32, 3, bias=False)])


def _bias(model, monkeypatch):
    model.bg_net[1] = torch.nn.Linear(64, 3, bias=True)


def _four_channels(model, monkeypatch):
    model.out_dim_color = 4
    model.bg_net[1] = torch.nn.Linear(64, 4, bias=False)


@pytest.mark.parametrize("reason,change,rays", [
    ("disabled", _disabled, {}),
    ("cpu", None, dict(is_cuda=False)),
    ("dtype", None, dict(dtype=torch.float16)),
    ("ray gradients", None, dict(requires_grad=True)),
    ("no bg_net", _no_bg_net, {}),
    ("encoder_bg", _encoder_3d, {}),
    ("encoder_bg", _encoder_level_dim, {}),
    ("encoder_dir", _encoder_dir, {}),
    ("bg_net", _three_layers, {}),
    ("bg_net", _hidden_32, {}),
    ("bg_net", _bias, {}),
    ("out_dim_color", _four_channels, {}),
])
def test_each_refusal_reason_on_its_own(monkeypatch, reason, change, rays):
    model = _model()
    if change is not None:
        change(model, monkeypatch)
    r = _device_rays(**rays)
    assert background.refusals(model, r, r) == [reason]
    assert not background.supported(model, r, r)


def test_autocast_is_refused(monkeypatch):
    rays = _device_rays()
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    assert background.refusals(_model(), rays, rays) == ["autocast"]


def test_background_from_rays_on_cpu_is_the_statement(cpu_oracle_backend):
    from enerf_amd import raymarching
    model = _model()
    g = torch.Generator().manual_seed(1)
    rd = torch.nn.functional.normalize(torch.randn(257, 3, generator=g), dim=-1)
    ro = 0.4 * RADIUS * (torch.rand(257, 3, generator=g) * 2 - 1)
    calls = background.stats["calls"]
    got = model.background_from_rays(ro, rd)
    want = model.background(raymarching.polar_from_ray(ro, rd, RADIUS), rd)
    assert got.shape == (257, 3) and torch.equal(got, want)
    assert background.stats["calls"] == calls
    # ... and it carries the statement's graph
    got.sum().backward()
    assert model.bg_net[0].weight.grad is not None and model.encoder_bg.embeddings.grad is not None


def test_library_exports_the_two_entry_points():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("enerf_background_forward", 19), ("enerf_background_backward", 22)):
        assert hasattr(raw, name), name
        assert len(_lib.SIGNATURES[name]) == nargs
    assert _lib.header_abi_version() == 13


def test_bad_arguments_are_refused_before_any_launch():
    """C, hidden width, level_dim, levels and NULL pointers are looked at on the host: no device is needed to be told."""
    lib = _lib.lib()
    one = ctypes.c_void_p(64)           # never dereferenced: every case below is refused on its arguments

    def fwd(L=4, level_dim=2, hidden=64, C=3, rays=one, bg=one):
        return lib.enerf_background_forward(rays, one, 2.0, 16, one, one, L, level_dim, 0.0, 16, 0, 1, one, one, hidden, C,
                                            bg, None, None)

    def bwd(L=4, level_dim=2, hidden=64, C=3, grad=one, gw=one):
        return lib.enerf_background_backward(one, one, 2.0, 16, one, one, L, level_dim, 0.0, 16, 0, 1, one, one, hidden, C,
                                             grad, None, gw, one, one, None)
    for f in (fwd, bwd):
        for kw in (dict(C=0), dict(C=4), dict(hidden=32), dict(level_dim=1), dict(L=0), dict(L=background.MAX_LEVELS + 1)):
            assert f(**kw) == -1, (f.__name__, kw)
    assert fwd(rays=None) == -1 and fwd(bg=None) == -1 and bwd(grad=None) == -1 and bwd(gw=None) == -1
    assert b"background" in lib.enerf_last_error()


def test_route_predicates_keep_their_answers_for_a_background_model():
    """The keyword drops the bg_radius clause and nothing else."""
    from enerf_amd import stratified
    model = _model()
    ro = torch.zeros(8, 3)
    assert "bg_radius" in stratified.refusals(model, ro, ro)
    with_kw = stratified.refusals(model, ro, ro, background_model=True)
    assert "bg_radius" not in with_kw
    assert with_kw == [r for r in stratified.refusals(model, ro, ro) if r != "bg_radius"]
    model.mlp_precision = 3                     # the fp16 regime keeps refusing a background model, by name
    assert "background model precision" in stratified.refusals(model, ro, ro, background_model=True)
    assert "background model precision" not in stratified.refusals(model, ro, ro)
    del model.mlp_precision
    bg = torch.zeros(8, 3, requires_grad=True)
    assert "bg_color" in stratified.refusals(model, ro, ro, bg_color=bg)
    assert "bg_color" not in stratified.refusals(model, ro, ro, bg_color=bg, background_model=True)
