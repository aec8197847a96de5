"""The compositing kernels at 1 and 2 colour channels (csrc/raymarching.hip, the _c entry points), through the C ABI
wrappers of enerf_amd.backends._raymarching.  A channel's scan does not depend on how many channels run beside it, so
the narrow kernels are held bit for bit to the three-channel kernel fed replicated colours; the MSE forms are held to
the general backward and to fp64.

Rays: sample counts 0, 1, 2, 63, 64, 65, 128, 200 (the empty ray and the edges of the 64-lane chunks) and a ninth ray
whose reservation runs past the buffer (offset + num_steps >= M: dropped, its clipped reservation zero-filled)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
COUNTS = [0, 1, 2, 63, 64, 65, 128, 200]
BGS = ["scalar", "shared", "per_ray"]


def _rb():
    from enerf_amd.backends import _raymarching
    return _raymarching


def _widen(x):
    """[.., C] -> [.., 3]: (c, c, c) for one channel, (c0, c1, c1) for two."""
    return x.expand(*x.shape[:-1], 3).contiguous() if x.shape[-1] == 1 else torch.cat([x, x[..., 1:]], -1).contiguous()


def _case(C, dropped=True, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    counts = COUNTS + ([200] if dropped else [])
    N, used = len(counts), sum(COUNTS)
    M = 640                                              # 523 real samples; the ninth ray reserves [523, 723): dropped
    offs = [sum(counts[:i]) for i in range(N)]
    index = torch.randperm(N, generator=g, device=DEV).to(torch.int32)          # ray ids are not the table's order
    rays = torch.stack([index, torch.tensor(offs, dtype=torch.int32, device=DEV),
                        torch.tensor(counts, dtype=torch.int32, device=DEV)], 1).contiguous()
    rnd = lambda *s: torch.rand(*s, generator=g, device=DEV)
    sigmas = rnd(M) * 20 + 0.01
    deltas = rnd(M, 2) * 0.02 + 1e-3
    rgbs = rnd(M, C)
    counter = torch.tensor([sum(counts), N], dtype=torch.int32, device=DEV)
    return dict(C=C, N=N, M=M, used=used, rays=rays, sigmas=sigmas, deltas=deltas, rgbs=rgbs, counter=counter,
                target=rnd(N, C), g_image=rnd(N, C) - 0.5, g_ws=rnd(N) - 0.5, bg_shared=rnd(C), bg_ray=rnd(N, C))


def _bg(k, form, wide=False):
    if form == "scalar":
        return 0.3
    b = k["bg_shared"] if form == "shared" else k["bg_ray"]
    return _widen(b) if wide else b.contiguous()


def _forward(k, rgbs, bg=None):
    """-> weights_sum, depth, image(, out_image) of the forward (with the blend when a background is given)."""
    N, M, C = k["N"], k["M"], rgbs.shape[1]
    f = dict(dtype=torch.float32, device=DEV)
    ws, depth, image = (torch.full(s, float("nan"), **f) for s in ((N,), (N,), (N, C)))
    if bg is None:
        _rb().composite_rays_train_forward(k["sigmas"], rgbs, k["deltas"], k["rays"], M, N, ws, depth, image)
        return ws, depth, image
    out = torch.full((N, C), float("nan"), **f)
    _rb().composite_rays_train_forward_blend(k["sigmas"], rgbs, k["deltas"], k["rays"], M, N, ws, depth, image, bg, out)
    return ws, depth, image, out


@pytest.mark.parametrize("C", [1, 2])
def test_forward_equals_three_channel_kernel_on_replicated_colours(C):
    k = _case(C)
    ws, depth, image = _forward(k, k["rgbs"])
    ws3, depth3, image3 = _forward(k, _widen(k["rgbs"]))
    assert torch.isfinite(image).all() and float(ws.max()) > 0.5
    assert torch.equal(ws, ws3) and torch.equal(depth, depth3)
    assert torch.equal(image, image3[:, :C])
    dropped = int(k["rays"][-1, 0])
    assert float(ws[dropped]) == 0 and float(image[dropped].abs().max()) == 0


@pytest.mark.parametrize("form", BGS)
@pytest.mark.parametrize("C", [1, 2])
def test_blend_equals_three_channel_kernel_for_every_background_form(C, form):
    k = _case(C)
    ws, depth, image, out = _forward(k, k["rgbs"], _bg(k, form))
    ws3, depth3, image3, out3 = _forward(k, _widen(k["rgbs"]), _bg(k, form, wide=True))
    assert torch.equal(ws, ws3) and torch.equal(depth, depth3) and torch.equal(image, image3[:, :C])
    assert torch.equal(out, out3[:, :C])
    # and the blend is torch's: image + (1 - weights_sum) * bg, multiply and add rounded separately
    bg = _bg(k, form)
    bgt = bg if isinstance(bg, torch.Tensor) else torch.tensor(bg, device=DEV)
    assert torch.equal(out, image + (1 - ws).unsqueeze(-1) * bgt)


def _backward(k, rgbs, g_image, ws, image):
    gs, gr = torch.zeros_like(k["sigmas"]), torch.zeros_like(rgbs)
    _rb().composite_rays_train_backward(k["g_ws"], g_image.contiguous(), k["sigmas"], rgbs, k["deltas"], k["rays"], ws,
                                        image, k["M"], k["N"], gs, gr)
    return gs, gr


def test_general_backward_of_one_channel_equals_three_channel_kernel_fed_zeros():
    """C = 1 with gradient g against the three-channel kernel fed (g, 0, 0): the two extra terms of d sigma are exact
    zeros (0 * finite), and adding them changes no rounding (the library is built without fp contraction)."""
    k = _case(1)
    ws, _, image = _forward(k, k["rgbs"])
    gs, gr = _backward(k, k["rgbs"], k["g_image"], ws, image)
    rgbs3 = _widen(k["rgbs"])
    ws3, _, image3 = _forward(k, rgbs3)
    g3 = torch.cat([k["g_image"], torch.zeros(k["N"], 2, device=DEV)], 1)
    gs3, gr3 = _backward(k, rgbs3, g3, ws3, image3)
    assert float(gs.abs().max()) > 0
    assert torch.equal(gr[:, 0], gr3[:, 0]) and float(gr3[:, 1:].abs().max()) == 0
    assert torch.equal(gs, gs3)
    assert float(gs[k["used"]:].abs().max()) == 0 and float(gr[k["used"]:].abs().max()) == 0      # the dropped ray


@pytest.mark.parametrize("form", BGS)
@pytest.mark.parametrize("C", [1, 2])
def test_fwd_bwd_mse_equals_forward_blend_then_backward_mse(C, form):
    """The header's contract, bit for bit; gradient rows no ray covers are zero (the buffers arrive uninitialised)."""
    k = _case(C)
    N, M, bg = k["N"], k["M"], _bg(k, form)
    scale = 2.0 * 1.7 / (C * N)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)
    ws, _, image, out = _forward(k, k["rgbs"], bg)
    gs, gr, loss = nan(M), nan(M, C), torch.zeros((), device=DEV)
    _rb().composite_rays_train_backward_mse(out, k["target"], scale, bg, k["counter"], k["sigmas"], k["rgbs"], k["deltas"],
                                            k["rays"], ws, image, M, N, gs, gr, loss)
    ws1, image1, out1, gs1, gr1, loss1 = nan(N), nan(N, C), nan(N, C), nan(M), nan(M, C), torch.zeros((), device=DEV)
    _rb().composite_rays_train_fwd_bwd_mse(k["sigmas"], k["rgbs"], k["deltas"], k["rays"], M, N, ws1, image1, bg, out1,
                                           k["target"], scale, k["counter"], gs1, gr1, loss1)
    for a, b in ((ws, ws1), (image, image1), (out, out1), (gs, gs1), (gr, gr1)):
        assert torch.equal(a, b)
    assert torch.isfinite(gs).all() and torch.isfinite(gr).all()
    assert float(gs[k["used"]:].abs().max()) == 0 and float(gr[k["used"]:].abs().max()) == 0
    want = float(((out.double() - k["target"].double()) ** 2).mean())
    for got in (float(loss), float(loss1)):
        assert abs(got - want) <= 1e-6 * want, (got, want)


@pytest.mark.parametrize("form", BGS)
@pytest.mark.parametrize("C", [1, 2])
def test_backward_mse_equals_general_backward_fed_the_loss_gradient(C, form):
    """atol = 1e-6 max|ref|: about ten fp32 roundings on the largest term."""
    k = _case(C)
    N, M, bg = k["N"], k["M"], _bg(k, form)
    scale = 2.0 / (C * N)
    ws, _, image, out = _forward(k, k["rgbs"], bg)
    gs = torch.full((M,), float("nan"), device=DEV)
    gr = torch.full((M, C), float("nan"), device=DEV)
    _rb().composite_rays_train_backward_mse(out, k["target"], scale, bg, k["counter"], k["sigmas"], k["rgbs"], k["deltas"],
                                            k["rays"], ws, image, M, N, gs, gr, None)
    g_image = (out - k["target"]) * scale
    bgt = bg if isinstance(bg, torch.Tensor) else torch.full((C,), bg, device=DEV)
    k2 = dict(k, g_ws=-(g_image * bgt).sum(-1).contiguous())
    gs0, gr0 = _backward(k2, k["rgbs"], g_image, ws, image)
    assert float(gs0.abs().max()) > 0 and float(gr0.abs().max()) > 0
    assert float((gs - gs0).abs().max()) <= 1e-6 * float(gs0.abs().max())
    assert float((gr - gr0).abs().max()) <= 1e-6 * float(gr0.abs().max())


@pytest.mark.parametrize("C", [1, 2])
def test_gradient_rows_past_the_counter_are_zero(C):
    """No dropped ray: the rows [counter, M) belong to nobody and are cleared by the kernels' tail workgroups."""
    k = _case(C, dropped=False)
    N, M = k["N"], k["M"]
    assert int(k["counter"][0]) == k["used"] < M
    ws, _, image, out = _forward(k, k["rgbs"], 0.3)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)
    gs, gr = nan(M), nan(M, C)
    _rb().composite_rays_train_backward_mse(out, k["target"], 2.0 / (C * N), 0.3, k["counter"], k["sigmas"], k["rgbs"],
                                            k["deltas"], k["rays"], ws, image, M, N, gs, gr, None)
    gs1, gr1 = nan(M), nan(M, C)
    _rb().composite_rays_train_fwd_bwd_mse(k["sigmas"], k["rgbs"], k["deltas"], k["rays"], M, N, nan(N), nan(N, C), 0.3,
                                           nan(N, C), k["target"], 2.0 / (C * N), k["counter"], gs1, gr1, None)
    for a, b in ((gs, gr), (gs1, gr1)):
        assert torch.isfinite(a).all() and torch.isfinite(b).all()
        assert float(a[k["used"]:].abs().max()) == 0 and float(b[k["used"]:].abs().max()) == 0
        assert float(a[:k["used"]].abs().max()) > 0


def test_inference_rounds_of_one_channel_equal_three_channel_kernel():
    """composite_rays over two rounds (the second on the survivors of the first), C = 1 against (c, c, c)."""
    N, n_step = 300, 4

    def run(C):
        gg = torch.Generator(device=DEV).manual_seed(10)
        ws, depth, image = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV), torch.zeros(N, C, device=DEV)
        alive = torch.arange(N, dtype=torch.int32, device=DEV)
        t = torch.rand(N, generator=gg, device=DEV) + 0.2
        for rnd_no in range(2):
            n = alive.numel()
            sig = torch.rand(n * n_step, generator=gg, device=DEV) * (400.0 if rnd_no == 0 else 40.0)
            col = torch.rand(n * n_step, 1, generator=gg, device=DEV)
            dl = torch.rand(n * n_step, 2, generator=gg, device=DEV) * 0.02 + 1e-3
            dl.view(n, n_step, 2)[::7, 2:] = 0                      # every seventh ray runs out of samples: it ends
            rgbs = col if C == 1 else _widen(col)
            _rb().composite_rays(n, n_step, alive, t, sig, rgbs.contiguous(), dl, ws, depth, image)
            keep = t >= 0
            alive, t = alive[keep].contiguous(), t[keep].contiguous()
        return ws, depth, image, alive, t

    ws, depth, image, alive, t = run(1)
    ws3, depth3, image3, alive3, t3 = run(3)
    assert 0 < alive.numel() < N
    assert torch.equal(alive, alive3) and torch.equal(t, t3)
    assert torch.equal(ws, ws3) and torch.equal(depth, depth3) and torch.equal(image[:, 0], image3[:, 0])
    assert float(image.max()) > 0


@pytest.mark.parametrize("form", BGS)
@pytest.mark.parametrize("C", [1, 2])
def test_frame_compositing_equals_three_channel_kernel(C, form):
    k = _case(C, dropped=False)
    N, M = k["N"], k["M"]
    k["sigmas"][300:] *= 40                              # some rays saturate: the termination rule runs
    nears = torch.rand(N, device=DEV) * 0.1 + 0.05
    fars = nears + 3.0

    def run(rgbs, bg):
        f = dict(dtype=torch.float32, device=DEV)
        ws, depth, image = (torch.full(s, float("nan"), **f) for s in ((N,), (N,), (N, rgbs.shape[1])))
        used = torch.zeros(1, dtype=torch.int32, device=DEV)
        _rb().composite_rays_frame(k["sigmas"], rgbs, k["deltas"], k["rays"], N, M, nears, fars, bg, ws, depth, image, used)
        return ws, depth, image, int(used)

    ws, depth, image, used = run(k["rgbs"], _bg(k, form))
    ws3, depth3, image3, used3 = run(_widen(k["rgbs"]), _bg(k, form, wide=True))
    assert 0 < used == used3 < k["used"]
    assert torch.equal(ws, ws3) and torch.equal(depth, depth3) and torch.equal(image, image3[:, :C])
    assert torch.isfinite(image).all()


def test_channel_counts_outside_one_to_three_are_refused():
    from enerf_amd import _lib as L
    k = _case(1)
    wide, image = torch.zeros(k["M"], 4, device=DEV), torch.zeros(k["N"], 4, device=DEV)
    rc = L.lib().enerf_composite_rays_train_forward_c(k["sigmas"].data_ptr(), wide.data_ptr(), k["deltas"].data_ptr(),
                                                      k["rays"].data_ptr(), k["M"], k["N"],
                                                      torch.zeros(k["N"], device=DEV).data_ptr(), None, image.data_ptr(), 4,
                                                      L.stream_handle())
    assert rc == -1 and "colour channels" in L.lib().enerf_last_error().decode()
    with pytest.raises(ValueError, match="1..3 colour channels"):
        _forward(k, torch.zeros(k["M"], 4, device=DEV))
