"""The native stratified route (enerf_amd/stratified.py, csrc/stratified.hip) against the PyTorch statement it replaces
(sampler.render_stratified), on the same GPU: sample points bit for bit, the reference's own fixtures, both arms on
the same model and rays, a CUDA-graph capture of forward + backward, and 20 event-only training steps."""
import contextlib

import numpy as np
import pytest
import torch

from util import golden, det_fill_, t, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"


@contextlib.contextmanager
def route(on):
    from enerf_amd import stratified
    prev = stratified.ENABLED
    stratified.ENABLED = on
    try:
        yield
    finally:
        stratified.ENABLED = prev


@contextlib.contextmanager
def mlp_precision(mode):
    from enerf_amd import _lib
    prev = _lib.lib().enerf_mlp32_precision(mode)
    try:
        yield
    finally:
        _lib.lib().enerf_mlp32_precision(prev)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _hit_rays(n, seed, radius=3.5, spread=1.5):
    """n rays from outside the box (bound 2) towards points inside it: every ray hits."""
    g = np.random.default_rng(seed)
    v = g.normal(size=(n, 3))
    o = radius * v / np.linalg.norm(v, axis=1, keepdims=True)
    d = g.uniform(-spread, spread, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return torch.tensor(o, dtype=torch.float32), torch.tensor(d, dtype=torch.float32)


def _empty_rays(n, seed):
    """n rays that cross the box along x inside the slab z < -1, where _scene's density is ~1e-9: no masked sample."""
    g = np.random.default_rng(seed)
    o = np.stack([np.full(n, -3.5), g.uniform(-1.8, 1.8, n), g.uniform(-1.9, -1.1, n)], -1)
    d = np.stack([np.ones(n), g.uniform(-0.1, 0.1, n), g.uniform(-0.05, 0.05, n)], -1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return torch.tensor(o, dtype=torch.float32), torch.tensor(d, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------------ 1. points
def _native_points(ro, rd, aabb, T, min_near, u):
    from enerf_amd import _lib as L
    N = ro.shape[0]
    f = dict(dtype=torch.float32, device=DEV)
    nears, fars, z, xyz = torch.empty(N, **f), torch.empty(N, **f), torch.empty(N, T, **f), torch.empty(N * T, 3, **f)
    lin = float(np.float32(1) / np.float32(T - 1))
    inv = float(np.float32(1) / np.float32(T))
    L.check(L.lib().enerf_stratified_points(ro.data_ptr(), rd.data_ptr(), aabb.data_ptr(), N, T, min_near, lin, inv,
                                            u.data_ptr() if u is not None else None, nears.data_ptr(), fars.data_ptr(),
                                            z.data_ptr(), xyz.data_ptr(), L.stream_handle()), "stratified_points")
    return nears, fars, z, xyz


@pytest.mark.parametrize("bound", [2, 3])
@pytest.mark.parametrize("T", [24, 128, 512])
@pytest.mark.parametrize("N", [1, 24, 4096])
def test_points_bit_equal_to_the_statement(N, T, bound):
    from enerf_amd import raymarching, sampler
    from util import camera_rays
    o, d = camera_rays(N, 100 + N + T, bound)               # (a few of them miss the box)
    ro, rd = torch.from_numpy(o).to(DEV).contiguous(), torch.from_numpy(d).to(DEV).contiguous()
    if N >= 24:                                            # and these surely do
        ro[:4] = torch.tensor([10.0, 10.0, 10.0], device=DEV)
        rd[:4] = torch.tensor([0.0, 0.0, 1.0], device=DEV)
    aabb = torch.tensor([-bound] * 3 + [bound] * 3, dtype=torch.float32, device=DEV)
    nears, fars = raymarching.near_far_from_aabb(ro, rd, aabb, 0.2)
    nears, fars = nears.unsqueeze(-1), fars.unsqueeze(-1)
    for perturb in (False, True):
        torch.manual_seed(5)
        z_ref, _ = sampler.stratified_depths(nears, fars, T, perturb)
        pts_ref = sampler._points(ro, rd, z_ref, aabb).reshape(-1, 3)
        u = None
        if perturb:
            torch.manual_seed(5)
            u = torch.rand((N, T), device=DEV)
        n_, f_, z, xyz = _native_points(ro, rd, aabb, T, 0.2, u)
        assert torch.equal(_bits(n_), _bits(nears[:, 0])) and torch.equal(_bits(f_), _bits(fars[:, 0]))
        bad = (_bits(z) != _bits(z_ref)).sum().item()
        assert bad == 0, f"perturb={perturb}: {bad} depths differ, e.g. {z[_bits(z) != _bits(z_ref)][:4].tolist()} vs " \
                         f"{z_ref[_bits(z) != _bits(z_ref)][:4].tolist()}"
        assert torch.equal(_bits(xyz), _bits(pts_ref)), f"perturb={perturb}"


# ------------------------------------------------------------------------------------------------------ 2. fixtures
def _make_network():
    from enerf_amd.network import NeRFNetwork
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=False, out_dim_color=3)
    det_fill_(list(model.parameters()), 41)
    return model


def test_reference_fixture_eval_on_the_native_route():
    from enerf_amd import stratified
    g = golden("ref_run_up0")
    model = _make_network().to(DEV).eval()
    calls = stratified.stats["calls"]
    with mlp_precision(0), torch.no_grad():
        out = model.render(t(g["rays_o"]).to(DEV), t(g["rays_d"]).to(DEV), staged=False, bg_color=None, perturb=False,
                           num_steps=24, upsample_steps=0, out_dim_color=3)
    assert stratified.stats["calls"] == calls + 1
    assert_close(out["image"], g["image"], rtol=1e-4, atol=1e-5)
    assert_close(out["depth"], g["depth"], rtol=1e-4, atol=1e-5)


def test_reference_fixture_gradients_on_the_native_route():
    from enerf_amd import stratified
    g = golden("ref_run_train")
    model = _make_network().to(DEV).train()
    calls = stratified.stats["calls"]
    with mlp_precision(0):
        out = model.render(t(g["rays_o"]).to(DEV), t(g["rays_d"]).to(DEV), staged=False,
                           bg_color=torch.full((3,), 0.25, device=DEV), perturb=False, num_steps=24, upsample_steps=0,
                           out_dim_color=3)
        ((out["image"] ** 2).sum() + out["depth"].sum()).backward()
    assert stratified.stats["calls"] == calls + 1
    assert_close(out["image"], g["image"], rtol=1e-4, atol=1e-5)
    assert_close(model.sigma_net[0].weight.grad, g["g_sigma0"], rtol=1e-3, atol=1e-5)
    assert_close(model.color_net[2].weight.grad, g["g_color2"], rtol=1e-3, atol=1e-5)
    assert_close(model.encoder.embeddings.grad[:4920], g["g_emb_l0"], rtol=1e-3, atol=1e-6)
    assert_close(model.encoder.embeddings.grad.abs().sum(), g["g_emb_sum"], rtol=1e-4)


# ------------------------------------------------------------------------------------------------------ 3. on vs off
def _scene(C, seed=3):
    """A bound-2 network whose density is ~1e7 for z > 0 (rays that reach it saturate: 1 - alpha == 0 in fp32) and
    ~1e-9 for z < -1 (rays that stay there have no masked sample).  Level 0 of the grid is dense (x fastest, z
    slowest): its rows from 2048 on (z > ~0) are +1, the rows below -1; the other levels are small noise.  The sigma
    net's output row 0 is signed so that h0 = +P on the + side and -Q on the - side (P, Q > 0)."""
    from enerf_amd.network import NeRFNetwork
    torch.manual_seed(seed)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=False, out_dim_color=C)
    det_fill_(list(model.parameters()), seed)
    with torch.no_grad():
        emb = model.encoder.embeddings
        n0 = int(model.encoder.offsets[1])
        emb.mul_(0.01)
        rows = torch.arange(n0)
        emb[:n0] = torch.where(rows >= 2048, 1.0, -1.0).unsqueeze(-1).expand(n0, 2)
        w0 = model.sigma_net[0].weight
        s = w0[:, 0] + w0[:, 1]
        model.sigma_net[1].weight[0] = torch.where(s > 0, 1.0, -1.0)
    return model


def _arm(model, ro, rd, T, bg, on):
    """One render + backward of Σimage² + Σdepth.  The MLP kernels run their fp32 arithmetic here: the two arms feed the
    colour net's first layer in different column orders, and under the split-bf16 default that alone moves a colour by
    ~1e-5 (the sigma values and weights stay bit-equal) -- more than the bar this comparison holds the compositing to."""
    from enerf_amd import stratified
    model.zero_grad(set_to_none=True)
    calls = stratified.stats["calls"]
    stratified.KEEP_LAST = True
    try:
        with route(on), mlp_precision(0):
            out = model.render(ro, rd, staged=False, bg_color=bg, perturb=False, num_steps=T, upsample_steps=0,
                               out_dim_color=model.out_dim_color)
            ((out["image"] ** 2).sum() + out["depth"].sum()).backward()
    finally:
        stratified.KEEP_LAST = False
    assert stratified.stats["calls"] == calls + (1 if on else 0)
    # (the statement leaves the colour net out of the graph when no sample is masked: no gradient is zero gradient)
    grads = {n: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for n, p in
             model.named_parameters()}
    return out["image"].detach(), out["depth"].detach(), grads, (stratified.last if on else None)


def _close_rel(a, b, rel, what):
    scale = b.abs().max().item()
    err = (a - b).abs().max().item()
    assert err <= rel * max(scale, 1e-30), f"{what}: max |diff| {err:.3e} vs max |ref| {scale:.3e}"


@pytest.mark.parametrize("bg_form", ["none", "shared", "per_ray"])
@pytest.mark.parametrize("C", [1, 3])
def test_route_on_vs_off(C, bg_form):
    _on_vs_off(C, bg_form, 512)


@pytest.mark.parametrize("T", [1100])
@pytest.mark.parametrize("bg_form", ["none", "shared", "per_ray"])
@pytest.mark.parametrize("C", [1, 3])
def test_route_on_vs_off_beyond_one_pass(C, bg_form, T):
    """The same at more than one scan pass per ray (64 lanes x 8 samples = 512): the carried product, the T_k kept in
    g_sigma between the backward's sweeps, the recount of earlier passes' rows and the reverse carry all run."""
    _on_vs_off(C, bg_form, T)


def _on_vs_off(C, bg_form, T):
    N = 4096
    model = _scene(C).to(DEV).train()
    o1, d1 = _hit_rays(N - 512, 11)
    o2, d2 = _empty_rays(512, 12)
    ro = torch.cat([o1, o2]).to(DEV)[None]
    rd = torch.cat([d1, d2]).to(DEV)[None]
    g = torch.Generator(device=DEV).manual_seed(9)
    bg = {"none": None, "shared": torch.rand(C, device=DEV, generator=g),
          "per_ray": torch.rand(1, N, C, device=DEV, generator=g)}[bg_form]
    img1, dep1, gr1, last = _arm(model, ro, rd, T, bg, True)
    img0, dep0, gr0, _ = _arm(model, ro, rd, T, bg, False)
    w, count = last["w"], last["count"]
    # the scene does what it is meant to: saturated rays, rays without a masked sample
    with torch.no_grad():
        sig = model.density(torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, -1.5]], device=DEV))["sigma"]
    assert sig[0].item() > 1e5 and sig[1].item() < 1e-4, sig
    assert (count[-512:] == 0).all().item()
    assert (count[:-512] > 0).sum().item() > 1000
    assert (w.sum(-1) > 1 - 1e-6).sum().item() > 100
    assert int(count.sum().item()) == int((w > 1e-4).sum().item())
    # The statement's own weights (its z and points are bit-equal to the route's, its density is the same kernels):
    # they differ from the route's by rounding (the product is scanned in another order), and where a weight sits within
    # that rounding of the 1e-4 threshold the two masks disagree -- the colour of that sample (w ~ 1e-4) is in one image
    # and not in the other.  Those rays are held to the size of one such sample, every other ray to 1e-5.
    flip = _mask_flips(model, ro, rd, T, w)
    assert int(flip.sum().item()) <= 4, int(flip.sum().item())
    keep = ~flip
    assert_close(img1[0][keep], img0[0][keep], rtol=0, atol=1e-5)
    assert_close(dep1[0][keep], dep0[0][keep], rtol=0, atol=1e-5)
    assert_close(img1, img0, rtol=0, atol=5e-4)
    assert_close(dep1, dep0, rtol=0, atol=1e-5)
    for n in gr0:
        _close_rel(gr1[n], gr0[n], 1e-4, n)


def _mask_flips(model, ro, rd, T, w):
    """Rays on which the statement's mask (w > 1e-4) differs from the route's; also checks that the two sets of
    weights agree to rounding."""
    from enerf_amd import raymarching, sampler
    with torch.no_grad(), mlp_precision(0):                   # (the arithmetic _arm ran the MLPs in)
        o, d = ro.reshape(-1, 3), rd.reshape(-1, 3)
        nears, fars = raymarching.near_far_from_aabb(o, d, model.aabb_train, model.min_near)
        nears, fars = nears.unsqueeze(-1), fars.unsqueeze(-1)
        z, width = sampler.stratified_depths(nears, fars, T, False)
        sigma = model.density(sampler._points(o, d, z, model.aabb_train).reshape(-1, 3))["sigma"].view(-1, T)
        w_ref, _ = sampler.ray_weights(z, sigma, width, model.density_scale)
    assert (w - w_ref).abs().max().item() < 1e-6
    return ((w > 1e-4) != (w_ref > 1e-4)).any(dim=1)


@contextlib.contextmanager
def _nan_buffers():
    """The route's uninitialised buffers (stratified.py's torch.empty) come NaN-filled -- what a freed NaN block of the
    caching allocator hands out, on every allocation: a pad row the kernels fail to zero shows up as a NaN gradient."""
    import types
    from enerf_amd import stratified

    class _Torch(types.ModuleType):
        def __getattr__(self, name):
            return getattr(torch, name)

    def empty(*shape, **kw):
        t = torch.empty(*shape, **kw)
        return t.fill_(float("nan")) if t.is_floating_point() else t

    proxy = _Torch("torch")
    proxy.empty = empty
    prev = stratified.torch
    stratified.torch = proxy
    try:
        yield
    finally:
        stratified.torch = prev


@pytest.mark.parametrize("kind", ["every_sample_masked", "partly_masked"])
def test_pad_rows_with_nan_filled_buffers(kind):
    """N*T not a multiple of 32.  Every sample masked (low uniform density: the compact list is as long as its capacity,
    total == cap) or some (the list ends inside a 32-row tile whose pad rows the MLP kernels process as real rows: the
    colour rows and d rgb there must be zero).  Every buffer the route leaves for its kernels to fill starts as NaN; the
    gradients must be finite and those of the statement."""
    C = 3
    N, T = (3, 24) if kind == "every_sample_masked" else (5, 24)
    model = _scene(C).to(DEV).train()
    if kind == "every_sample_masked":
        with torch.no_grad():
            model.encoder.embeddings.zero_()                  # features 0 -> h0 = 0 -> sigma = 1 everywhere
    o, d = _hit_rays(N, 31)
    ro, rd = o.to(DEV)[None], d.to(DEV)[None]
    bg = torch.full((C,), 0.4, device=DEV)
    img0, dep0, gr0, _ = _arm(model, ro, rd, T, bg, False)
    with _nan_buffers():
        img1, dep1, gr1, last = _arm(model, ro, rd, T, bg, True)
    total = int(last["incl"][-1].item())
    if kind == "every_sample_masked":
        assert total == N * T and (N * T) % 32 != 0
    else:
        assert 0 < total < N * T and total % 32 != 0, total
    assert not _mask_flips(model, ro, rd, T, last["w"]).any()
    for n in gr1:
        assert torch.isfinite(gr1[n]).all(), n
    assert_close(img1, img0, rtol=0, atol=1e-5)
    assert_close(dep1, dep0, rtol=0, atol=1e-5)
    for n in gr0:
        _close_rel(gr1[n], gr0[n], 1e-4, n)


def test_batch_without_masked_samples():
    N, T = 1024, 512
    model = _scene(3).to(DEV).train()
    o, d = _empty_rays(N, 13)
    ro, rd = o.to(DEV)[None], d.to(DEV)[None]
    bg = torch.full((3,), 0.3, device=DEV)
    img1, dep1, gr1, last = _arm(model, ro, rd, T, bg, True)
    img0, dep0, gr0, _ = _arm(model, ro, rd, T, bg, False)
    assert int(last["count"].sum().item()) == 0
    assert_close(img1, img0, rtol=0, atol=1e-5)
    assert_close(dep1, dep0, rtol=0, atol=1e-5)
    for n in gr0:
        _close_rel(gr1[n], gr0[n], 1e-4, n)
    assert gr1["color_net.2.weight"].abs().max().item() == 0.0


# ------------------------------------------------------------------------------------------------------ 4. graphs
def test_forward_backward_captured_in_a_cuda_graph():
    from enerf_amd import _lib, stratified
    N, T = 2048, 256
    model = _scene(3).to(DEV).train()
    o, d = _hit_rays(N, 21)
    ro, rd = o.to(DEV)[None], d.to(DEV)[None]
    bg = torch.full((3,), 0.5, device=DEV)
    params = list(model.parameters())

    def step():
        out = model.render(ro, rd, staged=False, bg_color=bg, perturb=False, num_steps=T, upsample_steps=0,
                           out_dim_color=3)
        loss = (out["image"] ** 2).sum() + out["depth"].sum()
        loss.backward()
        return loss.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            for p in params:
                p.grad = None
            eager = step()
        eager_grads = [p.grad.clone() for p in params]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gen = _lib.lib().enerf_workspace_generation()
    calls = stratified.stats["calls"]
    for p in params:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = step()
    assert stratified.stats["calls"] == calls + 1
    for p in params:
        p.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _lib.lib().enerf_workspace_generation() == gen
    assert_close(static_loss, eager, rtol=1e-6, atol=0)
    for p, ge in zip(params, eager_grads):
        _close_rel(p.grad, ge, 1e-5, "graph vs eager")


# ------------------------------------------------------------------------------------------------------ 5. training
def _event_batch(n, seed):
    from enerf_amd import scene
    g = torch.Generator().manual_seed(seed)
    inds = torch.randint(0, scene.H * scene.W, (n,), generator=g)
    (o1, d1) = scene.pixel_rays(scene.pose(5), inds, "cpu")
    (o2, d2) = scene.pixel_rays(scene.pose(5 + 1.0 / (360.0 / 32)), inds, "cpu")
    pols = torch.where(torch.rand(1, n, generator=g) < 0.5, -1.0, 1.0)
    data = {"images": torch.zeros(1, n, 1), "rays_evs_o1": o1, "rays_evs_d1": d1, "rays_evs_o2": o2,
            "rays_evs_d2": d2, "pols": pols}
    return {k: v.to(DEV) for k, v in data.items()}


def _train(on, steps=20, n=4096):
    from enerf_amd import events
    from enerf_amd.events import EventOptions
    from enerf_amd.network import NeRFNetwork
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=False, out_dim_color=1).to(DEV).train()
    opt = EventOptions(out_dim_color=1, use_luma=False, linlog=True, C_thres=0.2, event_only=True,
                       render_kwargs={"num_steps": 512, "upsample_steps": 0})
    adam = torch.optim.Adam(model.get_params(5e-3), betas=(0.9, 0.99), eps=1e-15)
    losses = []
    torch.manual_seed(1)
    with route(on):
        for i in range(steps):
            data = _event_batch(n, 100 + i)
            adam.zero_grad(set_to_none=True)
            loss, _ = events.train_step_events(model, data, opt)
            loss.backward()
            adam.step()
            losses.append(loss.item())
    return np.array(losses)


def test_event_training_route_on_vs_off():
    from enerf_amd import stratified
    calls = stratified.stats["calls"]
    on = _train(True)
    assert stratified.stats["calls"] == calls + 40
    off = _train(False)
    assert stratified.stats["calls"] == calls + 40
    assert np.all(np.isfinite(on)) and np.all(np.isfinite(off))
    np.testing.assert_allclose(on, off, rtol=1e-4, atol=0)
