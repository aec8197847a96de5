"""The stratified route's kernels (csrc/stratified.hip) and the fp16 regime's MLP arithmetic (enerf_mlp32_precision 3,
with and without enerf_mlp32_io16) called through the C ABI on synthetic inputs, each against a float64 reference
computed on the host from the very fp32 / fp16 values the kernel was given.  No network runs in between and the PyTorch
statement is not the reference.

Shapes are chosen where these kernels carry state or pad: rays of more than one scan pass (64 lanes x 8 samples = 512
samples; T = 511, 512, 513, 1100, 2048), N not a multiple of the 4 rays per block, C = 1..3, compact lists whose length
is not a multiple of 32 with every sample masked (total == cap), and one batch of ray families: empty, saturated early,
saturated in the second / third pass only, every sample masked, weights just above and below 1e-4, rays that miss the box.

Error model of the compositing kernels (u = 2^-24, the fp32 unit roundoff; k = the sample's index on its ray):
  alpha = 1 - exp(-step s sigma): the `1 - e` rounding and e's own error make |d alpha| <= 2u + 4u alpha, ABSOLUTE (for
    alpha ~ 1e-7 that is a relative error of order 1 -- the statement rounds the same way);
  T_k = prod_{j<k} (1 - alpha_j + 1e-15): k factors, |dT_k| <= 3k u T_k from the factors near 1, plus |d alpha_j| T_j
    (<= 2u T_j) for each strongly absorbing factor (alpha_j > 1/2), whose relative error is large;
  w_k = alpha_k T_k:   |dw_k| <= 4u (T_k + 2 (k + 8) M + 4 P)   (M: the ray's max w, P: the largest T_j of an absorbing
    sample on the ray) -- the bar is relative to the ray's own scale and grows with k as the product does, linearly;
  opacity, depth: the same summed, <= 4u (S + 2 (T + 8) max(O, M) + 4 P) (S = sum of T_k over samples with alpha > 0);
    depth twice that (its clamp((z - near) / (far - near)) has two roundings of its own);
  image = sum w rgb + (1 - opacity) bg: each lane adds 8 samples per pass, then a 64-lane tree:
    <= 2u (8 npass + 10) (sum |w rgb| + |bg|);
  d sigma_k = T_k (q_k - R_{k+1}) step_k s e_k with the reverse scan R: q - R cancels, so the bar is absolute on the ray's
    scale: <= 16u (T + 16) Q G (T_k: 3k u; R: 3 (T - k) u, and 4u |q| per absorbing step),
    Q = max_k (sum_c |g_c rgb_kc| + sum_c |g_c bg_c| + |g_depth|), G = max_k step_k s e_k.
d rgb (= g w rounded once), the colour rows and the geo_feat scatter are exact.

Error model of mode 3 (fp16 operands, fp32 accumulation, h = round to half, 2^-11 relative): the kernel rounds at the
points enerf_hip.h lists -- inputs, weights, each layer's activations and activation gradients, the output (sigmoid of
the rounded output, rounded again) -- and so does the reference, from exact sums.  The kernel's sums carry fp32 error
(<= 64 terms: ~2^-18 relative), which moves a rounded value by one half-ulp where the exact sum lies that close to a
rounding boundary, and such a one-ulp step propagates through the layers behind it, times |W|.  So every value is held to
2 half-ulps of itself plus one half-ulp of its MAGNITUDE (the same sum over |operands|) per rounding stage ahead of it (a
net of L layers: L + 1 for the output, 2L + 1 for dX and the weight gradients), and most values must be
bit-identical (a systematic half-ulp slip at any rounding point would make most of them differ).  A hidden unit whose
exact pre-activation lies within fp32 error of zero may sit on the other side of the ReLU on the device: rows with one
are kept out of the row-wise checks, and each may move a weight-gradient entry by its largest single term."""
import ctypes

import numpy as np
import pytest
import torch

from nerf_mlp_ref import sh64 as _sh64

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
KPASS = 512
TH = float(np.float32(1e-4))                 # the mask threshold as the kernels and torch compare in fp32
NAN16 = 0x7E00


def _lib():
    from enerf_amd import _lib as L
    return L


def _pad32(n):
    return (n + 31) // 32 * 32


def _sentinel(shape, dtype):
    """A buffer every element of which is NaN (fp16: 0x7E00), so that any row a kernel must not touch shows up."""
    if dtype == torch.float16:
        return torch.full(shape, NAN16, dtype=torch.int16, device=DEV).view(torch.float16)
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _is_sentinel(x):
    if x.dtype == torch.float16:
        return x.contiguous().view(torch.int16) == NAN16
    return torch.isnan(x)


def _bits(x):
    return x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32)


# ============================================================================================= 1. the stratified kernels
EMPTY, SAT, SAT_LATE, ALL, EDGE, MISS, RAND = range(7)
S_DENS = 1.25                                 # density_scale (not 1: a kernel that drops it must fail)

# (N, T, C, bg_per_ray, every ray fully masked)
CASES = [
    (1, 1, 1, 0, False), (5, 1, 2, 1, False), (5, 2, 3, 0, False), (4097, 2, 2, 1, False),
    (5, 24, 1, 1, False), (4097, 24, 3, 0, False), (3, 24, 2, 1, True),
    (5, 511, 2, 0, False), (1, 512, 3, 1, False), (4097, 512, 1, 0, False),
    (5, 513, 3, 1, False), (5, 513, 1, 0, True), (4097, 513, 2, 1, False),
    (5, 1100, 1, 0, False), (4097, 1100, 3, 1, False),
    (1, 2048, 2, 1, False), (5, 2048, 3, 0, False), (1025, 2048, 1, 1, False),
]
IDS = [f"N{c[0]}-T{c[1]}-C{c[2]}-{'bgray' if c[3] else 'bgshared'}{'-allmasked' if c[4] else ''}" for c in CASES]
STORAGES = ["f32", "f16"]


def _families(N, T, allmasked):
    if allmasked:
        return np.full(N, ALL)
    return np.array([(n + T) % 7 for n in range(N)])


def _rays(fam, seed):
    """Rays from outside the box (bound 2) towards points inside it; MISS rays pass beside it."""
    g = np.random.default_rng(seed)
    N = len(fam)
    v = g.normal(size=(N, 3))
    o = 3.5 * v / np.linalg.norm(v, axis=1, keepdims=True)
    d = g.uniform(-1.5, 1.5, (N, 3)) - o
    miss = fam == MISS
    o[miss] = np.stack([np.full(miss.sum(), 3.0), g.uniform(2.5, 4.0, miss.sum()), g.uniform(-1, 1, miss.sum())], -1)
    d[miss] = np.stack([g.uniform(-0.3, 0.3, miss.sum()), np.full(miss.sum(), 0.2), np.ones(miss.sum())], -1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    f = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV).contiguous()  # noqa: E731
    return f(o), f(d)


def _alpha_to_sigma(alpha, step):
    with np.errstate(divide="ignore", invalid="ignore"):
        s = -np.log1p(-alpha) / (step * S_DENS)
    return np.where((alpha > 0) & (step > 1e-30), s, 0.0)


def _sigma(fam, z, width, seed):
    """Per-ray sigma profiles [N,T] (fp64, before rounding to fp32) from the depths the points kernel produced."""
    g = np.random.default_rng(seed)
    N, T = z.shape
    zd = z.astype(np.float64)
    step = np.concatenate([zd[:, 1:] - zd[:, :-1], width.astype(np.float64)[:, None]], 1)
    k = np.arange(T)[None, :]
    sig = np.zeros((N, T))
    for f in range(7):
        r = fam == f
        n = int(r.sum())
        if n == 0 or f == EMPTY:
            continue
        st = step[r]
        if f == SAT:                         # absorbing samples, then sigma 1e7 from a third of the way on
            ks = T // 3
            a = g.uniform(0.005, 0.03, (n, T))
            s = _alpha_to_sigma(a, st)
            s[:, ks:] = 1e7
        elif f == SAT_LATE:                  # light through the first pass, saturated in the second (or third) only
            a = g.uniform(0.0, 2e-3, (n, T))
            s = _alpha_to_sigma(a, st)
            rows = np.nonzero(r)[0]
            for i, row in enumerate(rows):
                ks = T // 2 if T <= KPASS else (1024 + 77 if T > 1100 and row % 2 else KPASS + (T - KPASS) // 3)
                s[i, min(ks, T - 1):] = 1e7
        elif f == ALL:                       # w_k = 1 / (T + 2) for every k
            a = 1.0 / (T + 2 - np.broadcast_to(k, (n, T)))
            s = _alpha_to_sigma(a, st)
        elif f == EDGE:                      # weights 1e-4 (1 + delta): well outside and inside the bar of the threshold
            delta = np.array([3e-2, -3e-2, 1e-2, -1e-2, 3e-6, -3e-6, 0.5, -0.5])
            wt = 1e-4 * (1 + delta[(k + np.arange(n)[:, None]) % 8])
            trans = 1.0 - np.concatenate([np.zeros((n, 1)), np.cumsum(wt, 1)[:, :-1]], 1)
            s = _alpha_to_sigma(wt / trans, st)
        elif f == MISS:
            s = g.uniform(0.0, 5.0, (n, T))
        else:                                # RAND: moderate absorption, a fifth of the samples empty
            a = g.uniform(0.0, min(0.3, 6.0 / T), (n, T)) * (g.uniform(size=(n, T)) > 0.2)
            s = _alpha_to_sigma(a, st)
        sig[r] = s
    return sig


_built = {}


def _case(ci):
    """Inputs of one case, the weights kernel's outputs and their fp64 reference (built once per case)."""
    if ci in _built:
        return _built[ci]
    _built.clear()                           # (one case alive at a time: the large ones hold ~100 MB of host tensors)
    L = _lib()
    lib, stream = L.lib(), L.stream_handle()
    N, T, C, per_ray, allmasked = CASES[ci]
    seed = 1000 + ci
    fam = _families(N, T, allmasked)
    ro, rd = _rays(fam, seed)
    aabb = torch.tensor([-2.0] * 3 + [2.0] * 3, device=DEV)
    f32 = dict(dtype=torch.float32, device=DEV)
    lin = float(np.float32(1) / np.float32(T - 1)) if T > 1 else 0.0
    inv_T = float(np.float32(1) / np.float32(T))
    u = torch.rand((N, T), generator=torch.Generator(device=DEV).manual_seed(seed), **f32)
    nears, fars, z, xyz = torch.empty(N, **f32), torch.empty(N, **f32), torch.empty(N, T, **f32), torch.empty(N * T, 3, **f32)
    L.check(lib.enerf_stratified_points(ro.data_ptr(), rd.data_ptr(), aabb.data_ptr(), N, T, 0.2, lin, inv_T, u.data_ptr(),
                                        nears.data_ptr(), fars.data_ptr(), z.data_ptr(), xyz.data_ptr(), stream),
            "stratified_points")
    zc, nc, fc = z.cpu(), nears.cpu(), fars.cpu()
    width = ((fc - nc) * np.float32(inv_T)).numpy()          # fp32, as the kernels form it
    miss = fam == MISS
    # the rays that miss are what the route really produces for them: near = far = FLT_MAX, every step 0
    assert np.all(nc.numpy()[miss] == np.finfo(np.float32).max) and np.all(nc.numpy()[~miss] < 10)
    sigma_c = torch.from_numpy(_sigma(fam, zc.numpy(), width, seed).astype(np.float32))
    sigma = sigma_c.to(DEV)

    w, opacity, depth = _sentinel((N, T), torch.float32), _sentinel((N,), torch.float32), _sentinel((N,), torch.float32)
    count = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    L.check(lib.enerf_stratified_weights(z.data_ptr(), sigma.data_ptr(), nears.data_ptr(), fars.data_ptr(), N, T, inv_T,
                                         S_DENS, w.data_ptr(), opacity.data_ptr(), depth.data_ptr(), count.data_ptr(),
                                         stream), "stratified_weights")
    incl = torch.cumsum(count, 0, dtype=torch.int32)

    # fp64 reference: sampler.ray_weights + the depth of render_stratified, on the fp32 z / sigma
    zd, sd = zc.double(), sigma_c.double()
    step = torch.cat([zd[:, 1:] - zd[:, :-1], torch.from_numpy(width).double()[:, None]], 1)
    e = torch.exp(-step * S_DENS * sd)
    alpha = 1 - e
    trans = torch.cumprod(torch.cat([torch.ones(N, 1, dtype=torch.float64), 1 - alpha + 1e-15], 1), 1)[:, :-1]
    w64 = alpha * trans
    t64 = ((zd - nc.double()[:, None]) / (fc.double() - nc.double())[:, None]).clamp(0, 1)
    cap = N * T
    c = dict(N=N, T=T, C=C, per_ray=per_ray, fam=fam, ro=ro, rd=rd, z=z, zc=zc, nears=nears, fars=fars, nc=nc, fc=fc,
             inv_T=inv_T, width=width, sigma=sigma, sigma_c=sigma_c, w=w, opacity=opacity, depth=depth, count=count,
             incl=incl, cap=cap, capp=_pad32(cap), step=step, e=e, alpha=alpha, trans=trans, w64=w64, t64=t64,
             wc=w.cpu(), countc=count.cpu(), total=int(incl[-1]) if N else 0)
    m = c["wc"] > TH
    c["mask"] = m
    c["s_idx"] = torch.nonzero(m.reshape(-1))[:, 0]         # compact row r -> sample, (ray, depth) order
    c["ray_of_row"] = c["s_idx"] // T
    _built[ci] = c
    return c


def _check_rows(ref, got, bar, what, rays):
    """Per-ray check: |got - ref| <= bar elementwise ([N,...] tensors), NaN where ref is NaN."""
    nan_ref = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan_ref), f"{what}: NaN positions differ on rays " \
        f"{torch.nonzero((torch.isnan(got) != nan_ref).reshape(ref.shape[0], -1).any(1))[:8, 0].tolist()}"
    err = (got - ref).abs().nan_to_num(0.0)
    bad = err > bar
    if bad.any():
        idx = torch.nonzero(bad)[:4]
        first = tuple(idx[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} values beyond the bar, e.g. at {idx.tolist()} got {got[first]:.9g} "
                             f"ref {ref[first]:.9g} bar {float(torch.as_tensor(bar).expand_as(err)[first]):.3g} "
                             f"(ray family {rays[first[0]]})")


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_weights_against_fp64(ci):
    c = _case(ci)
    N, T = c["N"], c["T"]
    w64, trans, alpha = c["w64"], c["trans"], c["alpha"]
    M = w64.amax(1, keepdim=True)
    P = (trans * (alpha > 0.5)).amax(1, keepdim=True)
    k = torch.arange(T, dtype=torch.float64)[None, :]
    bar_w = 4 * U * (trans * (alpha > 0) + 2 * (k + 8) * M + 4 * P)
    _check_rows(w64, c["wc"].double(), bar_w, "w", c["fam"])
    op64 = w64.sum(1)
    dep64 = (w64 * c["t64"]).sum(1)
    S = (trans * (alpha > 0)).sum(1)
    bar_o = 4 * U * (S + 2 * (T + 8) * torch.maximum(op64, M[:, 0]) + 4 * P[:, 0])
    _check_rows(op64, c["opacity"].cpu().double(), bar_o, "opacity", c["fam"])
    _check_rows(dep64, c["depth"].cpu().double(), 2 * bar_o, "depth", c["fam"])
    # the mask counts: exactly the kernel's own w > 1e-4, and the fp64 mask except within the bar of the threshold
    count = c["countc"]
    assert torch.equal(count, c["mask"].sum(1).to(torch.int32))
    flip = (c["mask"] != (w64 > TH)) & ((w64 - TH).abs() > bar_w)
    assert not flip.any(), f"{int(flip.sum())} samples masked against the fp64 weights, e.g. " \
                           f"{torch.nonzero(flip)[:4].tolist()}"
    # the families are what they are meant to be
    fam = torch.from_numpy(c["fam"])
    assert (count[(fam == EMPTY) | (fam == MISS)] == 0).all()
    assert (count[fam == ALL] == T).all()
    if T > KPASS:
        late = fam == SAT_LATE
        assert (w64[late][:, :KPASS].sum(1) < 0.9).all() and (w64[late].sum(1) > 1 - 1e-6).all()
    if (fam == EDGE).any() and T >= 8:
        assert ((count[fam == EDGE] > 0) & (count[fam == EDGE] < T)).all()


def _rgb(c, storage, seed):
    dt = torch.float16 if storage == "f16" else torch.float32
    g = torch.Generator(device=DEV).manual_seed(seed)
    rgb = torch.rand(c["capp"], c["C"], generator=g, device=DEV).to(dt)
    return rgb


def _bg(c, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand((c["N"], c["C"]) if c["per_ray"] else (c["C"],), generator=g, device=DEV)


def _storage(storage):
    L = _lib()
    return (L.F16, torch.float16) if storage == "f16" else (L.F32, torch.float32)


def _check_pad(buf, total, cap, what):
    """Rows total .. min(pad32(total), cap) zero, every row beyond them untouched."""
    end = min(_pad32(total), cap)
    pad = buf[total:end]
    assert not _is_sentinel(pad).any(), f"{what}: pad rows {total}..{end} not written"
    assert (pad.float() == 0).all(), f"{what}: pad rows {total}..{end} not zero"
    assert _is_sentinel(buf[end:]).all(), f"{what}: rows from {end} on written"


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_color_input_rows(ci, storage):
    from enerf_amd import shencoder
    L = _lib()
    c = _case(ci)
    N, T, total, cap = c["N"], c["T"], c["total"], c["cap"]
    store, dt = _storage(storage)
    g = torch.Generator(device=DEV).manual_seed(ci)
    h16 = (torch.rand(N * T, 16, generator=g, device=DEV) * 4 - 2).contiguous()
    cin = _sentinel((c["capp"], 32), dt)
    L.check(L.lib().enerf_stratified_color_input_ex(c["w"].data_ptr(), c["incl"].data_ptr(), c["count"].data_ptr(),
                                                    h16.data_ptr(), c["rd"].data_ptr(), N, T, cap, cin.data_ptr(), store,
                                                    L.stream_handle()), "stratified_color_input")
    s_idx, ray = c["s_idx"].to(DEV), c["ray_of_row"].to(DEV)
    rows = cin[:total]
    assert (rows[:, 0].float() == 0).all() and not _is_sentinel(rows[:, 0]).any()
    assert torch.equal(_bits(rows[:, 1:16]), _bits(h16[s_idx][:, 1:16].to(dt)))
    # SH4 columns: bit for bit the library's own encoder (F16: its half form on the half-rounded directions) ...
    d_in = c["rd"].half() if storage == "f16" else c["rd"]
    sh = shencoder.sh_encode(d_in, 4)
    assert sh.dtype == dt
    assert torch.equal(_bits(rows[:, 16:32]), _bits(sh[ray]))
    # ... and within a few ulp of the basis in fp64 (F16: one half-ulp of rounding on top), relative to the row's scale
    ref = _sh64(d_in.double().cpu())[ray.cpu()]
    got = rows[:, 16:32].double().cpu()
    scale = ref.abs().amax(1, keepdim=True)
    bar = 16 * U * scale + (2.0 ** -11 * ref.abs() if storage == "f16" else 0)
    assert ((got - ref).abs() <= bar).all(), float(((got - ref).abs() / scale).max())
    _check_pad(cin, total, cap, "color_input")


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_composite_forward(ci, storage):
    L = _lib()
    c = _case(ci)
    N, T, C = c["N"], c["T"], c["C"]
    store, dt = _storage(storage)
    rgb, bg = _rgb(c, storage, 7 + ci), _bg(c, 8 + ci)
    image = _sentinel((N, C), torch.float32)
    L.check(L.lib().enerf_stratified_composite_forward_ex(c["w"].data_ptr(), c["incl"].data_ptr(), c["count"].data_ptr(),
                                                          c["opacity"].data_ptr(), rgb.data_ptr(), bg.data_ptr(),
                                                          c["per_ray"], N, T, C, image.data_ptr(), store,
                                                          L.stream_handle()), "stratified_composite_forward")
    wm = c["wc"].double()[c["mask"]]
    ray = c["ray_of_row"]
    contrib = wm[:, None] * rgb[:c["total"]].double().cpu()
    acc = torch.zeros(N, C, dtype=torch.float64).index_add_(0, ray, contrib)
    acc_abs = torch.zeros(N, C, dtype=torch.float64).index_add_(0, ray, contrib.abs())
    bgd = bg.double().cpu().expand(N, C)
    ref = acc + (1 - c["opacity"].cpu().double())[:, None] * bgd
    npass = (T + KPASS - 1) // KPASS
    bar = 2 * U * (8 * npass + 10) * (acc_abs + bgd.abs()).amax(1, keepdim=True)
    _check_rows(ref, image.cpu().double(), bar, "image", c["fam"])


@pytest.mark.parametrize("with_depth", [True, False], ids=["g_depth", "no_depth"])
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_composite_backward(ci, storage, with_depth):
    L = _lib()
    c = _case(ci)
    N, T, C, total, cap = c["N"], c["T"], c["C"], c["total"], c["cap"]
    store, dt = _storage(storage)
    rgb, bg = _rgb(c, storage, 17 + ci), _bg(c, 18 + ci)
    g = torch.Generator(device=DEV).manual_seed(19 + ci)
    g_image = torch.randn(N, C, generator=g, device=DEV)
    g_depth = torch.randn(N, generator=g, device=DEV) if with_depth else None
    g_sigma = _sentinel((N * T,), torch.float32)
    g_rgb = _sentinel((c["capp"], C), dt)
    L.check(L.lib().enerf_stratified_composite_backward_ex(
        g_image.data_ptr(), g_depth.data_ptr() if with_depth else None, c["z"].data_ptr(), c["sigma"].data_ptr(),
        c["w"].data_ptr(), c["nears"].data_ptr(), c["fars"].data_ptr(), c["incl"].data_ptr(), c["count"].data_ptr(),
        rgb.data_ptr(), bg.data_ptr(), c["per_ray"], N, T, C, c["inv_T"], S_DENS, cap, g_sigma.data_ptr(),
        g_rgb.data_ptr(), store, L.stream_handle()), "stratified_composite_backward")

    # fp64 autograd of the compositing, sigma the leaf, over the kernel's own mask
    mask = c["mask"]
    sig = c["sigma_c"].double().requires_grad_(True)
    alpha = 1 - torch.exp(-c["step"] * S_DENS * sig)
    trans = torch.cumprod(torch.cat([torch.ones(N, 1, dtype=torch.float64), 1 - alpha + 1e-15], 1), 1)[:, :-1]
    w = alpha * trans
    rgb_s = torch.zeros(N, T, C, dtype=torch.float64)
    rgb_s[mask] = rgb[:total].double().cpu()
    bgd = bg.double().cpu().expand(N, C)
    gi = g_image.double().cpu()
    image = (w[..., None] * rgb_s).sum(1) + (1 - w.sum(1))[:, None] * bgd
    loss = (gi * image).sum()
    if with_depth:
        gd = g_depth.double().cpu()
        loss = loss + (gd * (w * c["t64"]).sum(1)).sum()
    loss.backward()
    ref = sig.grad
    got = g_sigma.cpu().double().view(N, T)
    if not with_depth:                      # (rays that miss the box have t = NaN: without a depth term no NaN at all)
        assert torch.isfinite(got).all(), "g_sigma not finite without a depth gradient"
    q = (gi[:, None, :] * rgb_s).abs().sum(-1) + (gi * bgd).abs().sum(-1, keepdim=True)
    if with_depth:
        q = q + gd.abs()[:, None]
    Q = q.amax(1, keepdim=True)
    G = (c["step"] * S_DENS * c["e"]).amax(1, keepdim=True)
    bar = 16 * U * (T + 16) * Q * G
    _check_rows(ref, got, bar, "g_sigma", c["fam"])
    # d rgb of every compact row: g * w rounded once (F16: the fp32 product rounded to half, the gradient of h.to(fp32))
    # (caught the F16 kernel rounding the exact product to half in one step, v_fma_mixlo_f16: wrong at fp16 ties)
    wm = c["wc"][mask]
    prod = g_image.cpu()[c["ray_of_row"]] * wm[:, None]
    exp_rgb = prod.to(dt)
    got_rgb = g_rgb[:total].cpu()
    bad = _bits(got_rgb) != _bits(exp_rgb)
    assert not bad.any(), f"g_rgb: {int(bad.sum())} values differ, e.g. at {torch.nonzero(bad)[:4].tolist()}: " \
                          f"{got_rgb[bad][:4].tolist()} vs {exp_rgb[bad][:4].tolist()} (g * w in fp32: {prod[bad][:4].tolist()})"
    _check_pad(g_rgb, total, cap, "g_rgb")


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_scatter_geo_grad(ci, storage):
    L = _lib()
    c = _case(ci)
    N, T = c["N"], c["T"]
    store, dt = _storage(storage)
    g = torch.Generator(device=DEV).manual_seed(29 + ci)
    dx = torch.randn(c["capp"], 32, generator=g, device=DEV).to(dt)
    dh16 = _sentinel((N * T, 16), torch.float32)
    L.check(L.lib().enerf_stratified_scatter_geo_grad_ex(c["w"].data_ptr(), c["incl"].data_ptr(), c["count"].data_ptr(),
                                                         dx.data_ptr(), N, T, dh16.data_ptr(), store, L.stream_handle()),
            "stratified_scatter_geo_grad")
    exp = torch.zeros(N * T, 16, dtype=torch.float32)
    exp[c["s_idx"]] = dx[:c["total"], :16].float().cpu()       # column 0 too: the sigma net's backward replaces it
    assert torch.equal(_bits(dh16.cpu()), _bits(exp))


# ============================================================================================= 2. mode 3 MLP arithmetic
def _h(x):
    return x.half().double()


def _segs(tensors):
    return (ctypes.c_void_p * 4)(*[t.data_ptr() if t is not None else None for t in tensors])


class _Mode3:
    def __init__(self, io16):
        self.io16 = io16

    def __enter__(self):
        lib = _lib().lib()
        self.prev = lib.enerf_mlp32_precision(3)
        if self.io16:
            lib.enerf_mlp32_io16(1)
        return lib

    def __exit__(self, *exc):
        lib = _lib().lib()
        lib.enerf_mlp32_io16(0)
        lib.enerf_mlp32_valid_rows(None)
        lib.enerf_mlp32_precision(self.prev)
        return False


def _ulp_h(x):
    """one half-precision ulp of |x| (fp16 subnormal spacing below 2^-14)"""
    a = x.abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


def _w0_eff(w0, perm):
    """The first layer as the kernels apply it to their input rows (nerf_perm: [0 | geo 15 | SH 16] rows against memory
    columns [SH 16 | geo 15])."""
    if not perm:
        return w0
    z = torch.zeros(w0.shape[0], 1, dtype=w0.dtype)
    return torch.cat([z, w0[:, 16:31], w0[:, 0:16]], 1)


def _w0_grad_back(g_eff, perm):
    return torch.cat([g_eff[:, 16:32], g_eff[:, 1:16]], 1) if perm else g_eff


def _ref_forward(x, ws, perm):
    """mode 3 in fp64: x, weights and each layer's activations rounded to half; -> (pre-activations, rounded acts, out)"""
    hw = [_h(w) for w in ws]
    hw[0] = _w0_eff(hw[0], perm)
    acts, pres = [_h(x)], []
    for w in hw[:-1]:
        p = acts[-1] @ w.t()
        pres.append(p)
        acts.append(_h(torch.relu(p)))
    o = acts[-1] @ hw[-1].t()
    # magnitudes: the same sums over |operands|
    mags = [acts[i].abs() @ hw[i].abs().t() for i in range(len(hw))]
    return hw, pres, acts, o, mags


def _ref_backward(dy_eff, hw, pres, acts, perm):
    """gradients from the output-layer gradient (already in fp32 as the kernel forms it): each layer's activation gradient
    rounded to half, exact sums -> (dX, [dW], magnitude of dX, [magnitude of dW], max single term of each dW)"""
    g = _h(dy_eff)
    ga = g.abs()
    dws, dwm, dwt = [None] * len(hw), [None] * len(hw), [None] * len(hw)
    for li in range(len(hw) - 1, -1, -1):
        a = acts[li]
        dws[li] = g.t() @ a
        dwm[li] = ga.t() @ a.abs()
        dwt[li] = torch.zeros_like(dws[li])
        for c0 in range(0, a.shape[0], 1024):
            dwt[li] = torch.maximum(dwt[li], (ga[c0:c0 + 1024, :, None] * a[c0:c0 + 1024, None, :].abs()).amax(0))
        if li == 0:
            dx = g @ hw[0]
            dxm = ga @ hw[0].abs()
            break
        gp = (g @ hw[li]) * (pres[li - 1] > 0)
        gpm = (ga @ hw[li].abs()) * (pres[li - 1] > 0)
        g, ga = _h(gp), gpm
    dws[0] = _w0_grad_back(dws[0], perm)
    dwm[0] = _w0_grad_back(dwm[0], perm)
    dwt[0] = _w0_grad_back(dwt[0], perm)
    return dx, dws, dxm, dwm, dwt


def _kinks(pres, acts, hw):
    """rows with a hidden pre-activation within fp32 accumulation error of zero"""
    k = torch.zeros(pres[0].shape[0], dtype=torch.bool)
    for li, p in enumerate(pres):
        m = acts[li].abs() @ hw[li].abs().t()
        k |= ((p.abs() <= 64 * U * m) & (m > 0)).any(1)
    return k


def _close16(got, ref, mag, stages, what, min_exact):
    """|got - ref| <= 2 half-ulps of ref + one half-ulp of the magnitude per rounding stage ahead of it; at least
    `min_exact` of them bit-identical"""
    err = (got - ref).abs()
    bar = 2 * _ulp_h(ref) + stages * 2.0 ** -11 * mag
    assert torch.isfinite(got).all(), f"{what}: not finite"
    assert (err <= bar).all(), f"{what}: {int((err > bar).sum())} beyond the bar, worst {float((err / bar).max()):.2f}"
    if got.numel():
        exact = float((got.half() == ref.half()).double().mean())
        assert exact >= min_exact, f"{what}: only {exact:.4f} bit-identical"


# (num_hidden, out_dim, nerf_perm, B, valid rows (None: every row))
IO16_CASES = [
    (2, 3, 1, 4097, None), (2, 3, 1, 4097, 33), (2, 3, 1, 4097, 1), (2, 1, 1, 33, 32), (2, 2, 0, 31, 1),
    (2, 16, 0, 4097, 0), (2, 16, 1, 1, 1), (2, 2, 1, 33, 31), (3, 3, 1, 33, 31), (3, 1, 0, 4097, 4097),
    (3, 2, 1, 31, None), (3, 16, 0, 33, 33), (3, 3, 0, 4097, 32), (3, 16, 1, 4097, None),
]


@pytest.mark.parametrize("nh,out_dim,perm,B,valid", IO16_CASES,
                         ids=[f"nh{a}-out{b}-perm{c}-B{d}-valid{e}" for a, b, c, d, e in IO16_CASES])
def test_mlp32_io16_colour_net(nh, out_dim, perm, B, valid):
    """enerf_mlp32_io16 forward (sigmoid output at a wider row stride) and backward (sigmoid backward from that strided
    output, strided dY) against fp64 with mode 3's rounding points; rows past the valid tiles untouched by the forward,
    zero dX in the backward, and counted by no weight gradient."""
    L = _lib()
    stream = L.stream_handle()
    g = torch.Generator().manual_seed(nh * 1000 + out_dim * 100 + B + (valid or 0))
    w0c = 31 if perm else 32
    ws = [(torch.rand(64, w0c, generator=g) * 2 - 1) * 0.35]
    ws += [(torch.rand(64, 64, generator=g) * 2 - 1) * 0.25 for _ in range(nh - 1)]
    ws += [(torch.rand(out_dim, 64, generator=g) * 2 - 1) * 0.4]
    x = (torch.rand(B, 32, generator=g) * 2 - 1).half()
    if perm:
        x[:, 0] = 0                                            # (the route's rows: column 0 is the zero column)
    ys = out_dim + 3                                           # every stride wider than a row
    dys, yss = out_dim + 5, ys
    wd = [w.to(DEV).contiguous() for w in ws]
    seg = _segs(wd[:1] + wd[1:nh] + [None] * (3 - nh) + wd[-1:])
    xd = x.to(DEV)
    Y = _sentinel((B, ys), torch.float16)
    dY = _sentinel((B, dys), torch.float16)
    dY[:, :out_dim] = torch.randn(B, out_dim, generator=g).half().to(DEV)
    dX = _sentinel((B, 32), torch.float16)
    dw = [_sentinel(tuple(w.shape), torch.float32) for w in ws]
    dseg = _segs(dw[:1] + dw[1:nh] + [None] * (3 - nh) + dw[-1:])
    cnt = torch.tensor([valid if valid is not None else 0], dtype=torch.int32, device=DEV)
    with _Mode3(True) as lib:
        lib.enerf_mlp32_valid_rows(cnt.data_ptr() if valid is not None else None)
        L.check(lib.enerf_mlp32_forward_p(xd.data_ptr(), seg, w0c, perm, B, 32, out_dim, nh, 0, 3, None, Y.data_ptr(), 0,
                                          ys, None, None, stream), "mlp32_forward_p io16")
        bb = torch.empty(1, device=DEV)
        L.check(lib.enerf_mlp32_backward_p(dY.data_ptr(), xd.data_ptr(), seg, dseg, w0c, perm, 1, None, B, 32, out_dim, nh,
                                           0, bb.data_ptr(), dX.data_ptr(), 0, dys, Y.data_ptr(), yss, None, None, 0,
                                           stream), "mlp32_backward_p io16")
    rows = B if valid is None else min(valid, B)
    R = min(_pad32(rows), B)                                   # the valid tiles' rows: real rows for the kernels
    Yc, dXc = Y.cpu(), dX.cpu()
    # forward
    hw, pres, acts, o, mags = _ref_forward(x[:R].double(), ws, perm)
    y_ref = _h(torch.sigmoid(_h(o)))
    ymag = 0.25 * mags[-1] + _ulp_h(o)                          # (sigmoid' <= 1/4)
    nl = len(ws)
    _close16(Yc[:R, :out_dim].double(), y_ref, ymag, nl + 1, "Y", 0.9)
    assert _is_sentinel(Yc[:R, out_dim:]).all(), "Y: columns past out_dim written"
    assert _is_sentinel(Yc[R:]).all(), "Y: rows past the valid tiles written"
    # backward: the sigmoid backward in fp32 as the kernel forms it, from the forward's 16-bit output
    ysig = Yc[:R, :out_dim].float()
    dy_eff = ((dY.cpu()[:R, :out_dim].float() * (1.0 - ysig)) * ysig).double()
    dx_ref, dw_ref, dxm, dwm, dwt = _ref_backward(dy_eff, hw, pres, acts, perm)
    kink = _kinks(pres, acts, hw)
    ok = ~kink
    _close16(dXc[:R][ok].double(), dx_ref[ok], dxm[ok], 2 * nl + 1, "dX", 0.8)
    assert (dXc[R:].float() == 0).all() and not _is_sentinel(dXc[R:]).any(), "dX of padding tiles not zero"
    n_k = int(kink.sum())
    for li, (a, r) in enumerate(zip(dw, dw_ref)):
        got = a.cpu().double()
        bar = (2 * nl + 1) * 2.0 ** -11 * dwm[li] + n_k * dwt[li] + 1e-30
        err = (got - r).abs()
        assert torch.isfinite(got).all() and (err <= bar).all(), \
            f"dW[{li}]: worst {float((err / bar).max()):.2f} (kinks {n_k})"


@pytest.mark.parametrize("B", [4097, 33])
def test_mlp32_mode3_sigma_net(B):
    """The fp16 regime's sigma net: mode 3 with fp32 I/O, level-major input, one hidden layer, the output rounded to half
    and exp(h0) in fp32 (y0_exp); the backward with the trunc_exp gradient of column 0, dsigma * exp(clamp(h0, -15, 15)),
    evaluated in fp32 and rounded to half with the other 15 columns."""
    L = _lib()
    stream = L.stream_handle()
    Bp = _pad32(B)
    g = torch.Generator().manual_seed(B)
    ws = [(torch.rand(64, 32, generator=g) * 2 - 1) * 0.5, (torch.rand(16, 64, generator=g) * 2 - 1) * 0.3]
    ws[1][0] *= 12.0                                            # h0 past +-15 on some rows: the clamp is reached
    x = torch.rand(B, 32, generator=g) * 2 - 1
    xl = torch.zeros(16, Bp, 2)
    xl[:, :B] = x.view(B, 16, 2).permute(1, 0, 2)
    wd = [w.to(DEV).contiguous() for w in ws]
    seg = _segs([wd[0], None, None, wd[1]])
    xd = xl.to(DEV).contiguous()
    Y = _sentinel((B, 16), torch.float32)
    y0 = _sentinel((B,), torch.float32)
    fb = torch.empty(1, Bp, 64, device=DEV)
    dY = torch.randn(B, 16, generator=g).to(DEV)
    dsig = ((torch.rand(B, generator=g) * 2 - 1) * 1e-3).to(DEV)
    dX = _sentinel((16, Bp, 2), torch.float32)
    dw = [_sentinel(tuple(w.shape), torch.float32) for w in ws]
    dseg = _segs([dw[0], None, None, dw[1]])
    bb = torch.empty(1, Bp, 64, device=DEV)
    with _Mode3(False) as lib:
        L.check(lib.enerf_mlp32_forward_p(xd.data_ptr(), seg, 32, 0, B, 32, 16, 1, 0, 6, fb.data_ptr(), Y.data_ptr(), 1,
                                          16, y0.data_ptr(), None, stream), "mlp32_forward_p sigma")
        L.check(lib.enerf_mlp32_backward_p(dY.data_ptr(), xd.data_ptr(), seg, dseg, 32, 0, 1, fb.data_ptr(), B, 32, 16, 1,
                                           0, bb.data_ptr(), dX.data_ptr(), 1, 16, None, 0, dsig.data_ptr(), Y.data_ptr(),
                                           16, stream), "mlp32_backward_p sigma")
    Yc, y0c = Y.cpu(), y0.cpu()
    hw, pres, acts, o, mags = _ref_forward(x.double(), ws, False)
    _close16(Yc.double(), _h(o), mags[-1], 3, "Y", 0.95)
    assert torch.equal(Yc, Yc.half().float()), "Y not fp16 values"
    assert float(Yc[:, 0].abs().max()) > 15.0
    # sigma = exp(h0) of the kernel's own rounded h0, in fp32: a few fp32 ulp
    e64 = torch.exp(Yc[:, 0].double())
    assert ((y0c.double() - e64).abs() <= 4 * U * e64).all()
    # backward: column 0's gradient in fp32 from the kernel's h0 (its forward output), the rest dY as given
    dy_eff = dY.cpu().clone()
    dy_eff[:, 0] = dsig.cpu() * torch.exp(torch.clamp(Yc[:, 0], -15.0, 15.0))
    dx_ref, dw_ref, dxm, dwm, dwt = _ref_backward(dy_eff.double(), hw, pres, acts, False)
    kink = _kinks(pres, acts, hw)
    ok = ~kink
    dxr = dX.cpu()[:, :B].permute(1, 0, 2).reshape(B, 32).double()
    _close16(dxr[ok], dx_ref[ok], dxm[ok], 5, "dX", 0.0)           # (fp32 output: no rounding to half to match bits)
    assert (dX.cpu()[:, B:] == 0).all(), "dX pad rows not zero"
    n_k = int(kink.sum())
    for li, (a, r) in enumerate(zip(dw, dw_ref)):
        got = a.cpu().double()
        bar = 5 * 2.0 ** -11 * dwm[li] + n_k * dwt[li] + 1e-30
        err = (got - r).abs()
        assert torch.isfinite(got).all() and (err <= bar).all(), f"dW[{li}]: worst {float((err / bar).max()):.2f}"
