"""The fully fused MLP kernels (csrc/ffmlp.hip: k_ffmlp_fwd, k_ffmlp_bwd_act; csrc/ffmlp_wgrad.hip: k_ffmlp_bwd_w,
k_ffmlp_reduce_w), the recomputing entry points (enerf_mlp32::ffmlp16_forward / ffmlp16_backward) and the fused network_ff
inference kernel (csrc/ffnerf.hip: k_ffnerf_infer) against the fp64 reference, the a-priori bars and the exact nets of
tests/ffmlp_ref.py (the model is derived in that module's docstring; tests/test_ffmlp_ref.py holds the C oracle to the same
bars and shows that they reject thirteen seeded defects).

  a. buffered kernels, layer by layer, random values: every entry of every buffer inside the interval rule's interval,
     computed from the kernels' own previous layer -- no quantile, no entry left out;
  b. every route on exact nets, bit for bit;
  c. the persistent loops past their grid caps (a second trip), exact nets, bit for bit;
  d. the routes without intermediate buffers end to end on random values: inside the propagated intervals, whose widths
     are printed and held to the conditions of tests/test_ffmlp_ref.py;
  e. refusals: a non-zero code and nothing written.
Every output buffer starts as NaN and every buffer carries canary rows past its end, which must come back untouched.
139 cases in 16 - 18 s on one MI355X (half of it the four cases at 131 k rows with their fp64 references)."""
import functools

import numpy as np
import pytest
import torch

import ffmlp_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
TORCH16 = {"bf16": torch.bfloat16, "fp16": torch.float16}
CAN = 64                # canary rows past the end of every buffer
SENT = -777.0           # their value (a bf16 and an fp16 number)
NAN = float("nan")
WRAP_B = 131072 + 384
WIDTH_WSCALE = 0.15     # as in tests/test_ffmlp_ref.py


def _ff():
    from enerf_amd.backends import _ffmlp
    return _ffmlp


def _lib():
    from enerf_amd import _lib as L
    return L


class Buf:
    """[rows, cols] of `dtype` with CAN canary rows behind it"""

    def __init__(self, rows, cols, dtype, data=None, lead=()):
        n = int(np.prod(lead, dtype=np.int64)) * rows * cols
        self.full = torch.full((n + CAN * cols,), SENT, dtype=dtype, device=DEV)
        self.n = n
        self.t = self.full[:n].view(*lead, rows, cols)
        if data is None:
            self.t.fill_(NAN)
        else:
            self.t.copy_(torch.as_tensor(np.asarray(data, np.float64)).to(dtype).view(*lead, rows, cols))

    def np(self):
        if self.t.dtype == torch.float32:
            return self.t.double().cpu().numpy()
        bits = self.t.view(torch.int16).cpu().numpy().astype(np.uint16)           # decoded on the host, denormals included
        if self.t.dtype == torch.float16:
            return bits.view(np.float16).astype(np.float64)
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)

    def canary_ok(self):
        return bool((self.full[self.n:] == SENT).all())

    def untouched(self):
        return bool(torch.isnan(self.t).all()) and self.canary_ok()


def _canaries(**bufs):
    bad = [k for k, b in bufs.items() if not b.canary_ok()]
    assert not bad, f"canary rows written: {bad}"


def _finish(W, title):
    print(W.report(title))
    assert not W.fails, "\n".join(W.fails)


def _same_bits(W, name, got, want, dtype):
    """bit for bit (NaN == NaN, -0 == 0), compared on the device; the message comes from the host comparator"""
    w = torch.as_tensor(np.asarray(want, np.float64)).to(dtype).to(DEV).view(got.shape)
    if torch.equal(got, w) or bool(((got == w) | (torch.isnan(got) & torch.isnan(w))).all()):
        W.ratio[name] = max(W.ratio.get(name, 0.0), 0.0)
        return
    W.exact(name, got.double().cpu().numpy(), np.asarray(want, np.float64).reshape(tuple(got.shape)))


@pytest.fixture
def buffered():
    prev = _lib().lib().enerf_ffmlp_recompute(0)
    yield
    _lib().lib().enerf_ffmlp_recompute(prev)


@functools.lru_cache(maxsize=None)
def _random(in_dim, NL, B, kind, wscale, mean=0.0):
    rng = np.random.default_rng(1000 * in_dim + 10 * NL + B)
    W = R.r16((rng.uniform(-1, 1, R.blob_size(in_dim, NL)) + mean) * wscale, kind)
    return W, R.r16(rng.uniform(-1, 1, (B, in_dim)), kind), R.r16(rng.uniform(-1, 1, (B, 16)), kind)


@functools.lru_cache(maxsize=None)
def _net(NL, in_dim, B, dy_scale=1.0):
    return R.exact_net(NL, in_dim, B, 5, dy_scale=dy_scale)


def _forward(x, W, B, in_dim, NL, act, out_act, dtype, inference=False):
    fb = Buf(B, 64, dtype, lead=(NL,))
    y = Buf(B, 16, dtype)
    f = _ff().ffmlp_inference if inference else _ff().ffmlp_forward
    f(x.t, W.t, B, in_dim, 16, 64, NL, act, out_act, fb.t if not inference else fb.t[0], y.t)
    return fb, y


def _backward(dy, x, W, fb, B, in_dim, NL, act, dtype, want_dx=True, gw_old=None):
    bb = Buf(B, 64, dtype, lead=(NL,))
    dx = Buf(B, in_dim, dtype)
    gw = Buf(1, W.n, dtype, data=np.zeros(W.n) if gw_old is None else gw_old)
    _ff().ffmlp_backward(dy.t, x.t, W.t, fb.t, B, in_dim, 16, 64, NL, act, 6, want_dx, bb.t, dx.t, gw.t.view(-1))
    return bb, dx, gw


# ---------------------------------------------------------------------------- a. buffered kernels, layer-wise, random values
def _plant_special_values(fb, seed):
    """exact zeros, the smallest positive 16-bit value and negative zero among the entries of a forward_buffer"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    bits = fb.t.view(torch.int16).view(-1)
    idx = torch.randperm(bits.numel(), generator=g)[: 3 * max(bits.numel() // 50, 3)].to(DEV)
    k = idx.numel() // 3
    bits[idx[:k]] = 0
    bits[idx[k:2 * k]] = 1
    bits[idx[2 * k:]] = -32768


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("B", [128, 384, 6272 + 128])
@pytest.mark.parametrize("NL", [2, 3, 4])
@pytest.mark.parametrize("in_dim", [16, 32, 64])
def test_buffered_kernels_layer_by_layer(in_dim, NL, B, kind, buffered):
    dtype = TORCH16[kind]
    Wn, xn, dyn = _random(in_dim, NL, B, kind, float(np.sqrt(3 / 64) * 1.5))
    W, x, dy = Buf(1, Wn.size, dtype, Wn), Buf(B, in_dim, dtype, xn), Buf(B, 16, dtype, dyn)
    Wo = R.Worst()
    fb, y = _forward(x, W, B, in_dim, NL, 0, 6, dtype)
    R.check_forward_layers(Wo, xn, Wn, in_dim, NL, 0, 6, kind, fb.np(), y.np())
    fbi, yi = _forward(x, W, B, in_dim, NL, 0, 6, dtype, inference=True)
    assert torch.equal(yi.t, y.t) and fbi.untouched()
    # the backward on a forward_buffer of the test's own
    _plant_special_values(fb, B + NL)
    fbn = fb.np()
    assert np.signbit(fbn[fbn == 0]).any() and not np.signbit(fbn[fbn == 0]).all()
    assert np.abs(fbn[fbn != 0]).min() == (2.0 ** -133 if kind == "bf16" else 2.0 ** -24)
    K_w = R.wgrad_chain(B)
    old = R.r16(np.random.default_rng(B).uniform(-1, 1, Wn.size), kind)
    for gw_old in (None, old):
        bb, dx, gw = _backward(dy, x, W, fb, B, in_dim, NL, 0, dtype, gw_old=gw_old)
        R.check_backward_layers(Wo, dyn, xn, Wn, fbn, in_dim, NL, 0, kind, bb.np(), dx.np(), gw.np(), K_w, gw_old=gw_old,
                                tag="" if gw_old is None else "prefilled ")
        _canaries(bb=bb, dx=dx, gw=gw)
    bb2, dx2, gw2 = _backward(dy, x, W, fb, B, in_dim, NL, 0, dtype, want_dx=False)
    assert dx2.untouched() and torch.equal(bb2.t, bb.t)
    R.check_backward_layers(Wo, dyn, xn, Wn, fbn, in_dim, NL, 0, kind, bb2.np(), None, gw2.np(), K_w, tag="no dX ")
    _canaries(W=W, x=x, dy=dy, fb=fb, y=y, yi=yi, bb2=bb2, gw2=gw2)
    _finish(Wo, f"layer-wise in={in_dim} NL={NL} B={B} {kind} (K_w={K_w})")


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("act", [1, 3, 4, 5])
def test_buffered_kernels_other_activations(act, kind, buffered):
    in_dim, NL, B, dtype = 32, 2, 128, TORCH16[kind]
    Wn, xn, dyn = _random(in_dim, NL, B, kind, 0.02 if act == 1 else 0.1)
    W, x, dy = Buf(1, Wn.size, dtype, Wn), Buf(B, in_dim, dtype, xn), Buf(B, 16, dtype, dyn)
    fb, y = _forward(x, W, B, in_dim, NL, act, 6, dtype)
    fbn = fb.np()
    m = R.split(Wn, in_dim, NL)
    assert max(np.abs(xn @ m[0].T).max(), np.abs(fbn[0] @ m[1].T).max()) <= 4          # |pre-activation| <= 4
    Wo = R.Worst()
    R.check_forward_layers(Wo, xn, Wn, in_dim, NL, act, 6, kind, fbn, y.np())
    bb, dx, gw = _backward(dy, x, W, fb, B, in_dim, NL, act, dtype)
    R.check_backward_layers(Wo, dyn, xn, Wn, fbn, in_dim, NL, act, kind, bb.np(), dx.np(), gw.np(), R.wgrad_chain(B))
    _canaries(fb=fb, y=y, bb=bb, dx=dx, gw=gw)
    _finish(Wo, f"activation {act} {kind}")


# -------------------------------------------------------------------------------------- b. every route, exact nets, bit for bit
def _exact_route(n, kind, recompute, want_dx, gw_old=None):
    """one forward + backward of an exact net on one route; -> Worst"""
    dtype, NL, in_dim, B = TORCH16[kind], n["NL"], n["in_dim"], n["B"]
    L = _lib().lib()
    prev = L.enerf_ffmlp_recompute(1 if recompute else 0)
    try:
        W, x, dy = Buf(1, n["W"].size, dtype, n["W"]), Buf(B, in_dim, dtype, n["x"]), Buf(B, 16, dtype, n["dy"])
        Wo = R.Worst()
        fb, y = _forward(x, W, B, in_dim, NL, 0, 6, dtype)
        _same_bits(Wo, "y", y.t, n["y"], dtype)
        if recompute:
            assert fb.untouched()
            fb_in = Buf(B, 64, dtype, lead=(NL,))
        else:
            _same_bits(Wo, "fb", fb.t, n["fb"], dtype)
            fb_in = fb
        bb, dx, gw = _backward(dy, x, W, fb_in, B, in_dim, NL, 0, dtype, want_dx=want_dx, gw_old=gw_old)
        if recompute:
            assert bb.untouched() and fb_in.untouched()
        else:
            _same_bits(Wo, "bb", bb.t, n["bb"], dtype)
        if want_dx:
            _same_bits(Wo, "dX", dx.t, n["dx"], dtype)
        else:
            assert dx.untouched()
        _same_bits(Wo, "dW", gw.t.view(-1), R.exact_gw(n, kind, gw_old), dtype)
        _canaries(W=W, x=x, dy=dy, fb=fb, y=y, bb=bb, dx=dx, gw=gw)
        return Wo
    finally:
        L.enerf_ffmlp_recompute(prev)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("want_dx", [True, False])
@pytest.mark.parametrize("recompute", [False, True], ids=["buffered", "recompute"])
@pytest.mark.parametrize("NL", [2, 3])
def test_exact_nets_every_route(NL, recompute, want_dx, kind):
    n = _net(NL, 32, 384)
    _finish(_exact_route(n, kind, recompute, want_dx), f"exact NL={NL} {'recompute' if recompute else 'buffered'} dX={want_dx} {kind}")


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("NL,in_dim,B", [(4, 64, 384), (2, 16, 384), (2, 32, 6400)])
def test_exact_nets_buffered_other_shapes_and_prefilled_grad_weights(NL, in_dim, B, kind):
    n = _net(NL, in_dim, B)
    old = np.random.default_rng(3).integers(-3, 4, n["sums"].size).astype(np.float64)
    _finish(_exact_route(n, kind, False, True, gw_old=old), f"exact buffered in={in_dim} NL={NL} B={B} prefilled {kind}")


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("B", [1, 127, 129])
@pytest.mark.parametrize("NL", [2, 3])
def test_exact_nets_through_the_module(monkeypatch, NL, B, kind):
    """enerf_amd.ffmlp.FFMLP pads B to a multiple of 128 and output_dim 3 to 16: neither the pad rows nor the pad outputs
    reach grad_weights"""
    from enerf_amd.ffmlp import FFMLP
    dtype = TORCH16[kind]
    monkeypatch.setattr(FFMLP, "compute_dtype", dtype)
    n = _net(NL, 32, 384)
    Bp = B + (128 - B % 128)
    xp, dyp = np.zeros((Bp, 32)), np.zeros((Bp, 16))
    xp[:B], dyp[:B, :3] = n["x"][:B], n["dy"][:B, :3]
    y, fb = R.forward(xp, n["W"], 32, NL, 0, 6, None)
    dx, gw, bb = R.backward(dyp, xp, n["W"], fb, 32, NL, 0, None)
    assert all(R._is_exact(a) for a in (y, fb, bb, dx)) and not gw[-13 * 64:].any() and np.abs(gw).max() < 2.0 ** 24
    gw = R.r16(gw, kind)                     # the one rounding of the exact total
    net = FFMLP(32, 3, 64, NL).to(DEV).train()
    net.weights.data.copy_(torch.as_tensor(n["W"], dtype=torch.float32))
    xt = torch.as_tensor(xp[:B], dtype=torch.float32, device=DEV).requires_grad_(True)
    out = net(xt)
    assert out.shape == (B, 3) and out.dtype == dtype
    (out.float() * torch.as_tensor(dyp[:B, :3], dtype=torch.float32, device=DEV)).sum().backward()
    Wo = R.Worst()
    Wo.exact("y", out.detach().double().cpu().numpy(), y[:B, :3])
    Wo.exact("dX", xt.grad.double().cpu().numpy(), dx[:B])
    Wo.exact("dW", net.weights.grad.double().cpu().numpy(), gw)
    net.eval()
    with torch.no_grad():
        Wo.exact("y (inference)", net(xt.detach()).double().cpu().numpy(), y[:B, :3])
    _finish(Wo, f"module NL={NL} B={B} {kind}")


def _ffnerf_run(n, kind, misalign=0):
    """-> (sigma Buf, rgb Buf, return code)"""
    L = _lib()
    M, Mp = n["M"], n["Mp"]
    feats = Buf(16 * Mp, 2, torch.float32, n["feats"].reshape(16 * Mp, 2))
    dirs = Buf(M, 3, torch.float32, n["dirs"])
    Ws, Wc = Buf(1, R.SIGMA_W, torch.float32, n["Ws"]), Buf(1, R.COLOR_W, torch.float32, n["Wc"])
    sigma, rgb = Buf(M, 1, torch.float32), Buf(M, 3, torch.float32)
    code = {"bf16": L.BF16, "fp16": L.F16}.get(kind, L.F32)
    rc = L.lib().enerf_ffnerf_inference(feats.t.data_ptr() + misalign, dirs.t.data_ptr(), Ws.t.data_ptr(), Wc.t.data_ptr(), M,
                                        code, sigma.t.data_ptr(), rgb.t.data_ptr(), L.stream_handle())
    torch.cuda.synchronize()
    _canaries(feats=feats, dirs=dirs, Ws=Ws, Wc=Wc, sigma=sigma, rgb=rgb)
    return sigma, rgb, rc


def _ffnerf_check(n, kind, exact, title):
    iv = R.ffnerf_intervals(n["feats"], n["dirs"], n["Ws"], n["Wc"], n["M"], kind, exact_sigma=exact)
    sigma, rgb, rc = _ffnerf_run(n, kind)
    assert rc == 0
    Wo = R.Worst()
    Wo.interval("sigma", sigma.np()[:, 0], *iv["sigma"])
    Wo.interval("rgb", rgb.np(), *iv["rgb"])
    ws = R.width_stats(iv["raw_s"][0][:, :1], iv["raw_s"][1][:, :1], kind) if not exact else dict(max=0.0, q99=0.0, median=0.0)
    wc = R.width_stats(*iv["raw_c"], kind)
    print(f"{title}: widths sigma_raw max {ws['max']:.3g} median {ws['median']:.3g}, colour max {wc['max']:.3g} "
          f"q99 {wc['q99']:.3g} median {wc['median']:.3g}")
    assert max(ws["max"], wc["max"]) <= 64 and max(ws["median"], wc["median"]) <= 16
    _finish(Wo, title)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("M", [1, 31, 33, 64, 65, 4097])
def test_exact_nets_fused_inference(M, kind):
    _ffnerf_check(R.exact_ffnerf(M, 9), kind, True, f"fused inference exact M={M} {kind}")


# ---------------------------------------------------------------------------- c. the wrapped persistent loops (bf16 only)
def test_wrapped_forward_and_inference(buffered):
    n = _net(2, 32, WRAP_B, 2.0 ** -6)
    assert R.fwd_geometry(WRAP_B) == (512, 2048, 2, 1)          # 2054 pairs on 2048 waves: some make two trips, most one
    dtype = torch.bfloat16
    W, x = Buf(1, n["W"].size, dtype, n["W"]), Buf(WRAP_B, 32, dtype, n["x"])
    Wo = R.Worst()
    fb, y = _forward(x, W, WRAP_B, 32, 2, 0, 6, dtype)
    _same_bits(Wo, "y", y.t, n["y"], dtype)
    _same_bits(Wo, "fb", fb.t, n["fb"], dtype)
    fbi, yi = _forward(x, W, WRAP_B, 32, 2, 0, 6, dtype, inference=True)
    _same_bits(Wo, "y (inference)", yi.t, n["y"], dtype)
    assert fbi.untouched()
    _canaries(W=W, x=x, fb=fb, y=y, yi=yi)
    _finish(Wo, f"wrapped forward B={WRAP_B}")


@pytest.mark.parametrize("recompute", [False, True], ids=["buffered", "recompute"])
def test_wrapped_backward(recompute):
    n = _net(2, 32, WRAP_B, 2.0 ** -6)
    assert R.bwd_geometry(WRAP_B)[2:] == (3, 2) and R.bwd_geometry(WRAP_B, 256)[2:] == (5, 4)
    # (the recomputing route: mlp32.hip's pgrid, forward cap 512 and backward cap 256 workgroups of four 32-row waves)
    assert [g[2:] for g in R.recompute_geometry(WRAP_B)] == [(3, 2), (5, 4)]
    _finish(_exact_route(n, "bf16", recompute, True), f"wrapped backward B={WRAP_B} {'recompute' if recompute else 'buffered'}")


@pytest.mark.parametrize("M", [131072 + 97, 131072 + 65])
def test_wrapped_fused_inference(M):
    # 131072 + 97 samples are 4100 tiles; 131072 + 65 are 4099, an odd count: the last group's second tile is past the end
    blocks, nw, most, least, tiles = R.ffnerf_geometry(M)
    assert (blocks, most, least) == (512, 2, 1) and tiles == (4100 if M == 131072 + 97 else 4099)
    _ffnerf_check(R.exact_ffnerf(M, 9), "bf16", True, f"wrapped fused inference M={M}")


# --------------------------------------------------------------------------------------- d. end to end, random values
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("NL,B", [(2, 256), (3, 640), (2, 640), (3, 256)])
def test_recomputing_entry_points_end_to_end(NL, B, kind):
    assert _lib().lib().enerf_ffmlp_recompute(-1) == 1
    dtype = TORCH16[kind]
    # (zero-mean weights put the widest of the three-layer fp16 intervals at 42 .. 74 units, around the cap whatever the
    # scale -- ReLU nets are scale invariant; a mean of 0.1 halves the widths and leaves a fifth of the units inactive)
    Wn, xn, dyn = _random(32, NL, B, kind, WIDTH_WSCALE, 0.1)
    (ylo, yhi), layers = R.propagate_forward(xn, xn, Wn, 32, NL, 0, 6, kind)
    dX, dW = R.propagate_backward(dyn, xn, Wn, layers, 32, NL, 0, kind, R.wgrad_chain_any_order(B))
    W, x, dy = Buf(1, Wn.size, dtype, Wn), Buf(B, 32, dtype, xn), Buf(B, 16, dtype, dyn)
    fb, y = _forward(x, W, B, 32, NL, 0, 6, dtype)
    bb, dx, gw = _backward(dy, x, W, fb, B, 32, NL, 0, dtype)
    assert fb.untouched() and bb.untouched()
    Wo = R.Worst()
    Wo.interval("y", y.np(), ylo, yhi)
    Wo.interval("dX", dx.np(), *dX)
    Wo.interval("dW", gw.np().ravel(), *dW)
    st = R.width_stats(ylo, yhi, kind)
    print(f"recompute NL={NL} B={B} {kind}: y widths max {st['max']:.3g} q99 {st['q99']:.3g} median {st['median']:.3g}; "
          f"dX median {np.median(R.width_units(*dX, kind)):.3g}, dW median {np.median(R.width_units(*dW, kind)):.3g}")
    assert st["max"] <= 64 and st["median"] <= 16
    _canaries(W=W, x=x, dy=dy, y=y, dx=dx, gw=gw)
    _finish(Wo, f"recompute end to end NL={NL} B={B} {kind}")


@functools.lru_cache(maxsize=None)
def _random_ffnerf(M, kind):
    rng = np.random.default_rng(M)
    Mp = (M + 31) // 32 * 32
    feats = np.zeros((16, Mp, 2))
    feats[:, :M] = rng.uniform(-1, 1, (16, M, 2)).astype(np.float32)
    d = rng.normal(size=(M, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    # five layers deep, zero-mean weights leave outputs that are mostly cancellation, which intervals cannot follow (widths of
    # 75 .. 130 units at every scale tried on the host); a mean of 0.3 keeps the widths at 12 (bf16) and 24 (fp16) units
    Ws = R.r16((rng.uniform(-1, 1, R.SIGMA_W) + 0.3) * 0.15, kind)
    Wc = R.r16((rng.uniform(-1, 1, R.COLOR_W) + 0.3) * 0.08, kind)
    return dict(M=M, Mp=Mp, feats=feats, dirs=d, Ws=Ws, Wc=Wc)


@pytest.mark.parametrize("kind", R.KINDS)
def test_fused_inference_end_to_end(kind):
    _ffnerf_check(_random_ffnerf(4000, kind), kind, False, f"fused inference random M=4000 {kind}")


# ------------------------------------------------------------------------------------------------------------ e. refusals
REFUSALS = [("B % 128 != 0", dict(B=192)), ("hidden != 64", dict(hidden=32)), ("in = 48", dict(in_dim=48)),
            ("NL = 1", dict(NL=1)), ("NL = 5", dict(NL=5)), ("fp32", dict(fp32=True)), ("sine backward", dict(act=2))]


@pytest.mark.parametrize("recompute", [0, 1])
@pytest.mark.parametrize("what,over", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_write_nothing(what, over, recompute):
    L = _lib()
    a = dict(B=256, hidden=64, in_dim=32, NL=2, act=0, fp32=False)
    a.update(over)
    dtype = torch.float32 if a["fp32"] else torch.bfloat16
    code = L.F32 if a["fp32"] else L.BF16
    B, NL, in_dim = a["B"], a["NL"], a["in_dim"]
    W = Buf(1, 64 * (in_dim + 64 * 4 + 16), dtype, np.zeros(64 * (in_dim + 64 * 4 + 16)) + 0.125)
    x, dy = Buf(B, in_dim, dtype, np.ones((B, in_dim))), Buf(B, 16, dtype, np.ones((B, 16)))
    fb, bb = Buf(B, 64, dtype, lead=(5,)), Buf(B, 64, dtype, lead=(5,))
    y, dx, gw = Buf(B, 16, dtype), Buf(B, in_dim, dtype), Buf(1, W.n, dtype)
    lib, s = L.lib(), L.stream_handle()
    prev = lib.enerf_ffmlp_recompute(recompute)
    try:
        if what != "sine backward":
            assert lib.enerf_ffmlp_forward(x.t.data_ptr(), W.t.data_ptr(), B, in_dim, 16, a["hidden"], NL, a["act"], 6,
                                           fb.t.data_ptr(), y.t.data_ptr(), code, s) != 0
            assert lib.enerf_ffmlp_inference(x.t.data_ptr(), W.t.data_ptr(), B, in_dim, 16, a["hidden"], NL, a["act"], 6,
                                             fb.t.data_ptr(), y.t.data_ptr(), code, s) != 0
        fb_in = Buf(B, 64, dtype, np.ones((5 * B, 64)), lead=(5,))
        assert lib.enerf_ffmlp_backward(dy.t.data_ptr(), x.t.data_ptr(), W.t.data_ptr(), fb_in.t.data_ptr(), B, in_dim, 16,
                                        a["hidden"], NL, a["act"], 6, 1, bb.t.data_ptr(), dx.t.data_ptr(), gw.t.data_ptr(),
                                        code, s) != 0
    finally:
        lib.enerf_ffmlp_recompute(prev)
    torch.cuda.synchronize()
    assert fb.untouched() and bb.untouched() and y.untouched() and dx.untouched() and gw.untouched()
    _canaries(W=W, x=x, dy=dy, fb_in=fb_in)


@pytest.mark.parametrize("what", ["misaligned feats", "fp32"])
def test_fused_inference_refusals_write_nothing(what):
    n = _random_ffnerf(4000, "bf16")
    sigma, rgb, rc = _ffnerf_run(n, "bf16" if what == "misaligned feats" else "fp32", misalign=4 if what == "misaligned feats" else 0)
    assert rc != 0 and sigma.untouched() and rgb.untouched()
