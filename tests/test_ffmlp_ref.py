"""tests/ffmlp_ref.py on the host: R16 against torch's casts, the float64 definition against autograd, the C oracle's
rounded FFMLP against the layer-wise interval comparator, the exact nets and their assertions, the width conditions that
keep the propagated intervals from being vacuous, and thirteen seeded defects, each applied to a numpy model of the
kernels' result and each rejected on a named case (7 and 8 by the random layer-wise cases, the rest by the exact nets)."""
import functools

import numpy as np
import pytest
import torch

import ffmlp_ref as R

TORCH16 = {"bf16": torch.bfloat16, "fp16": torch.float16}
WRAP_B = 131072 + 384
WIDTH_WSCALE = 0.15      # weights U(-1, 1) x this in the width conditions (0.2 gave 67 > 64 units at fp16, three layers)


# ------------------------------------------------------------------------------------------------------------------ R16
@pytest.mark.parametrize("kind", R.KINDS)
def test_r16_is_torch_cast(kind):
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.normal(size=20000) * 10.0 ** rng.integers(-12, 5, 20000), [0.0, -0.0, 1.0, 65504.0, 65519.9],
                        2.0 ** -24 * np.arange(-9, 10) / 2, 2.0 ** -133 * np.arange(-9, 10) / 2, 2.0 ** -126 * (1 + 2.0 ** -8 * np.arange(8))])
    v32 = v.astype(np.float32)
    # ties of the 16-bit grid, exactly representable in fp32
    grid = torch.tensor(v32).to(TORCH16[kind]).float().numpy().astype(np.float64)
    grid = grid[np.isfinite(grid)]
    ties = (grid + 0.5 * R.ulp16(grid, kind) * np.sign(grid + 1e-300)).astype(np.float32)
    allv = np.concatenate([v32, ties])
    want = torch.tensor(allv).to(TORCH16[kind]).double().numpy()
    got = R.r16(allv.astype(np.float64), kind)
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
    t = R.r16(allv.astype(np.float64), kind, trunc=True)
    assert np.all(np.abs(t) <= np.abs(allv.astype(np.float64))) and np.all(np.abs(t - allv) < R.ulp16(allv, kind) * (1 + 1e-9))
    assert np.array_equal(R.r16(t, kind), t)


# ------------------------------------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("act", [0, 3, 5, 6])
@pytest.mark.parametrize("in_dim", [16, 32, 64])
@pytest.mark.parametrize("NL", [2, 3, 4])
def test_definition_is_autograd(NL, in_dim, act):
    rng = np.random.default_rng(NL * 100 + in_dim + act)
    B = 48
    W = rng.uniform(-1, 1, R.blob_size(in_dim, NL)) * 0.3
    x, dy = rng.uniform(-1, 1, (B, in_dim)), rng.uniform(-1, 1, (B, 16))
    gw_old = rng.uniform(-1, 1, W.size)
    y, fb = R.forward(x, W, in_dim, NL, act, 6, None)
    dx, gw, _ = R.backward(dy, x, W, fb, in_dim, NL, act, None, gw_old=gw_old)
    f = {0: torch.relu, 3: torch.sigmoid, 5: lambda t: torch.nn.functional.softplus(t, beta=10.0, threshold=1e9), 6: lambda t: t}[act]
    xt = torch.tensor(x, requires_grad=True)
    Wt = torch.tensor(W, requires_grad=True)
    h, off = xt, 0
    for l in range(NL + 1):
        rows, cols = (16 if l == NL else 64), (in_dim if l == 0 else 64)
        h = torch.nn.functional.linear(h, Wt[off:off + rows * cols].view(rows, cols))
        off += rows * cols
        if l < NL:
            h = f(h)
    (h * torch.tensor(dy)).sum().backward()
    assert np.abs(y - h.detach().numpy()).max() < 1e-12
    assert np.abs(dx - xt.grad.numpy()).max() < 1e-12
    assert np.abs(gw - gw_old - Wt.grad.numpy()).max() < 1e-12


# ---------------------------------------------------------------------------------------------------------- the C oracle
def _random_case(in_dim, NL, B, kind, seed, wscale=np.sqrt(3 / 64) * 1.5):
    rng = np.random.default_rng(seed)
    W = R.r16(rng.uniform(-1, 1, R.blob_size(in_dim, NL)) * wscale, kind)
    return W, R.r16(rng.uniform(-1, 1, (B, in_dim)), kind), R.r16(rng.uniform(-1, 1, (B, 16)), kind)


@pytest.mark.parametrize("rnd", [1, 2])
@pytest.mark.parametrize("in_dim,NL,B,act", [(32, 2, 256, 0), (64, 4, 384, 0), (16, 3, 128, 0), (32, 2, 128, 3),
                                              (32, 2, 128, 5), (32, 2, 128, 1), (32, 2, 128, 4)])
def test_oracle_passes_the_layerwise_comparator(in_dim, NL, B, act, rnd):
    from oracle import oracle as O
    kind = R.KINDS[rnd - 1]
    W, x, dy = _random_case(in_dim, NL, B, kind, 11 * in_dim + NL, wscale=0.3 if act else np.sqrt(3 / 64) * 1.5)
    y, fb = O.ffmlp_forward(x, W, in_dim, 16, 64, NL, act, 6, rnd=rnd)
    dx, gw, bb = O.ffmlp_backward(dy, x, W, fb, in_dim, 16, 64, NL, act, True, rnd=rnd)
    Wo = R.Worst()
    R.check_forward_layers(Wo, x, W, in_dim, NL, act, 6, kind, fb, y)
    # the oracle sums the batch sequentially (a chain of B additions) and leaves the weight gradient in fp32: its one
    # rounding to 16 bits is applied here
    R.check_backward_layers(Wo, dy, x, W, fb, in_dim, NL, act, kind, bb, dx, R.r16(gw, kind), K_w=B + 1)
    print(Wo.report(f"oracle rnd={rnd} in={in_dim} NL={NL} B={B} act={act}"))
    assert not Wo.fails, "\n".join(Wo.fails)


# ------------------------------------------------------------------------------------------------------------ exact nets
@functools.lru_cache(maxsize=None)
def _net(NL, in_dim, B, seed=5, dy_scale=1.0):
    return R.exact_net(NL, in_dim, B, seed, dy_scale=dy_scale)


@pytest.mark.parametrize("NL,in_dim", [(2, 32), (3, 32), (4, 64), (2, 16)])
def test_exact_nets_exist(NL, in_dim):
    n = _net(NL, in_dim, 384)
    for kind in R.KINDS:                          # the rounded definition reproduces them bit for bit in both types
        y, fb = R.forward(n["x"], n["W"], in_dim, NL, 0, 6, kind)
        dx, gw, bb = R.backward(n["dy"], n["x"], n["W"], fb, in_dim, NL, 0, kind)
        assert np.array_equal(y, n["y"]) and np.array_equal(fb, n["fb"]) and np.array_equal(bb, n["bb"])
        assert np.array_equal(dx, n["dx"]) and np.array_equal(gw, R.exact_gw(n, kind))
    for f in n["fb"]:
        assert (f != 0).mean() >= 0.15 and np.unique(f).size >= 5
    assert (n["bb"] != 0).mean() > 0.02 and (n["dx"] != 0).mean() > 0.1
    # any summation order: an fp32 accumulation in a scrambled order gives the same bits
    perm = np.random.default_rng(0).permutation(n["B"])
    d, i = R.wgrad_operands(n["dy"], n["x"], n["fb"], n["bb"], NL, 1)
    a = np.zeros((64, 64), np.float32)
    for s in perm[:128]:
        a += np.outer(d[s], i[s]).astype(np.float32)
    assert np.array_equal(a.astype(np.float64), d[perm[:128]].T @ i[perm[:128]])


def test_wrapped_loop_net_is_exact_and_wraps():
    n = _net(2, 32, WRAP_B, dy_scale=2.0 ** -6)
    assert float(np.abs(R.exact_gw(n, "bf16")).max()) > 0
    assert R.fwd_geometry(WRAP_B)[2:] == (2, 1) and R.bwd_geometry(WRAP_B)[2:] == (3, 2)
    assert R.bwd_geometry(WRAP_B, 256)[2:] == (5, 4) and R.ffnerf_geometry(131072 + 97)[2:4] == (2, 1)
    # (131072 + 97 samples are 4100 tiles, an even count; 131072 + 65 are 4099: the last group's second tile is past the end)
    assert R.ffnerf_geometry(131072 + 65)[2:] == (2, 1, 4099)
    assert [g[2:] for g in R.recompute_geometry(WRAP_B)] == [(3, 2), (5, 4)]


# ---------------------------------------------------------------------------------------------------------------- widths
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("NL", [2, 3])
def test_propagated_intervals_are_not_vacuous(NL, kind):
    W, x, dy = _random_case(32, NL, 4096, kind, 40 + NL, wscale=WIDTH_WSCALE)
    (lo, hi), layers = R.propagate_forward(x, x, W, 32, NL, 0, 6, kind)
    st = R.width_stats(lo, hi, kind)
    print(f"widths {kind} NL={NL}: max {st['max']:.3g} q99 {st['q99']:.3g} median {st['median']:.3g}")
    assert st["max"] <= 64 and st["median"] <= 16
    y, _ = R.forward(x, W, 32, NL, 0, 6, kind)
    assert np.all((y >= lo) & (y <= hi))
    y32 = _model_forward(x, W, 32, NL, 0, kind)[0]
    assert np.all((y32 >= lo) & (y32 <= hi))


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("NL,B", [(2, 256), (3, 640)])
def test_propagated_backward_holds_the_definition_and_an_fp32_model(NL, B, kind):
    W, x, dy = _random_case(32, NL, B, kind, 60 + NL, wscale=0.2)
    (lo, hi), layers = R.propagate_forward(x, x, W, 32, NL, 0, 6, kind)
    dX, dW = R.propagate_backward(dy, x, W, layers, 32, NL, 0, kind, R.wgrad_chain_any_order(B))
    for fwd in (lambda: R.forward(x, W, 32, NL, 0, 6, kind), lambda: _model_forward(x, W, 32, NL, 0, kind)):
        y, fb = fwd()
        dx, gw, _ = R.backward(dy, x, W, fb, 32, NL, 0, kind)
        assert np.all((dx >= dX[0]) & (dx <= dX[1])) and np.all((gw >= dW[0]) & (gw <= dW[1]))
    for name, (l, h), ref in (("dX", dX, dx), ("dW", dW, gw)):
        w = (h - l) / (np.sqrt(np.mean(ref * ref)) * R.EPS16[kind])
        print(f"widths {kind} NL={NL} B={B} {name}: max {w.max():.3g} q99 {np.quantile(w, 0.99):.3g} median {np.median(w):.3g}")


# ------------------------------------------------------------------------------------- numpy models of the kernels' result
def _model_forward(x, W, in_dim, NL, act, kind, mode="fp32"):
    """a forward as a kernel might compute it: fp32 sums (mode fp32), sums accumulated in 16 bits (acc16: defect 7),
    truncating stores (trunc: defect 8)"""
    m = R.split(np.asarray(W, np.float64), in_dim, NL)
    h, fb = np.asarray(x, np.float64), []
    for l in range(NL + 1):
        if mode == "acc16":
            z = np.zeros((h.shape[0], m[l].shape[0]))
            for k in range(h.shape[1]):
                z = R.r16(z + h[:, k:k + 1] * m[l][None, :, k], kind)
        else:
            z = (h.astype(np.float32) @ m[l].T.astype(np.float32)).astype(np.float64)
        a = R.act_fwd(z, act if l < NL else 6).astype(np.float32).astype(np.float64)
        h = R.r16(a, kind, trunc=(mode == "trunc"))
        fb.append(h)
    return fb[-1], np.stack(fb[:-1])


NAT = [8 * h + e for h in range(2) for e in range(8)]
PERM = [4 * h + (e & 3) + 8 * (e >> 2) for h in range(2) for e in range(8)]


def _defective_forward(n, defect):
    NL, in_dim, B = n["NL"], n["in_dim"], n["B"]
    W, x = n["W"].copy(), n["x"].copy()
    if defect == 1:                # K-block 1 of the first hidden matrix read in natural instead of permuted order
        Wh = R.split(W, in_dim, NL)[1]
        blk = Wh[:, 16:32].copy()
        Wh[:, 16 + np.array(NAT)] = blk[:, PERM]
    if defect == 3:                # second trip: the first trip's inputs
        nw = R.fwd_geometry(B)[1]
        x[64 * nw:] = x[:B - 64 * nw]
    y, fb = R.forward(x, W, in_dim, NL, 0, 6, "bf16")
    if defect == 2:                # the last 32-sample tile left stale (the NaN fill)
        y[-32:] = np.nan
    return y, fb


def _defective_backward(n, defect, kind="bf16", gw_old=None, canary=4):
    """-> dX [B + canary rows, in], dW [blob + canary], bb: the buffers as a defective kernel leaves them (NaN fill)"""
    NL, in_dim, B = n["NL"], n["in_dim"], n["B"]
    m = R.split(n["W"], in_dim, NL)
    fb, dy, x = n["fb"], n["dy"], n["x"]
    g, bb = dy, []
    for jj in range(NL):
        wt = m[NL] if jj == 0 else m[NL - jj]
        src = NL - 1 - jj
        if defect == 4 and jj > 0:
            src += 1                # the ReLU mask from fb[l] instead of fb[l-1]
        g = R.r16((g @ wt) * (fb[src] > 0), kind)
        bb.append(g)
    bb = np.stack(bb)
    dx = np.full((B + canary, in_dim), np.nan)
    dx[:B] = R.r16(g @ m[0], kind)
    if defect == 11 and in_dim == 64:
        dx[:B, 32:] = np.nan       # the second 32-column block never written
    if defect == 11 and in_dim == 16:
        flat = dx.reshape(-1)      # 32 columns written per row: rows overlap, the last one spills past the end
        full = np.concatenate([R.r16(g @ m[0], kind), np.zeros((B, 16))], 1)
        for s in range(B):
            flat[16 * s:16 * s + 32] = full[s]
    rows = np.ones(B, bool)
    if defect == 9:                # the reduce drops the last partial group of 16 workgroups
        nblocks, nw = R.bwd_geometry(B, 256)[:2]
        blk = (np.arange(B // 32) % nw) // 4
        rows = np.repeat(blk < 16 * (nblocks // 16), 32)
    bbw = bb[::-1] if defect == 5 else bb          # slots indexed m instead of NL-1-m
    sums = R.weight_sums(dy[rows], x[rows], fb[:, rows], bbw[:, rows], NL)
    old = np.zeros_like(sums) if gw_old is None else gw_old
    gw = np.full(sums.size + canary * 64, np.nan)
    gw[:sums.size] = R.r16((0 if defect == 10 else old) + sums, kind)
    if defect == 11 and in_dim == 64:
        gw[:64 * 64].reshape(64, 64)[:, 32:] = old[:64 * 64].reshape(64, 64)[:, 32:]
    if defect == 6:                # rows 16..31 of the Wout tile live: its weight-gradient rows land past the blob's end
        gw[sums.size:sums.size + canary * 64] = 0.0
    return dx, gw, bb


def _clean(n, kind="bf16", gw_old=None, canary=4):
    dx = np.full((n["B"] + canary, n["in_dim"]), np.nan)
    dx[:n["B"]] = n["dx"]
    gw = np.full(n["sums"].size + canary * 64, np.nan)
    gw[:n["sums"].size] = R.exact_gw(n, kind, gw_old)
    return dx, gw, n["bb"]


def _rejects(got, want):
    Wo = R.Worst()
    for k, (g, w) in enumerate(zip(got, want)):
        Wo.exact(str(k), g, w)
    return bool(Wo.fails)


@pytest.mark.parametrize("defect", [1, 2, 3])
def test_exact_nets_reject_forward_defects(defect):
    n = _net(2, 32, WRAP_B, dy_scale=2.0 ** -6) if defect == 3 else _net(3, 32, 384)
    assert not _rejects(_defective_forward(n, None), (n["y"], n["fb"]))
    assert _rejects(_defective_forward(n, defect), (n["y"], n["fb"]))


@pytest.mark.parametrize("defect,NL,in_dim,B", [(4, 3, 32, 384), (5, 3, 32, 384), (6, 2, 32, 384), (9, 2, 32, 6400),
                                                 (10, 2, 32, 384), (11, 4, 64, 384), (11, 2, 16, 384)])
def test_exact_nets_reject_backward_defects(defect, NL, in_dim, B):
    n = _net(NL, in_dim, B)
    old = np.random.default_rng(3).integers(-3, 4, n["sums"].size).astype(np.float64)
    assert not _rejects(_defective_backward(n, None, gw_old=old), _clean(n, gw_old=old))
    assert _rejects(_defective_backward(n, defect, gw_old=old), _clean(n, gw_old=old))
    if defect == 9:
        assert R.bwd_geometry(B, 256)[0] % 16 != 0


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("defect", [7, 8])
def test_random_layerwise_cases_reject_16_bit_sums_and_truncation(defect, kind):
    W, x, _ = _random_case(32, 2, 384, kind, 77)

    def run(mode):
        y, fb = _model_forward(x, W, 32, 2, 0, kind, mode)
        Wo = R.Worst()
        R.check_forward_layers(Wo, x, W, 32, 2, 0, 6, kind, fb, y)
        return Wo
    assert not run("fp32").fails
    assert run({7: "acc16", 8: "trunc"}[defect]).fails


def _ffnerf_model(n, kind, defect=None):
    M = n["M"]
    x = R.r16(R.feats_rows(n["feats"], M), kind)
    raw, _ = _model_forward(x, n["Ws"], 32, 2, 0, kind)
    d = n["dirs"].copy()
    if defect == 13:               # a sample's direction taken from its neighbour
        d = np.roll(d, -1, axis=0)
    sh = R.r16(R.sh4(d)[0].astype(np.float32).astype(np.float64), kind)
    cin = np.concatenate([sh, raw[:, 1:], np.zeros((M, 1))], 1)
    if defect == 12:               # sigma_raw as geo feature 0: the structural zero lost
        cin = np.concatenate([sh, raw], 1)
    out, _ = _model_forward(cin, n["Wc"], 32, 3, 0, kind)
    sig = R.r16(np.exp(raw[:, 0]).astype(np.float32).astype(np.float64), kind)
    rgb = R.r16((1 / (1 + np.exp(-out[:, :3]))).astype(np.float32).astype(np.float64), kind)
    return sig, rgb


@pytest.mark.parametrize("kind", R.KINDS)
def test_exact_fused_net_rejects_its_defects(kind):
    n = R.exact_ffnerf(97, 9)
    iv = R.ffnerf_intervals(n["feats"], n["dirs"], n["Ws"], n["Wc"], n["M"], kind, exact_sigma=True)
    # the sigma net of such a net is a single value per entry, the colour net's intervals single values or close neighbours
    assert np.array_equal(*iv["raw_s"])
    w = R.width_units(*iv["raw_c"], kind)
    print(f"exact fused net {kind}: colour output widths max {w.max():.3g} median {np.median(w):.3g}")
    assert w.max() <= 64 and np.median(w) <= 16

    def fails(defect):
        sig, rgb = _ffnerf_model(n, kind, defect)
        Wo = R.Worst()
        Wo.interval("sigma", sig, *iv["sigma"])
        Wo.interval("rgb", rgb, *iv["rgb"])
        return bool(Wo.fails), Wo
    bad, Wo = fails(None)
    assert not bad, Wo.fails
    assert fails(12)[0] and fails(13)[0]
    assert float(np.std(iv["rgb"][0])) > 0.01 and float(np.std(iv["sigma"][0])) > 0
