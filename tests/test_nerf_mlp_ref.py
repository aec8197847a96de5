"""The checker of tests/nerf_mlp_ref.py has teeth: an ideal kernel (the fp64 reference rounded to fp32) passes every bar, and
nine deliberately wrong kernels, rounded the same way, each fail at least one.  No GPU: `_kernel` below is the whole
forward + backward once more in fp64, with one wrong step per mutant."""
import pytest
import torch

import nerf_mlp_ref as R


def _bf16(t):
    return t.float().bfloat16().double()


def _kernel(inp, ws, scale=1.0, wrong=None):
    """What a kernel with the defect `wrong` (None: none) hands back, as fp32."""
    X, d, g_rgb, g_sigma = (inp[k].double() for k in ("X", "d", "g_rgb", "g_sigma"))
    ws0, ws1, wc0, wc1, wc2 = (w.double() for w in ws)
    wc0 = wc0[:, :31]
    sh = R.sh64(d)
    if wrong == "sh 1 <-> 3":
        sh = sh[:, [0, 3, 2, 1] + list(range(4, 16))]
    wc0_used = wc0
    if wrong == "geo columns shifted":
        wc0_used = torch.cat([wc0[:, :16], torch.roll(wc0[:, 16:], 1, dims=1)], dim=1)
    p0 = X @ ws0.t()
    a0 = torch.relu(p0)
    h = a0 @ ws1.t()
    cin = torch.cat([sh, h[:, 1:16]], dim=1)
    p1 = cin @ wc0_used.t()
    a1 = torch.relu(p1)
    p2 = a1 @ wc1.t()
    a2 = torch.relu(p2)
    s = torch.sigmoid(a2 @ wc2.t())
    ds = s * (1 - s)
    if wrong == "no sigmoid' from channel 4":
        ds[:, 4:] = 1.0
    dp3 = g_rgb * ds
    dp2 = (dp3 @ wc2) * ((p1 if wrong == "mask of layer 2 from layer 1" else p2) > 0)
    dp1 = (dp2 @ wc1) * (p1 > 0)
    dcin = dp1 @ wc0_used
    h0 = h[:, 0] if wrong == "no clamp" else h[:, 0].clamp(-15, 15)
    dh0 = g_sigma * (1.0 if wrong == "no sigma_scale" else scale) * torch.exp(h0)
    dh = torch.cat([dh0[:, None], dcin[:, 16:31]], dim=1)
    dp0 = (dh @ ws1) * (p0 > 0)
    pairs = dict(dwc2=(dp3, a2), dwc1=(dp2, a1), dwc0=(dp1, cin), dws1=(dh, a0), dws0=(dp0, X))
    keep = torch.ones(X.shape[0], dtype=torch.float64)
    if wrong == "row 17 dropped":
        keep[17] = 0
    if wrong == "rows 128..159 dropped":
        keep[128:160] = 0
    out = {k: (dy * keep[:, None]).t() @ x for k, (dy, x) in pairs.items()}
    out["dX"] = dp0 @ ws0
    if wrong == "bf16 operands":                 # the sigma net's first layer in the backward: lo halves dropped
        out["dws0"] = _bf16(dp0).t() @ _bf16(X)
        out["dX"] = _bf16(dp0) @ _bf16(ws0)
    out.update(sigma=torch.exp(h[:, 0]), rgb=s)
    return {k: v.float() for k, v in out.items()}


def _large_h0(B, seed):
    ws = R.default_weights(3, seed)
    inp = R.make_batch(B, ws, seed + 1)
    R.scale_h0_row(ws, inp["X"])
    return ws, inp


def test_explicit_backward_equals_fp64_autograd():
    for out_c, scale, big in ((3, 1.0, False), (5, 0.25, True)):
        ws = R.default_weights(out_c, 11)
        inp = R.make_batch(257, ws, 12)
        if big:
            R.scale_h0_row(ws, inp["X"])
        ref = R.reference(inp["X"], inp["d"], ws, inp["g_rgb"], inp["g_sigma"], scale)

        class TruncExp(torch.autograd.Function):         # enerf_amd/activation.py in fp64
            @staticmethod
            def forward(ctx, x):
                ctx.save_for_backward(x)
                return torch.exp(x)

            @staticmethod
            def backward(ctx, g):
                return g * torch.exp(ctx.saved_tensors[0].clamp(-15, 15))

        X = inp["X"].double().requires_grad_(True)
        wd = [w.double().requires_grad_(True) for w in ws]
        h = torch.relu(X @ wd[0].t()) @ wd[1].t()
        cin = torch.cat([R.sh64(inp["d"].double()), h[:, 1:16]], dim=1)
        rgb = torch.sigmoid(torch.relu(torch.relu(cin @ wd[2].t()) @ wd[3].t()) @ wd[4].t())
        sigma = TruncExp.apply(h[:, 0])
        ((rgb * inp["g_rgb"].double()).sum() + (sigma * scale * inp["g_sigma"].double()).sum()).backward()
        assert torch.equal(rgb.detach(), ref["rgb"]) and torch.equal(sigma.detach(), ref["sigma"])
        for name, t in zip(("dX",) + R.DW_NAMES, [X] + wd):
            top = float(t.grad.abs().max())
            assert top > 0 and float((ref[name] - t.grad).abs().max()) <= 1e-12 * top, name


@pytest.mark.parametrize("B", [33, 4097])
def test_ideal_kernel_passes_every_bar(B):
    ws = R.default_weights(3, 100 + B)
    inp = R.make_batch(B, ws, 200 + B)
    assert inp["rejected"] <= 0.15
    ref = R.reference(inp["X"], inp["d"], ws, inp["g_rgb"], inp["g_sigma"])
    got = _kernel(inp, ws)
    for k in R.OUTPUTS:                                  # `_kernel` without a defect is the reference
        assert torch.equal(got[k], ref[k].float()), k
    q = R.check(ref, got, f"ideal, B {B}")
    assert set(q) == set(R.OUTPUTS) and max(q.values()) <= 2e-3       # (fp32 rounding: 2^-25 of an rgb below 1 against 2e-5)


def test_large_h0_weights_clamp_on_both_sides():
    ws, inp = _large_h0(321, 40)
    R.assert_large_h0(R.reference(inp["X"], inp["d"], ws, inp["g_rgb"], inp["g_sigma"], 0.25))


# wrong kernel -> (B, out_c, sigma_scale, large |h0|, the outputs that may carry the failure)
MUTANTS = {
    "row 17 dropped": (33, 3, 1.0, False, R.DW_NAMES),
    "rows 128..159 dropped": (289, 3, 1.0, False, R.DW_NAMES),
    "no sigma_scale": (33, 3, 0.25, False, ("dX", "dws0", "dws1")),
    "no clamp": (321, 3, 0.25, True, ("dX", "dws0", "dws1")),
    "sh 1 <-> 3": (33, 3, 1.0, False, R.OUTPUTS),
    "geo columns shifted": (33, 3, 1.0, False, R.OUTPUTS),
    "no sigmoid' from channel 4": (33, 5, 1.0, False, R.OUTPUTS),
    "mask of layer 2 from layer 1": (33, 3, 1.0, False, R.OUTPUTS),
    "bf16 operands": (33, 3, 1.0, False, ("dX", "dws0")),
}


@pytest.mark.parametrize("wrong", list(MUTANTS))
def test_wrong_kernel_fails_a_bar(wrong):
    B, out_c, scale, big, where = MUTANTS[wrong]
    if big:
        ws, inp = _large_h0(B, 40)
    else:
        ws = R.default_weights(out_c, 304 + B + out_c)
        inp = R.make_batch(B, ws, 404 + B + out_c)
    ref = R.reference(inp["X"], inp["d"], ws, inp["g_rgb"], inp["g_sigma"], scale)
    if big:
        R.assert_large_h0(ref)
    R.check(ref, _kernel(inp, ws, scale), f"ideal for '{wrong}'")
    q = R.ratios(ref, _kernel(inp, ws, scale, wrong))
    print(f"err / bar ['{wrong}']: " + "  ".join(f"{k} {v:.3g}" for k, v in q.items()))
    failed = [k for k, v in q.items() if not v <= 1.0]
    assert failed and set(failed) <= set(where), (wrong, q)


def test_every_batch_of_the_gpu_module_can_be_drawn():
    """The GPU module's inputs are drawn on the host: the rejection share (asserted inside make_batch) and case D's
    conditions hold for every one of them, and each holds its all-zero row."""
    import test_gpu_nerf_mlp_fp64 as G
    n = 0
    for name, spec in G.all_specs():
        ws, inp = G.draw(spec)
        assert inp["rejected"] <= 0.15, name
        assert spec["B"] < 2 or bool((inp["X"] == 0).all(dim=1).any()), name
        if spec["large_h0"]:
            R.assert_large_h0(R.reference(inp["X"], inp["d"], ws, inp["g_rgb"], inp["g_sigma"], spec["scale"]))
        n += 1
    assert n >= 20
