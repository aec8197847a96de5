"""fp64 reference, error model and checker for the fused NeRF MLP (csrc/nerf_mlp.hip: k_nerf_fwd, k_nerf_bwd).

The operation (nerf/network.py:104-132, weights without bias):
    h     = relu(X @ ws0.T) @ ws1.T                                  X [B, 32], ws0 [64, 32], ws1 [16, 64]
    cin   = [SH16(d) | h[:, 1:16]]                                   wc0 [64, 31] in memory order [SH 16 | geo 15]
    rgb   = sigmoid(relu(relu(cin @ wc0.T) @ wc1.T) @ wc2.T)         wc1 [64, 64], wc2 [out_c, 64]
    sigma = exp(h[:, 0])
and its backward under the kernel's contract (enerf_amd/activation.py: trunc_exp; torch's sigmoid_backward):
    d h0 = g_sigma * sigma_scale * exp(clamp(h0, -15, 15)),   d pre_rgb = g_rgb * s (1 - s)
-> dX and the five dW.  X is the row-major view of the kernel's feats [16, Bp, 2]: level l is columns 2l and 2l + 1.
reference() writes all of it out as plain fp64 matrix products and keeps every layer's input, pre-activation and
output gradient; tests/test_nerf_mlp_ref.py holds the explicit backward to fp64 autograd of the same graph.

Error model: that of test_fused_mlp_forward_backward (tests/test_gpu_mlp32.py) carried through the two-net chain.  Every
matrix product of the kernel errs by at most u x (the product of its operands' MAGNITUDES), u = 2^-16 being one split-bf16
product (hi*hi + hi*lo + lo*hi).  So magnitudes are propagated with the reference's own ReLU masks:
    forward   X^ = |X| -> A0^ = mask0 (X^ |ws0|^T) -> H^ = A0^ |ws1|^T -> Cin^ = [|SH| | H^[:, 1:16]] -> A1^ -> A2^ -> P3^
    backward  D3^ = |g_rgb| (s (1 - s) + e_rgb),   DH0^ = |g_sigma| sigma_scale exp(clamp h0) (1 + e_h0)
              D2^ = mask2 (D3^ |wc2|), D1^ = mask1 (D2^ |wc1|), DCin^ = D1^ |wc0|, DH^ = [DH0^ | DCin^[:, 16:31]],
              D0^ = mask0 (DH^ |ws1|), DX^ = D0^ |ws0|
e_h0 = 3 u H0^ is the forward's own bound on h0 (two products + 1); the same count bounds the colour net's pre-sigmoid
output by 6 u P3^ (five products + 1), the sigmoid's slope is at most 1/4 and |d(s (1 - s)) / ds| = |1 - 2 s| <= 1, so
e_rgb = 6 u P3^ / 4.  With A^ = D^T X^ of a layer, every entry must satisfy
    |dW - dW_fp64| <= 1e-4 |dW_fp64| + 6 u A^ + 1e-12        (6 = the five products of the chain + 1)
    |dX - dX_fp64| <= 1e-4 |dX_fp64| + 6 u DX^
and the forward  |rgb - rgb_fp64| <= 2e-5,  |sigma - sigma_fp64| <= (1e-4 + 3 u H0^) sigma_fp64.
A weight-gradient bar built from summed magnitudes grows with B while random round-off grows with sqrt(B): at a large
batch the per-sample dX bar carries the precision check (tests/test_nerf_mlp_ref.py: the lost-lo-half mutant).

Knife-edge samples get no allowance and no share of wrong entries is tolerated.  make_batch() instead draws
ceil(1.25 B) candidate rows, rejects a row when any of its three hidden layers' fp64 pre-activations lies within
4 * 8 * 2e-6 * max(max|pre|, 1) of zero without being zero (the "near" criterion of tests/test_gpu_mlp32.py) and keeps
the first B survivors: the strict bars then apply to every row.  At most 15 % of the pool may be rejected (asserted).
Every batch of two rows or more holds one row of all-zero features, whose first-layer pre-activations are exactly zero.
"""
import math

import torch

U = 2.0 ** -16                       # one split-bf16 product
NEAR = 4 * 8 * 2e-6                  # knife-edge distance, relative to max(max|pre|, 1) of the layer
DW_NAMES = ("dws0", "dws1", "dwc0", "dwc1", "dwc2")
OUTPUTS = ("sigma", "rgb", "dX") + DW_NAMES


def sh64(d):
    """The 16 real spherical harmonics of degree < 4 (shencoder.cu's polynomials) in float64."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xy, yz, xz, x2, y2, z2 = x * y, y * z, x * z, x * x, y * y, z * z
    return torch.stack([
        torch.full_like(x, 0.28209479177387814), -0.48860251190291987 * y, 0.48860251190291987 * z,
        -0.48860251190291987 * x, 1.0925484305920792 * xy, -1.0925484305920792 * yz,
        0.94617469575755997 * z2 - 0.31539156525251999, -1.0925484305920792 * xz,
        0.54627421529603959 * x2 - 0.54627421529603959 * y2, 0.59004358992664352 * y * (-3.0 * x2 + y2),
        2.8906114426405538 * xy * z, 0.45704579946446572 * y * (1.0 - 5.0 * z2),
        0.3731763325901154 * z * (5.0 * z2 - 3.0), 0.45704579946446572 * x * (1.0 - 5.0 * z2),
        1.4453057213202769 * z * (x2 - y2), 0.59004358992664352 * x * (-x2 + 3.0 * y2)], -1)


def pad32(n):
    return (n + 31) // 32 * 32


def to_level_major(X):
    """[B, 32] rows -> the kernel's feats [16, Bp, 2] (pad rows zero)."""
    B = X.shape[0]
    feats = torch.zeros(16, pad32(B), 2, dtype=X.dtype, device=X.device)
    feats[:, :B] = X.view(B, 16, 2).permute(1, 0, 2)
    return feats


def from_level_major(feats, B):
    """feats / dfeat [16, Bp, 2] -> its first B rows as [B, 32]."""
    return feats[:, :B].permute(1, 0, 2).reshape(B, 32)


def default_weights(out_c, seed):
    """ws0, ws1, wc0 [64, 31], wc1, wc2 in fp32 as nn.Linear initialises them (uniform, bound 1 / sqrt(fan_in))."""
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand(o, i, generator=g) * 2 - 1) / math.sqrt(i)).contiguous()
            for o, i in ((64, 32), (16, 64), (64, 31), (64, 64), (out_c, 64))]


def _pre_activations(X, d, ws):
    ws0, ws1, wc0, wc1 = (w.double() for w in ws[:4])
    p0 = X.double() @ ws0.t()
    h = torch.relu(p0) @ ws1.t()
    p1 = torch.cat([sh64(d.double()), h[:, 1:16]], dim=1) @ wc0[:, :31].t()
    p2 = torch.relu(p1) @ wc1.t()
    return p0, p1, p2


def _near(pres):
    near = torch.zeros(pres[0].shape[0], dtype=torch.bool)
    for pre in pres:
        near |= ((pre.abs() < NEAR * max(float(pre.abs().max()), 1.0)) & (pre != 0)).any(dim=1)
    return near


def make_batch(B, ws, seed):
    """-> dict(X [B, 32], d [B, 3], g_rgb [B, out_c], g_sigma [B]) of fp32 CPU tensors: features uniform in [-1, 1], unit
    directions, normal gradients, none of the rows a knife-edge sample for the weights `ws` (module docstring)."""
    out_c = ws[4].shape[0]
    P = math.ceil(1.25 * B)
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(P, 32, generator=g) * 2 - 1
    d = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1)
    g_rgb = torch.randn(P, out_c, generator=g)
    g_sigma = torch.randn(P, generator=g)
    ws = [w.cpu() for w in ws]
    if B >= 2:
        # the all-zero row: the first candidate after row 0 that is no knife-edge sample with its features zeroed
        zeroed = _near(_pre_activations(torch.zeros_like(X), d, ws))
        zeroed[0] = True
        X[int((~zeroed).nonzero()[0])] = 0
    near = _near(_pre_activations(X, d, ws))
    share = float(near.float().mean())
    assert share <= 0.15, f"{share:.3f} of the {P} candidate rows are knife-edge samples"
    keep = (~near).nonzero()[:B, 0]
    assert keep.numel() == B
    out = dict(X=X[keep].contiguous(), d=d[keep].contiguous(), g_rgb=g_rgb[keep].contiguous(),
               g_sigma=g_sigma[keep].contiguous())
    assert B < 2 or bool((out["X"] == 0).all(dim=1).any())
    out["rejected"] = share
    return out


def scale_h0_row(ws, X):
    """Scales row 0 of ws1 in place so that the largest |h0| of the rows X is 29: trunc_exp's clamp at +-15 then decides
    the gradient of a few per cent of the rows on either side (assert_large_h0).  The colour net never sees h0, so the
    rows' pre-activations -- and with them make_batch's choice of rows -- stay as they are."""
    h0 = torch.relu(X.double().cpu() @ ws[0].double().cpu().t()) @ ws[1][0].double().cpu()
    ws[1][0] *= 29.0 / float(h0.abs().max())


def assert_large_h0(ref):
    h0 = ref["h"][:, 0]
    hi, lo, top = float((h0 > 15).float().mean()), float((h0 < -15).float().mean()), float(h0.abs().max())
    assert hi >= 0.02 and lo >= 0.02 and top <= 30, (hi, lo, top)


def reference(X, d, ws, g_rgb, g_sigma, sigma_scale=1.0):
    """The fp64 statement of forward and backward on the given device, with every intermediate and the magnitudes of the
    error model.  `ws`: the five weights (wc0 with 31 or 32 columns: a pad column is ignored)."""
    X, d, g_rgb, g_sigma = X.double(), d.double(), g_rgb.double(), g_sigma.double()
    ws0, ws1, wc0, wc1, wc2 = (w.double() for w in ws)
    wc0 = wc0[:, :31]
    r = {}
    # ---- forward
    sh = sh64(d)
    p0 = X @ ws0.t()
    a0 = torch.relu(p0)
    h = a0 @ ws1.t()
    cin = torch.cat([sh, h[:, 1:16]], dim=1)
    p1 = cin @ wc0.t()
    a1 = torch.relu(p1)
    p2 = a1 @ wc1.t()
    a2 = torch.relu(p2)
    p3 = a2 @ wc2.t()
    s = torch.sigmoid(p3)
    r.update(sh=sh, p0=p0, a0=a0, h=h, cin=cin, p1=p1, a1=a1, p2=p2, a2=a2, p3=p3, rgb=s, sigma=torch.exp(h[:, 0]))
    # ---- backward
    ds = s * (1 - s)
    eh0 = torch.exp(h[:, 0].clamp(-15, 15))
    dp3 = g_rgb * ds
    dp2 = (dp3 @ wc2) * (p2 > 0)
    dp1 = (dp2 @ wc1) * (p1 > 0)
    dcin = dp1 @ wc0
    dh = torch.cat([(g_sigma * sigma_scale * eh0)[:, None], dcin[:, 16:31]], dim=1)
    dp0 = (dh @ ws1) * (p0 > 0)
    r.update(dp3=dp3, dp2=dp2, dp1=dp1, dcin=dcin, dh=dh, dp0=dp0)
    r.update(dwc2=dp3.t() @ a2, dwc1=dp2.t() @ a1, dwc0=dp1.t() @ cin, dws1=dh.t() @ a0, dws0=dp0.t() @ X,
             dX=dp0 @ ws0)
    # ---- magnitudes
    m0, m1, m2 = p0 > 0, p1 > 0, p2 > 0
    A0 = (X.abs() @ ws0.abs().t()) * m0
    H = A0 @ ws1.abs().t()
    Cin = torch.cat([sh.abs(), H[:, 1:16]], dim=1)
    A1 = (Cin @ wc0.abs().t()) * m1
    A2 = (A1 @ wc1.abs().t()) * m2
    P3 = A2 @ wc2.abs().t()
    e_h0 = 3 * U * H[:, 0]
    e_rgb = 6 * U * P3 / 4
    D3 = g_rgb.abs() * (ds + e_rgb)
    D2 = (D3 @ wc2.abs()) * m2
    D1 = (D2 @ wc1.abs()) * m1
    DH = torch.cat([(g_sigma.abs() * abs(sigma_scale) * eh0 * (1 + e_h0))[:, None], (D1 @ wc0.abs())[:, 16:31]], dim=1)
    D0 = (DH @ ws1.abs()) * m0
    mag = dict(dwc2=D3.t() @ A2, dwc1=D2.t() @ A1, dwc0=D1.t() @ Cin, dws1=DH.t() @ A0, dws0=D0.t() @ X.abs(),
               dX=D0 @ ws0.abs())
    bar = {k: 1e-4 * r[k].abs() + 6 * U * mag[k] + (1e-12 if k != "dX" else 0.0) for k in mag}
    bar["rgb"] = torch.full_like(s, 2e-5)
    bar["sigma"] = (1e-4 + e_h0) * r["sigma"]
    r.update(mag=mag, bar=bar, H0=H[:, 0])
    return r


def ratios(ref, got, base=None):
    """Worst err / bar of every output in `got` (a dict over OUTPUTS, any subset).  `base`: what the weight gradients were
    added to (overwrite == 0): the expected value is base + G and the bar grows by the fp32 rounding of that sum."""
    out = {}
    for k in [k for k in OUTPUTS if k in got]:
        v = got[k]
        want, bar = ref[k], ref["bar"][k]
        if base is not None and k in base:
            want = base[k].double() + want
            bar = bar + 2.0 ** -23 * want.abs()
        v = v.double()
        assert v.shape == want.shape, (k, tuple(v.shape), tuple(want.shape))
        err = (v - want).abs()
        inf = torch.full_like(err, float("inf"))
        # (a zero bar -- the all-zero row's dX -- asks for the exact value; anything not finite is over every bar)
        q = torch.where(bar > 0, err / bar.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), inf))
        out[k] = float(torch.where(torch.isfinite(v), q, inf).max()) if q.numel() else 0.0
    return out


def check(ref, got, what, base=None):
    """Prints the worst err / bar per output and asserts that none exceeds 1."""
    q = ratios(ref, got, base)
    print(f"err / bar [{what}]: " + "  ".join(f"{k} {v:.3f}" for k, v in q.items()))
    bad = {k: v for k, v in q.items() if not v <= 1.0}
    assert not bad, (what, bad)
    return q
