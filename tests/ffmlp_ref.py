"""fp64 reference, a-priori bars, interval comparator and exact nets for the fully fused MLP kernels (csrc/ffmlp.hip:
k_ffmlp_fwd, k_ffmlp_bwd_act; csrc/ffmlp_wgrad.hip: k_ffmlp_bwd_w, k_ffmlp_reduce_w; the recomputing entry points through
enerf_mlp32::ffmlp16_forward / ffmlp16_backward; csrc/ffnerf.hip: k_ffnerf_infer).  tests/test_ffmlp_ref.py holds this
module to autograd and to the C oracle on the host and shows that it rejects thirteen seeded defects;
tests/test_gpu_ffmlp_fp64.py holds the kernels to it on the device.

DEFINITION (float64; weight blob W0 [64,in] | hidden [64,64] x (NL-1) | Wout [16,64]; R16 = round to nearest even to
bf16 or fp16):
  forward    h_l = R16(act(W_l h_{l-1})),  y = R16(out_act(Wout h))
  backward   bb[0] = R16(act'(Wout^T dY ; fb[NL-1])),  bb[jj] = R16(act'(W_h[NL-1-jj]^T bb[jj-1] ; fb[NL-1-jj])),
             dX = R16(W0^T bb[NL-1])                                     (act' takes the POST-activation value)
  weights    dW_m = R16(gw_old + sum_s dOut_m[s] (x) In_m[s]),  dOut_m = bb[NL-1-m] (m < NL) or dY (m = NL),
             In_m = X (m = 0) or fb[m-1]

ERROR MODEL.  Products of two 16-bit values are exact in fp32.  An fp32 accumulation of K terms in any order, rounding or
truncating at every addition, is within
  gamma = K 2^-23 sum_k |w_k x_k| + K 2^-126
of the exact sum (unit 2^-23: nothing promises that the matrix unit's accumulator rounds to nearest; 2^-126: any partial
sum may be flushed when it is denormal).  For the weight gradient K is the longest chain of additions one element meets,
from the launch geometry (wgrad_chain).  gamma is derived, never tuned.
  interval rule: every activation is monotone, so for one layer with GIVEN inputs the stored value satisfies
  R16(act(z - gamma) - e) <= got <= R16(act(z + gamma) + e) at EVERY entry, z the fp64 sum; e is the evaluation error of
  the activation in fp32 (act_eval_err: relu / none 0; __expf, __logf and the fast division (2 + |x|) 2^-23 relative per
  call; squareplus and softplus by counting their roundings, as absolute bars because both cancel).
  propagation: for routes that expose no intermediate buffer [lo, hi] per unit is carried through the layers (positive
  and negative weight parts apart, +-gamma, act, R16 at both ends; through the ReLU mask of the backward a unit whose
  forward interval contains 0 contributes [min(0, g), max(0, g)]).  Sound but wider than the truth: `width_units` states
  the widths in units of rms(output) 2^-8 (bf16) or 2^-11 (fp16) so that a test can refuse a vacuous statement.
  exact nets: weights with 2-3 entries of +-1 per row, inputs and upstream gradients small integers -- every value of the
  forward and the backward is its own R16 in both types, and every partial sum of a weight gradient is an integer below
  2^24, so every summation order gives the same bits and the comparison is bit for bit on every route."""
import numpy as np

HID, OUT = 64, 16
U23 = 2.0 ** -23
ETA = 2.0 ** -126
KINDS = ("bf16", "fp16")
EPS16 = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
K_ACT = 10.0


# ------------------------------------------------------------------------------------------------------------- R16
def r16(x, kind, trunc=False):
    """float64 -> the nearest (ties to even) bf16 / fp16 value, as float64.  kind None: identity."""
    x = np.asarray(x, np.float64)
    if kind is None:
        return x.copy()
    if kind == "fp16":
        if trunc:
            with np.errstate(over="ignore"):
                r = x.astype(np.float16).astype(np.float64)
            over = np.abs(r) > np.abs(x)
            return np.where(over, np.nextafter(r.astype(np.float16), np.float16(0)).astype(np.float64), r)
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float64)
    assert kind == "bf16"
    a = np.abs(x)
    bits = a.view(np.uint64) if a.flags.c_contiguous else np.ascontiguousarray(a).view(np.uint64)
    drop = np.uint64(45)                                              # 52 - 7 mantissa bits
    if trunc:
        rb = bits & ~((np.uint64(1) << drop) - np.uint64(1))
    else:
        lsb = (bits >> drop) & np.uint64(1)
        rb = (bits + ((np.uint64(1) << np.uint64(44)) - np.uint64(1)) + lsb) & ~((np.uint64(1) << drop) - np.uint64(1))
    r = rb.view(np.float64).reshape(a.shape)
    q = 2.0 ** -133                                                   # below 2^-126 bf16 is a fixed-point grid
    small = a < 2.0 ** -126
    r = np.where(small, (np.floor(a / q) if trunc else np.rint(a / q)) * q, r)
    r = np.where(r > 3.3895313892515355e38, np.inf, r)
    r = np.where(np.isnan(x), np.nan, r)
    return np.copysign(r, x)


def ulp16(x, kind):
    """spacing of the 16-bit grid at |x| (float64)"""
    a = np.abs(np.asarray(x, np.float64))
    mant, emin = (7, -126) if kind == "bf16" else (10, -14)
    e = np.floor(np.log2(np.maximum(a, 2.0 ** emin)))
    return 2.0 ** (e - mant)


# ------------------------------------------------------------------------------------------------------ activations
def act_fwd(x, a):
    x = np.asarray(x, np.float64)
    if a == 0:
        return np.maximum(x, 0.0)
    if a == 1:
        return np.exp(x)
    if a == 3:
        return 1.0 / (1.0 + np.exp(-x))
    if a == 4:
        v = x * K_ACT
        return 0.5 * (v + np.sqrt(v * v + 4.0)) / K_ACT
    if a == 5:
        return np.logaddexp(x * K_ACT, 0.0) / K_ACT
    assert a == 6
    return x.copy()


def act_eval_err(x, a):
    """absolute bound of the fp32 evaluation error of act_fwd at x (ffmlp_common.h: act_fwd)"""
    x = np.asarray(x, np.float64)
    if a in (0, 6):
        return np.zeros_like(x)
    y = act_fwd(x, a)
    if a == 1:                                       # one __expf
        return (2 + np.abs(x)) * U23 * y
    if a == 3:                                       # __expf, the addition, the fast division
        e = np.exp(-x)
        return y * U23 * ((2 + np.abs(x)) * e / (1 + e) + 1 + 2)
    if a == 4:
        # v = 10 x (1), v v (1), + 4 (1), sqrt (<= 2), v + s (1): absolute (|v| + 4 s) u on the sum, which cancels for
        # v < 0; the division by 10 (fast: 2) and the slack of the count: 4 u relative
        v = x * K_ACT
        s = np.sqrt(v * v + 4.0)
        return U23 * (5 * (np.abs(v) + s) / (2 * K_ACT) + 4 * y)
    # softplus: a = e^v + 1 carries relative (e^v / a)(2 + |v|) u + u; log turns it into an absolute error; __logf itself
    # 2 u relative on its result, the product 10 x one more on v (folded into 2 + |v|), the division by 10 2 u
    v = x * K_ACT
    ev_a = 1.0 / (1.0 + np.exp(-v))                  # e^v / (e^v + 1)
    L = y * K_ACT
    return U23 * ((ev_a * (3 + np.abs(v)) + 1) + 4 * L) / K_ACT


def act_bwd_factor(fwd, a):
    """act'(.) as the factor f(fwd) of ffmlp_common.h: act_bwd, with (relative, absolute) bounds of its fp32 evaluation"""
    fwd = np.asarray(fwd, np.float64)
    z = np.zeros_like(fwd)
    if a == 0:
        return (fwd > 0).astype(np.float64), z, z
    if a == 6:
        return np.ones_like(fwd), z, z
    if a == 1:
        return fwd.copy(), z, z
    if a == 3:
        return fwd * (1 - fwd), z + 3 * U23, z
    if a == 4:
        y = fwd * K_ACT
        return y * y / (y * y + 1), z + 12 * U23, z
    assert a == 5
    e = np.exp(-fwd * K_ACT)
    return 1 - e, z + U23, e * (3 + K_ACT * np.abs(fwd)) * U23


# ------------------------------------------------------------------------------------------------------- the reference
def blob_size(in_dim, NL):
    return HID * (in_dim + HID * (NL - 1) + OUT)


def split(W, in_dim, NL):
    """flat blob -> [W0 [64,in], hidden [64,64] x (NL-1), Wout [16,64]] (views)"""
    W = np.asarray(W)
    assert W.size == blob_size(in_dim, NL)
    mats, off = [W[:HID * in_dim].reshape(HID, in_dim)], HID * in_dim
    for _ in range(NL - 1):
        mats.append(W[off:off + HID * HID].reshape(HID, HID))
        off += HID * HID
    mats.append(W[off:].reshape(OUT, HID))
    return mats


def forward(x, W, in_dim, NL, act=0, out_act=6, kind="bf16"):
    """-> y [B,16], fb [NL,B,64]"""
    m = split(np.asarray(W, np.float64), in_dim, NL)
    h = np.asarray(x, np.float64)
    fb = []
    for l in range(NL):
        h = r16(act_fwd(h @ m[l].T, act), kind)
        fb.append(h)
    return r16(act_fwd(h @ m[NL].T, out_act), kind), np.stack(fb)


def backward(dy, x, W, fb, in_dim, NL, act=0, kind="bf16", gw_old=None, want_dx=True):
    """-> dX [B,in] (or None), dW (flat), bb [NL,B,64]"""
    m = split(np.asarray(W, np.float64), in_dim, NL)
    dy, x, fb = np.asarray(dy, np.float64), np.asarray(x, np.float64), np.asarray(fb, np.float64)
    bb = []
    g = dy
    for jj in range(NL):
        wt = m[NL] if jj == 0 else m[NL - jj]
        g = r16((g @ wt) * act_bwd_factor(fb[NL - 1 - jj], act)[0], kind)
        bb.append(g)
    bb = np.stack(bb)
    dx = r16(g @ m[0], kind) if want_dx else None
    sums = weight_sums(dy, x, fb, bb, NL)
    old = np.zeros_like(sums) if gw_old is None else np.asarray(gw_old, np.float64).ravel()
    return dx, r16(old + sums, kind), bb


def wgrad_operands(dy, x, fb, bb, NL, m):
    """(dOut_m, In_m) of matmul m"""
    return (bb[NL - 1 - m] if m < NL else dy), (x if m == 0 else fb[m - 1])


def weight_sums(dy, x, fb, bb, NL, absolute=False):
    f = np.abs if absolute else (lambda a: a)
    return np.concatenate([(f(d).T @ f(i)).ravel() for d, i in (wgrad_operands(dy, x, fb, bb, NL, m) for m in range(NL + 1))])


# ------------------------------------------------------------------------------------------------------------ geometry
def div_up(a, b):
    return -(-a // b)


def fwd_geometry(B):
    """k_ffmlp_fwd: (workgroups, waves, trips of the busiest wave, trips of the idlest) over 64-sample pairs"""
    blocks = min(div_up(B // 64, 4), 512)
    nw, pairs = 4 * blocks, B // 64
    return blocks, nw, div_up(pairs, nw), pairs // nw


def bwd_geometry(B, cap=512):
    """k_ffmlp_bwd_act (cap 512) / k_ffmlp_bwd_w (cap 256) over 32-sample tiles"""
    blocks = min(div_up(B // 32, 4), cap)
    nw, tiles = 4 * blocks, B // 32
    return blocks, nw, div_up(tiles, nw), tiles // nw


def ffnerf_geometry(M):
    """k_ffnerf_infer over groups of two 32-sample tiles"""
    tiles = div_up(M, 32)
    groups = div_up(tiles, 2)
    blocks = min(div_up(groups, 4), 512)
    nw = 4 * blocks
    return blocks, nw, div_up(groups, nw), groups // nw, tiles


def recompute_geometry(B):
    """mlp32.hip's pgrid for the recomputing route: forward cap 512 workgroups, fused backward cap 256, 32-row tiles"""
    tiles = div_up(B, 32)
    out = []
    for cap in (512, 256):
        blocks = min(div_up(tiles, 4), cap)
        out.append((blocks, 4 * blocks, div_up(tiles, 4 * blocks), tiles // (4 * blocks)))
    return out


def wgrad_chain(B):
    """longest chain of fp32 additions one weight-gradient element meets, mirroring ffmlp_wgrad_launch: a wave's 32 samples
    per tile x its tiles, four wave turns in LDS, the reduce's strided chain, the 16 wave sums, and gw_old."""
    nblocks = bwd_geometry(B, 256)[0]
    per_wave = bwd_geometry(B, 256)[2]
    return 32 * per_wave + 4 + (div_up(nblocks, 64) + 2) + 16 + 1


def wgrad_chain_any_order(B):
    """the recomputing route sums in its own order (mlp32s.hip); B products, at most 256 x 4 partial sums and the final
    ones cannot meet more additions than there are terms and partial results, whatever the order"""
    return B + 4 * recompute_geometry(B)[1][0] + 64


def gamma(K, abs_sum):
    return K * U23 * abs_sum + K * ETA


# ---------------------------------------------------------------------------------------------------------- comparator
class Worst:
    """collects, per tensor, the worst |got - centre| / half-width of the 16-bit intervals (0: the only value of a
    one-value interval; 1: an end of a two-value one; above 1: outside), the failures, and -- where the bounds before R16
    are given -- the worst (|got - centre| - half a 16-bit ulp) / half-width before the rounding (`used`): the share of
    gamma (and of the activation's evaluation bar) that the result can be shown to have used"""

    def __init__(self):
        self.ratio, self.err, self.fails, self.kind = {}, {}, [], "bf16"

    def interval(self, name, got, lo, hi, plo=None, phi=None):
        got = np.asarray(got, np.float64)
        assert got.shape == lo.shape == hi.shape, (name, got.shape, lo.shape)
        if plo is not None:
            h = 0.5 * (phi - plo)
            use = np.isfinite(got) & (h > 0) & (plo != 0) & (phi != 0)          # (not where ReLU clips an end to 0)
            e = np.maximum(np.abs(got - 0.5 * (plo + phi)) - 0.5 * ulp16(got, self.kind), 0.0)[use] / h[use]
            self.err[name] = max(self.err.get(name, 0.0), float(e.max()) if e.size else 0.0)
        ok = (got >= lo) & (got <= hi)
        c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(h > 0, np.abs(got - c) / h, np.where(got == c, 0.0, np.inf))
        r = np.where(np.isnan(r), np.inf, r)
        worst = float(r.max()) if r.size else 0.0
        self.ratio[name] = max(self.ratio.get(name, 0.0), worst)
        if not ok.all():
            k = np.unravel_index(int(np.argmax(~ok)), ok.shape)
            self.fails.append(f"{name}: {int((~ok).sum())} of {ok.size} outside, first at {k}: got {got[k]!r}, "
                              f"interval [{lo[k]!r}, {hi[k]!r}]")
        return bool(ok.all())

    def exact(self, name, got, want):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
        self.ratio[name] = max(self.ratio.get(name, 0.0), float("inf") if bad.any() else 0.0)
        if bad.any():
            k = np.unravel_index(int(np.argmax(bad)), bad.shape)
            self.fails.append(f"{name}: {int(bad.sum())} of {bad.size} differ, first at {k}: got {got[k]!r}, want {want[k]!r}")
        return not bad.any()

    def report(self, title):
        return title + ": " + ", ".join(f"{k} {v:.3g}" + (f" (used {self.err[k]:.3f})" if k in self.err else "")
                                        for k, v in self.ratio.items())


def layer_interval(inp, Wm, K, act, kind):
    """the interval rule for h = R16(act(inp Wm^T)) with given 16-bit inputs -> (lo, hi, the same before R16)"""
    inp, Wm = np.asarray(inp, np.float64), np.asarray(Wm, np.float64)
    z, A = inp @ Wm.T, np.abs(inp) @ np.abs(Wm).T
    g = gamma(K, A)
    lo = act_fwd(z - g, act) - act_eval_err(z - g, act)
    hi = act_fwd(z + g, act) + act_eval_err(z + g, act)
    return r16(lo, kind), r16(hi, kind), lo, hi


def grad_interval(gin, WmT, fwd, K, act, kind):
    """the interval rule for bb = R16(act'(gin WmT ; fwd)), WmT [k, n] the matrix as it multiplies gin [B, k]"""
    gin, WmT = np.asarray(gin, np.float64), np.asarray(WmT, np.float64)
    z, A = gin @ WmT, np.abs(gin) @ np.abs(WmT)
    g = gamma(K, A)
    if fwd is None:
        return r16(z - g, kind), r16(z + g, kind), z - g, z + g
    f, rel, ab = act_bwd_factor(fwd, act)
    e = f * rel + ab
    c = np.stack([(z - g) * (f - e), (z - g) * (f + e), (z + g) * (f - e), (z + g) * (f + e)])
    lo, hi = c.min(0), c.max(0)
    if act not in (0, 6):                                   # the product with g rounds once more
        lo, hi = lo - U23 * np.abs(lo), hi + U23 * np.abs(hi)
    return r16(lo, kind), r16(hi, kind), lo, hi


def wgrad_interval(dy, x, fb, bb, NL, K, kind, gw_old=None):
    s, A = weight_sums(dy, x, fb, bb, NL), weight_sums(dy, x, fb, bb, NL, absolute=True)
    old = np.zeros_like(s) if gw_old is None else np.asarray(gw_old, np.float64).ravel()
    g = gamma(K, A + np.abs(old))
    return r16(old + s - g, kind), r16(old + s + g, kind), old + s - g, old + s + g


def check_forward_layers(W_, x, Wb, in_dim, NL, act, out_act, kind, fb, y, tag=""):
    """forward_buffer[l] against the route's OWN forward_buffer[l-1], outputs against its own last layer"""
    m = split(np.asarray(Wb, np.float64), in_dim, NL)
    W_.kind = kind
    prev = np.asarray(x, np.float64)
    for l in range(NL):
        W_.interval(f"{tag}fb[{l}]", fb[l], *layer_interval(prev, m[l], prev.shape[1], act, kind))
        prev = np.asarray(fb[l], np.float64)
    W_.interval(f"{tag}y", y, *layer_interval(prev, m[NL], HID, out_act, kind))


def check_backward_layers(W_, dy, x, Wb, fb, in_dim, NL, act, kind, bb, dx, gw, K_w, gw_old=None, tag=""):
    """each backward_buffer slot against the route's own previous slot, grad_inputs from the last slot, grad_weights from
    the buffers as given"""
    m = split(np.asarray(Wb, np.float64), in_dim, NL)
    W_.kind = kind
    g = np.asarray(dy, np.float64)
    for jj in range(NL):
        wt, K = (m[NL], OUT) if jj == 0 else (m[NL - jj], HID)
        W_.interval(f"{tag}bb[{jj}]", bb[jj], *grad_interval(g, wt, fb[NL - 1 - jj], K, act, kind))
        g = np.asarray(bb[jj], np.float64)
    if dx is not None:
        W_.interval(f"{tag}dX", dx, *grad_interval(g, m[0], None, HID, act, kind))
    if gw is not None:
        W_.interval(f"{tag}dW", np.asarray(gw).ravel(), *wgrad_interval(dy, x, fb, bb, NL, K_w, kind, gw_old))


# --------------------------------------------------------------------------------------------------------- propagation
def _imatmul(lo, hi, Wt):
    """[lo, hi] @ Wt (Wt [k, n]) -> (lo, hi, bound of sum |terms|)"""
    p, n = np.maximum(Wt, 0), np.minimum(Wt, 0)
    return lo @ p + hi @ n, hi @ p + lo @ n, np.maximum(np.abs(lo), np.abs(hi)) @ np.abs(Wt)


def _ilayer(lo, hi, Wm, K, act, kind):
    zl, zh, A = _imatmul(lo, hi, np.asarray(Wm, np.float64).T)
    g = gamma(K, A)
    return (r16(act_fwd(zl - g, act) - act_eval_err(zl - g, act), kind),
            r16(act_fwd(zh + g, act) + act_eval_err(zh + g, act), kind))


def propagate_forward(xlo, xhi, W, in_dim, NL, act, out_act, kind):
    """-> (ylo, yhi), [(lo, hi) of every hidden layer]"""
    m = split(np.asarray(W, np.float64), in_dim, NL)
    lo, hi = np.asarray(xlo, np.float64), np.asarray(xhi, np.float64)
    layers = []
    for l in range(NL):
        lo, hi = _ilayer(lo, hi, m[l], m[l].shape[1], act, kind)
        layers.append((lo, hi))
    return _ilayer(lo, hi, m[NL], HID, out_act, kind), layers


def _imask(glo, ghi, flo, fhi, act):
    if act == 6:
        return glo, ghi
    assert act == 0, "propagation through the backward: relu or none"
    on, off = flo > 0, fhi <= 0
    lo = np.where(on, glo, np.where(off, 0.0, np.minimum(glo, 0.0)))
    hi = np.where(on, ghi, np.where(off, 0.0, np.maximum(ghi, 0.0)))
    return lo, hi


def _iprod_sum(al, ah, bl, bh, chunk=64):
    """sum_s [al, ah][s, o] * [bl, bh][s, i] -> (lo, hi, bound of sum |terms|), [o, i]"""
    lo = np.zeros((al.shape[1], bl.shape[1]))
    hi, A = lo.copy(), lo.copy()
    for s in range(0, al.shape[0], chunk):
        a0, a1 = al[s:s + chunk, :, None], ah[s:s + chunk, :, None]
        b0, b1 = bl[s:s + chunk, None, :], bh[s:s + chunk, None, :]
        c = np.stack([a0 * b0, a0 * b1, a1 * b0, a1 * b1])
        lo += c.min(0).sum(0)
        hi += c.max(0).sum(0)
        A += np.abs(c).max(0).sum(0)
    return lo, hi, A


def propagate_backward(dy, x, W, layers, in_dim, NL, act, kind, K_w, want_dx=True):
    """the recomputing route end to end: -> (dXlo, dXhi) or None, (dWlo, dWhi) flat"""
    m = split(np.asarray(W, np.float64), in_dim, NL)
    dy, x = np.asarray(dy, np.float64), np.asarray(x, np.float64)
    gl, gh = dy, dy
    gs = []
    for jj in range(NL):
        wt, K = (m[NL], OUT) if jj == 0 else (m[NL - jj], HID)
        zl, zh, A = _imatmul(gl, gh, wt)
        g = gamma(K, A)
        gl, gh = _imask(zl - g, zh + g, *layers[NL - 1 - jj], act)
        gl, gh = r16(gl, kind), r16(gh, kind)
        gs.append((gl, gh))
    dX = None
    if want_dx:
        zl, zh, A = _imatmul(gl, gh, m[0])
        g = gamma(HID, A)
        dX = (r16(zl - g, kind), r16(zh + g, kind))
    lo, hi = [], []
    for mm in range(NL + 1):
        d = gs[NL - 1 - mm] if mm < NL else (dy, dy)
        i = (x, x) if mm == 0 else layers[mm - 1]
        l, h, A = _iprod_sum(d[0], d[1], i[0], i[1])
        g = gamma(K_w, A)
        lo.append(r16(l - g, kind).ravel())
        hi.append(r16(h + g, kind).ravel())
    return dX, (np.concatenate(lo), np.concatenate(hi))


def width_units(lo, hi, kind, scale=None):
    """interval widths in units of rms(output) 2^-8 (bf16) / 2^-11 (fp16)"""
    c = 0.5 * (lo + hi)
    rms = float(np.sqrt(np.mean(c * c))) if scale is None else scale
    return (hi - lo) / (rms * EPS16[kind])


def width_stats(lo, hi, kind):
    w = width_units(lo, hi, kind)
    return dict(max=float(w.max()), q99=float(np.quantile(w, 0.99)), median=float(np.median(w)))


# ----------------------------------------------------------------------------------- the fused network of network_ff.py
SIGMA_W, COLOR_W = blob_size(32, 2), blob_size(32, 3)


def _sh_norm():
    from math import pi, sqrt
    n = np.zeros((4, 4))
    for l in range(4):
        for m in range(l + 1):
            ratio = 1.0
            for k in range(l - m + 1, l + m + 1):
                ratio /= k
            v = sqrt((2.0 * l + 1.0) / (4.0 * pi) * ratio)
            n[l, m] = np.float32(v * sqrt(2.0) if m else v)           # the kernel holds the norms in fp32
    return n


def sh4(d):
    """the 16 real spherical harmonics of sh_basis.h in float64 -> (Y [M,16], magnitude bound [M,16]): the bound runs the
    same recurrences on absolute values, which is what the fp32 roundings are relative to (the recurrences cancel)"""
    d = np.asarray(d, np.float64)
    n = _sh_norm()
    out = []
    for absolute in (False, True):
        x, y, z = (np.abs(d[:, k]) if absolute else d[:, k] for k in range(3))
        sgn = 1.0 if absolute else -1.0
        A, Bm = [np.ones_like(x)], [np.zeros_like(x)]
        for m in range(1, 4):
            A.append(x * A[m - 1] + sgn * y * Bm[m - 1])
            Bm.append(x * Bm[m - 1] + y * A[m - 1])
        Y = np.zeros((d.shape[0], 16))
        for m in range(4):
            qmm = 1.0
            for k in range(1, m + 1):
                qmm *= (2.0 * k - 1.0) if absolute else -(2.0 * k - 1.0)
            Q = {m: qmm * np.ones_like(x)}
            if m + 1 < 4:
                Q[m + 1] = (2.0 * m + 1.0) * z * qmm
            for l in range(m + 2, 4):
                Q[l] = ((2.0 * l - 1.0) * z * Q[l - 1] + sgn * (l + m - 1) * Q[l - 2]) * (1.0 / (l - m))
            for l in range(m, 4):
                nq = n[l, m] * Q[l]
                Y[:, l * l + l + m] = nq * A[m]
                if m:
                    Y[:, l * l + l - m] = nq * Bm[m]
        out.append(Y)
    return out[0], out[1]


def feats_rows(feats_lm, M):
    """level-major [16, Mp, 2] -> row-major [M, 32]"""
    return np.ascontiguousarray(np.transpose(np.asarray(feats_lm, np.float64), (1, 0, 2)).reshape(-1, 32)[:M])


def ffnerf_intervals(feats_lm, dirs, Ws, Wc, M, kind, sh_ulps=4.0, exact_sigma=False):
    """k_ffnerf_infer end to end -> dict(sigma=(lo, hi), rgb=(lo, hi), raw_s=..., raw_c=...).  The 16 SH inputs are held by
    the interval of R16 around the fp64 basis widened by `sh_ulps` fp32 ulp of the recurrences' magnitude.  exact_sigma: the
    sigma net is an exact net (asserted), its outputs single values."""
    x = r16(feats_rows(feats_lm, M), kind)
    Ws, Wc = r16(Ws, kind), r16(Wc, kind)
    if exact_sigma:
        slo, fbs = forward(x, Ws, 32, 2, 0, 6, None)
        assert _is_exact(slo) and _is_exact(fbs) and _is_exact(Ws) and np.array_equal(x, feats_rows(feats_lm, M))
        shi = slo
    else:
        (slo, shi), _ = propagate_forward(x, x, Ws, 32, 2, 0, 6, kind)
    Y, Ymag = sh4(np.asarray(dirs, np.float64)[:M])
    e = sh_ulps * U23 * Ymag
    zero = np.zeros((M, 1))
    clo = np.concatenate([r16(Y - e, kind), slo[:, 1:], zero], 1)
    chi = np.concatenate([r16(Y + e, kind), shi[:, 1:], zero], 1)
    (rlo, rhi), _ = propagate_forward(clo, chi, Wc, 32, 3, 0, 6, kind)
    rlo, rhi = rlo[:, :3], rhi[:, :3]

    def through(f, lo, hi, a):
        return r16(f(lo) - act_eval_err(lo, a), kind), r16(f(hi) + act_eval_err(hi, a), kind)
    return dict(sigma=through(np.exp, slo[:, 0], shi[:, 0], 1), rgb=through(lambda v: act_fwd(v, 3), rlo, rhi, 3),
                raw_s=(slo, shi), raw_c=(rlo, rhi))


# ---------------------------------------------------------------------------------------------------------- exact nets
def _sparse_rows(rng, rows, cols):
    Wm = np.zeros((rows, cols))
    for r in range(rows):
        k = int(rng.integers(2, 4))
        c = rng.choice(cols, size=k, replace=False)
        Wm[r, c] = rng.choice([-1.0, 1.0], size=k)
    return Wm


def _is_exact(a):
    a = np.asarray(a, np.float64)
    return bool(np.all(np.abs(a) < 2.0 ** 24) and all(np.array_equal(r16(a, k), a) for k in KINDS))


def exact_net(NL, in_dim, B, seed, act=0, dy_scale=1.0, dy_rows=None, tries=200):
    """A net whose every value is exactly representable in bf16 AND fp16: weights with 2-3 entries of +-1 per row at seeded
    random columns, inputs and upstream gradients integers in [-2, 2] (dY times `dy_scale`, a power of two; `dy_rows`: only
    these rows of dY are non-zero).  Asserts that every value of the forward and of the backward is its own R16 in both
    types, that every layer keeps >= 15 % non-zero activations and >= 5 distinct values, and that sum |terms| of every
    weight-gradient element is below 2^24 -- its partial sums are then integers (times dy_scale) that fp32 holds exactly in
    any order, so that R16 of the exact total is the only rounding (`gw` of the result states it per type)."""
    for t in range(tries):
        rng = np.random.default_rng(seed + 7919 * t)
        W = np.concatenate([_sparse_rows(rng, HID, in_dim).ravel()] +
                           [_sparse_rows(rng, HID, HID).ravel() for _ in range(NL - 1)] +
                           [_sparse_rows(rng, OUT, HID).ravel()])
        x = rng.integers(-2, 3, (B, in_dim)).astype(np.float64)
        dy = rng.integers(-2, 3, (B, OUT)).astype(np.float64) * dy_scale
        if dy_rows is not None:
            keep = np.zeros((B, 1))
            keep[np.asarray(dy_rows)] = 1.0
            dy = dy * keep
        y, fb = forward(x, W, in_dim, NL, act, 6, None)
        dx, _, bb = backward(dy, x, W, fb, in_dim, NL, act, None)
        live = all((f != 0).mean() >= 0.15 and np.unique(f).size >= 5 for f in fb)
        if live and all(_is_exact(a) for a in (y, fb, bb, dx)):
            break
    else:
        raise AssertionError(f"no exact net for NL={NL} in={in_dim} B={B} seed={seed}")
    for name, a in (("y", y), ("fb", fb), ("bb", bb), ("dX", dx), ("W", W), ("x", x), ("dY", dy)):
        assert _is_exact(a), name
    assert live
    for l, f in enumerate(fb):
        assert (f != 0).mean() >= 0.15 and np.unique(f).size >= 5, l
    sums = weight_sums(dy, x, fb, bb, NL)
    top = weight_sums(dy, x, fb, bb, NL, absolute=True)
    assert float(top.max()) / dy_scale < 2.0 ** 24 and np.array_equal(sums / dy_scale, np.rint(sums / dy_scale))
    return dict(NL=NL, in_dim=in_dim, B=B, act=act, W=W, x=x, dy=dy, y=y, fb=fb, bb=bb, dx=dx, sums=sums, sums_abs=top,
                dy_scale=dy_scale)


def exact_gw(net, kind, gw_old=None):
    """grad_weights of an exact net: the one rounding of the exact total"""
    old = 0.0 if gw_old is None else np.asarray(gw_old, np.float64).ravel()
    assert float((net["sums_abs"] + np.abs(old)).max()) / net["dy_scale"] < 2.0 ** 24
    return r16(old + net["sums"], kind)


def exact_ffnerf(M, seed, tries=200):
    """exact sigma and colour nets with integer features in level-major layout and unit directions; the colour net's
    inputs are the (inexact) SH basis and the sigma net's outputs, so its results are held by ffnerf_intervals, whose
    intervals are single values or two neighbours for such weights"""
    Mp = (M + 31) // 32 * 32
    for t in range(tries):
        rng = np.random.default_rng(seed + 7919 * t)
        Ws = np.concatenate([_sparse_rows(rng, HID, 32).ravel(), _sparse_rows(rng, HID, HID).ravel(),
                             _sparse_rows(rng, OUT, HID).ravel()])
        Wc = np.concatenate([_sparse_rows(rng, HID, 32).ravel(), _sparse_rows(rng, HID, HID).ravel(),
                             _sparse_rows(rng, HID, HID).ravel(), _sparse_rows(rng, OUT, HID).ravel()])
        # sigma_raw small (exp of it is stored in 16 bits), geo features alive
        feats = np.zeros((16, Mp, 2))
        feats[:, :M] = rng.integers(-2, 3, (16, M, 2))
        d = rng.normal(size=(M, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        d = d.astype(np.float32).astype(np.float64)
        y, fb = forward(feats_rows(feats, M), Ws, 32, 2, 0, 6, None)
        if not all(_is_exact(a) for a in (y, fb)) or np.abs(y[:, 0]).max() > 8:
            continue
        if M >= 31 and ((y[:, 1:] != 0).mean() < 0.15 or np.unique(y[:, 0]).size < 3):
            continue
        return dict(M=M, Mp=Mp, Ws=Ws, Wc=Wc, feats=feats, dirs=d)
    raise AssertionError(f"no exact fused net for M={M} seed={seed}")
