"""fp64 reference, synthetic inputs, a-priori error bars and the comparator for the marching route's compositing kernels
(csrc/raymarching.hip: k_composite_train_fwd, k_composite_train_bwd, k_composite_train_fwd_bwd_mse with both tails,
k_composite_rays, k_composite_rays_frame).  tests/test_composite_ref.py holds this module to autograd, to the C oracle and
to a numpy fp32 statement of the kernels' scan order (kernel_statement below, with seeded defects) on the host;
tests/test_gpu_composite_fp64.py holds the kernels to it on the device.

The reference states the DEFINITION in float64 from the fp32 values the kernel is given (reference_ray):
  alpha_k = -expm1(-sigma_k delta_k0),  Tpre_k = prod_{j<k} (1 - alpha_j),  Tpost_k = Tpre_{k+1},  w_k = alpha_k Tpre_k,
  weights_sum = sum w,  image_c = sum w_k rgb_kc,  t_k = cumsum(delta_k1),  depth = sum w_k t_k,
  out = image + (1 - weights_sum) bg,  d rgb_kc = g_c w_k,
  d sigma_k = delta_k0 (sum_c g_c (Tpost_k rgb_kc - sum_{j>k} w_j rgb_jc) + g_ws (Tpost_k - sum_{j>k} w_j)),
the suffix sums taken by reverse cumulative sums, never as `final - running`.  A ray with count == 0 or
offset + count >= M outputs zeros and out == bg; in the MSE and frame forms its gradient rows inside the buffer and all
rows of [counter, M) are zero.  For those forms the upstream gradient is formed in fp64 from the out_image the kernel
itself wrote (checked on its own): g = (out - target) scale, g_ws = -(g . bg); the frame tail's target is
gt = pixels, or pixels[:C] a + bg (1 - a), and the term's weight multiplies the finished gradients.

Error model (u = 2^-24, the fp32 unit roundoff; eta = 2^-126: every rounding may also flush a denormal; k = the sample's
index on its ray, from 0).  Every constant is a count of roundings of the statements; none is taken from a kernel's
observed error.  The same bars hold the sequential fp32 oracle (k roundings in T_k) and the kernels' scan order (fewer).
  alpha = 1 - __expf(-sigma delta0).  The argument is rounded three times before the hardware sees it (the product, the
    log2(e) constant, the product with it): relative 3u on x = sigma delta0, so relative 3u x on e = exp(-x); v_exp_f32 is
    good to one ulp, relative 2u; `1 - e` rounds once, u alpha.  |d alpha_k| <= da_k = u (3 x e + 2 e + alpha), ABSOLUTE:
    x e <= 1/e keeps the term that grows with the argument bounded, da <= 4.2 u (expf: the same with smaller constants).
    1 - alpha itself is exact (alpha is a multiple of 2^-24 below 1/2 and Sterbenz above).
  Tpre_k: E_T[0] = 0;  E' = E_T[k] (1 - alpha_k + da_k) + Tpre_k da_k;  E_T[k+1] = E' + u (Tpost_k + E') + eta.
    Unrolled: sum_j da_j T/(1 - alpha_j) + k u T_k -- linear in k.  A product tree of the same factors has the same
    first-order terms and at most as many roundings on any path, so the bound does not depend on the association.  An
    opaque sample (1 - alpha ~ u) leaves an ABSOLUTE error Tpre da behind it, however large that is relative to Tpost.
  w_k = alpha_k Tpre_k:  E' = (alpha_k + da_k) E_T[k] + Tpre_k da_k;  E_w[k] = E' + u (w_k + E') + eta.
  sums (weights_sum, image_c, depth; every term >= 0): s_k = sum_{j<=k} a_j with |d a_j| <= E_a[j].  Sequentially every
    addition rounds its own partial sum: u sum_{j<=k} s_j.  In the scan a lane's value passes six additions inside its
    chunk, none larger than s_k, and one addition of the carry per chunk, each a partial sum s_j at a chunk end: u (6 s_k
    + sum_j s_j) at the most.  A separately rounded product w rgb or w t adds u s_k.  So
    E_s[k] = sum_{j<=k} E_a[j] + u (sum_{j<=k} s^_j + 7 s^_k), s^ the sums of the terms plus their bars: on the ray's own
    scale.  t_k = cumsum(delta1) carries k roundings: E_t[k] = k u t_k, inside depth's terms.
  out = image + (1 - ws) bg:  E_image + |bg| (E_ws + u |1 - ws|^) + u |bg| |1 - ws|^ + u |out|^   (^: value plus its bar).
  d sigma_k: A_c = Tpost_k rgb_kc - R_c, R_c = F_c - I_kc computed as final minus running, both sums with their bars:
    E_A = E_T[k+1] rgb + u Tpost^ rgb + (2 E_image_c + u R^_c) + u |A|^;  B = Tpost_k - (ws - ws_k) likewise.  Then one
    product per term, C additions and the product with delta0: (C + 2) u on sum |terms|.  With the upstream gradient's own
    bars dg_c, dg_ws (zero when it is given in fp32):
    E_dsigma[k] = delta_k0 (sum_c (|g_c| E_A_c + dg_c |A_c|^) + |g_ws| E_B + dg_ws |B|^ + (C + 2) u sum |terms|^) + eta.
    This is an absolute bar on delta_k0 Q, Q = max_k (sum_c |g_c| (rgb_kc + |image_c|) + |g_ws|): |A_c| <= rgb_kc +
    image_c and |B| <= 1, the factors of u are the ray's E_T, E_image and E_ws.  It is NOT relative to d sigma_k, which
    cancels.
  d rgb_kc = g_c w_k:  |g_c| E_w[k] + dg_c w^_k + u |g_c| w^_k + eta.
  fused forms: g_c = fl(fl(out_c - target_c) scale): dg_c = 2 u |g_c|; g_ws = -(g . bg): dg_ws = sum |bg_c| dg_c +
    C u sum |g_c bg_c|.  Frame tail: gt with alpha has four roundings, E_gt = u (|p a| + 2 |bg (1 - a)| + |gt|), and
    dg_c = scale (E_gt + u |out - gt|) + u |g_c|.  The weight multiplies the finished gradients: weight E + u |weight x|,
    and -- what an absolute bar cannot see -- a weighted call's gradients are fl(weight * the unweighted call's), ONE
    rounding: bar u |weight x_1| + eta against the same call at weight 1 (weight_reference).  Folded into g the
    rounding passes the cancelling sum and lands tens of ulp away.
  inference (composite_rays, composite_rays_frame: sequential, T = 1 - weight_sum): with dS the error of the running
    weight_sum, dS' = dS (1 - alpha^) + alpha^ rho + T d alpha + roundings, rho <= u T^ the rounding of 1 - S:
    E_S' = E_S (1 - alpha + da) + (alpha + da) u T^ + T da + u (w^ + S'^) + eta -- contracting; E_T = E_S + u T^,
    E_w as above from E_T; depth and colours are fma chains: E' = E + E_w v + w^ E_v + u |new value|^.  The frame
    epilogue: depth = max(d - near, 0) / (far - near): (E_d + u |d - near|) / (far - near) + 2 u depth.
    The stop is an fp32 comparison T < 1e-5: a ray whose fp64 T comes within max(1e-8, E_T) of 1e-5 at any step is
    dropped from the comparison (infer_case keeps the share of such rays at or below 1 %).
Rows a kernel must zero or must not touch are compared exactly (bar 0; untouched: the NaN sentinel)."""
import functools

import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -126
F32 = np.float32
W03 = float(F32(0.3))

FAMILIES = ["RAND", "THIN", "WALL", "SAT_LATE", "ZERO", "ONE_HOT"]
EMPTY, DROPPED = "EMPTY", "DROPPED"
COUNTS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 200, 1023, 1024]
NS = [1, 3, 4, 5, 15, 16, 17, 33]
N_CASES = 16                                   # two rounds of NS: 162 live rays, every (family, count) pair at least once
BG_FORMS = ["scalar", "shared", "ray"]
SEED = 20240611


def _slot(s):
    """(family, count) of the s-th live ray over all cases: s = 0 .. 119 walks every pair exactly once."""
    f = s % 6
    return FAMILIES[f], COUNTS[(s // 6 + 3 * f) % len(COUNTS)]


def _live_slots(N):
    return N - (1 if N >= 3 else 0) - (1 if N >= 4 else 0)


def make_samples(fam, n, rng):
    """-> sigma [n], delta [n, 2] in fp32.  delta in [1e-3, 2e-2], delta_1 drawn on its own."""
    d = rng.uniform(1e-3, 2e-2, (n, 2)).astype(F32)
    d0 = d[:, 0].astype(np.float64)
    s = np.zeros(n)
    if fam == "RAND":
        s = rng.uniform(0.0, 25.0, n)
        s[rng.random(n) < 0.1] = 0.0
    elif fam in ("THIN", "SAT_LATE"):
        s = 10.0 ** rng.uniform(-7.0, -5.0 if (fam == "THIN" and n % 2) else -4.0, n) / d0
        if fam == "SAT_LATE":                  # one opaque sample: in chunk 2 or later where the ray has one
            p = int(rng.integers(64, n)) if n > 64 else n - 1 - int(rng.integers(0, max(1, n // 3)))
            s[p] = rng.uniform(8.0, 14.0) / d0[p]
    elif fam == "WALL":                        # zeros, then sigma delta > 100: alpha == 1 and T == 0 from there on
        z = int(rng.integers(n // 3, 2 * n // 3 + 1)) if n > 1 else 0
        s[z:] = rng.uniform(120.0, 400.0, n - z) / d0[z:]
    elif fam == "ONE_HOT":
        p = int(rng.integers(0, n))
        s[p] = 200.0 / d0[p]
    return s.astype(F32), d


@functools.lru_cache(maxsize=None)
def make_case(i, C=None):
    """Case i of N_CASES: N = NS[i % 8] rays in permuted table order with permuted ids, one empty ray from N = 3, one
    dropped ray from N = 4 (its reservation ends at M exactly in even cases, 3 rows past M in odd ones, and starts 2 rows
    below `counter`), C and the background form cycling (C given: that channel count, for the three-channel oracle)."""
    N = NS[i % len(NS)]
    C = C or (3, 1, 2)[i % 3]
    form = BG_FORMS[(i + i // 3) % 3]
    rng = np.random.default_rng([SEED, i, C])
    s0 = sum(_live_slots(NS[j % len(NS)]) for j in range(i))
    kinds = [_slot(s0 + j) for j in range(_live_slots(N))]
    if N >= 3:
        kinds.insert(int(rng.integers(0, len(kinds) + 1)), (EMPTY, 0))
    fam, off, cnt, sig, dl = [], [], [], [], []
    used = 0
    for f, n in kinds:
        fam.append(f), off.append(used), cnt.append(n)
        if n:
            s, d = make_samples(f, n, rng)
            sig.append(s), dl.append(d)
            used += n
    if N >= 4:
        n_drop = 40
        fam.append(DROPPED), off.append(used), cnt.append(n_drop)
        M = used + n_drop - (0 if i % 2 == 0 else 3)
        counter = used + 2
    else:
        M, counter = used + 5, used
    sigmas, deltas = np.concatenate(sig), np.concatenate(dl)
    pad = M - used                                              # unowned rows hold ordinary values, not zeros
    sigmas = np.concatenate([sigmas, rng.uniform(0.0, 25.0, pad).astype(F32)])
    deltas = np.concatenate([deltas, rng.uniform(1e-3, 2e-2, (pad, 2)).astype(F32)])
    rgbs = rng.uniform(0.0, 1.0, (M, C)).astype(F32)
    order = rng.permutation(N)
    rays = np.stack([rng.permutation(N), np.array(off)[order], np.array(cnt)[order]], 1).astype(np.int32)
    bg = {"scalar": float(F32(0.37)), "shared": rng.uniform(0.0, 1.0, C).astype(F32),
          "ray": rng.uniform(0.0, 1.0, (N, C)).astype(F32)}[form]
    bg_rows = np.broadcast_to(np.asarray(bg, F32), (N, C)).copy()
    pixels = rng.uniform(0.0, 1.0, (N, C + 1)).astype(F32)
    c = dict(i=i, N=N, C=C, M=M, used=used, counter=counter, form=form, rays=rays, fam=[fam[k] for k in order],
             sigmas=sigmas, deltas=deltas, rgbs=rgbs, bg=bg, bg_rows=bg_rows,
             target=rng.uniform(0.0, 1.0, (N, C)).astype(F32), pixels=pixels,
             g_image=rng.normal(size=(N, C)).astype(F32), g_ws=rng.normal(size=N).astype(F32),
             grad_scale=float(F32(2.5 / (C * N))), frame_scale=float(F32(2.0 / (C * N))))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def marched(c, n, rule_gt=False):
    off, cnt = int(c["rays"][n, 1]), int(c["rays"][n, 2])
    return cnt != 0 and not (off + cnt > c["M"] if rule_gt else off + cnt >= c["M"])


# ------------------------------------------------------------------------------------------ the fp64 reference and its bars
def _incl(a):
    return np.cumsum(a, axis=0)


def _sum_bar(term, e_term, products):
    """(s_k, E_s[k]) of the docstring's `sums`, along axis 0."""
    hat = _incl(term + e_term)
    return _incl(term), _incl(e_term) + U * (_incl(hat) + (6 + products) * hat)


def reference_ray(sig, dl, rgb):
    """Forward quantities of one ray and their bars, everything float64."""
    s, d0, d1, c = sig.astype(np.float64), dl[:, 0].astype(np.float64), dl[:, 1].astype(np.float64), rgb.astype(np.float64)
    n = len(s)
    x = s * d0
    alpha, om = -np.expm1(-x), np.exp(-x)
    Tpost = np.cumprod(om)
    Tpre = np.concatenate([[1.0], Tpost[:-1]])
    w = alpha * Tpre
    da = U * (3.0 * x * om + 2.0 * om + alpha)
    ET = np.zeros(n + 1)
    for k in range(n):
        e = ET[k] * (om[k] + da[k]) + Tpre[k] * da[k]
        ET[k + 1] = e + U * (Tpost[k] + e) + ETA
    e = (alpha + da) * ET[:-1] + Tpre * da
    Ew = e + U * (w + e) + ETA
    t = np.cumsum(d1)
    Et = np.arange(n) * U * t
    ws_k, Ews_k = _sum_bar(w, Ew, 0)
    im_k, Eim_k = _sum_bar(w[:, None] * c, Ew[:, None] * c, 1)
    dp_k, Edp_k = _sum_bar(w * t, Ew * t + (w + Ew) * Et, 1)
    return dict(n=n, d0=d0, c=c, alpha=alpha, Tpre=Tpre, Tpost=Tpost, w=w, ET=ET, Ew=Ew, ws_k=ws_k, im_k=im_k,
                ws=ws_k[-1], E_ws=Ews_k[-1], image=im_k[-1], E_image=Eim_k[-1], depth=dp_k[-1], E_depth=Edp_k[-1])


def blend(r, bg):
    """out = image + (1 - ws) bg and its bar; r None: an unmarched ray (out == bg, exactly)."""
    bg = bg.astype(np.float64)
    if r is None:
        return bg, np.zeros_like(bg)
    rest = abs(1.0 - r["ws"]) + r["E_ws"]
    out = r["image"] + (1.0 - r["ws"]) * bg
    e = r["E_image"] + np.abs(bg) * (r["E_ws"] + U * rest) + U * np.abs(bg) * rest
    return out, e + U * (np.abs(out) + e)


def gradients_ray(r, g, gws, dg=None, dgws=0.0, weight=None):
    """d sigma [n], d rgb [n, C] of one ray for the upstream (g [C], gws) with bars (dg, dgws), and their bars."""
    C = len(g)
    dg = np.zeros(C) if dg is None else dg
    c, w, Tpost = r["c"], r["w"], r["Tpost"]
    wc = w[:, None] * c
    R = np.concatenate([np.cumsum(wc[::-1], axis=0)[::-1][1:], np.zeros((1, C))])
    Rw = np.concatenate([np.cumsum(w[::-1])[::-1][1:], [0.0]])
    A, B = Tpost[:, None] * c - R, Tpost - Rw
    ETp = r["ET"][1:]
    That = Tpost + ETp
    EA = ETp[:, None] * c + U * That[:, None] * c + 2.0 * r["E_image"] + U * (R + 2.0 * r["E_image"])
    EA = EA + U * (np.abs(A) + EA)
    EB = ETp + U * That + 2.0 * r["E_ws"] + U * (Rw + 2.0 * r["E_ws"])
    EB = EB + U * (np.abs(B) + EB)
    Ahat, Bhat = np.abs(A) + EA, np.abs(B) + EB
    ghat, gwhat = np.abs(g) + dg, abs(gws) + dgws
    terms = (ghat * Ahat).sum(1) + gwhat * Bhat
    ds = r["d0"] * ((g * A).sum(1) + gws * B)
    Eds = r["d0"] * ((np.abs(g) * EA + dg * Ahat).sum(1) + abs(gws) * EB + dgws * Bhat + (C + 2) * U * terms) + ETA
    what = w + r["Ew"]
    dr = g * w[:, None]
    Edr = np.abs(g) * r["Ew"][:, None] + dg * what[:, None] + U * ghat * what[:, None] + ETA
    if weight is not None:
        Eds = weight * Eds + U * weight * (np.abs(ds) + Eds) + ETA
        Edr = weight * Edr + U * weight * (np.abs(dr) + Edr) + ETA
        ds, dr = weight * ds, weight * dr
    return ds, Eds, dr, Edr


def frame_gt(c, with_alpha):
    """The frame tail's target in fp64 and its bar: pixels, or pixels[:C] a + bg (1 - a)."""
    C = c["C"]
    p = c["pixels"][:, :C].astype(np.float64)
    if not with_alpha:
        return p, np.zeros_like(p)
    a, bg = c["pixels"][:, C:].astype(np.float64), c["bg_rows"].astype(np.float64)
    gt = p * a + bg * (1.0 - a)
    return gt, U * (np.abs(p * a) + 2.0 * np.abs(bg * (1.0 - a)) + np.abs(gt))


@functools.lru_cache(maxsize=None)
def forward_reference(i, C=None):
    """Per-output (reference, bar) arrays indexed by ray id, and the per-ray records (None: unmarched) by table row."""
    c = make_case(i, C)
    N, Cc = c["N"], c["C"]
    ref = {k: (np.zeros(s), np.zeros(s)) for k, s in dict(ws=N, depth=N, image=(N, Cc), out=(N, Cc)).items()}
    recs = []
    for n in range(N):
        idx, off, cnt = (int(v) for v in c["rays"][n])
        r = reference_ray(c["sigmas"][off:off + cnt], c["deltas"][off:off + cnt], c["rgbs"][off:off + cnt]) \
            if marched(c, n) else None
        recs.append(r)
        if r is not None:
            for k in ("ws", "depth", "image"):
                ref[k][0][idx], ref[k][1][idx] = r[k], r["E_" + k]
        ref["out"][0][idx], ref["out"][1][idx] = blend(r, c["bg_rows"][idx])
    return ref, recs


def upstream(c, form, out_written=None):
    """-> g [N, C], gws [N], dg [N, C], dgws [N], weight by ray id.  form: plain (the case's random fp32 gradients), mse,
    frames, frames_alpha (from `out_written`, the kernel's own out_image)."""
    N, C = c["N"], c["C"]
    if form == "plain":
        return c["g_image"].astype(np.float64), c["g_ws"].astype(np.float64), np.zeros((N, C)), np.zeros(N), None
    o, bg = out_written.astype(np.float64), c["bg_rows"].astype(np.float64)
    if form == "mse":
        g = (o - c["target"].astype(np.float64)) * c["grad_scale"]
        dg = 2.0 * U * np.abs(g)
        weight = None
    else:
        gt, Egt = frame_gt(c, form == "frames_alpha")
        g = (o - gt) * c["frame_scale"]
        dg = c["frame_scale"] * (Egt + U * np.abs(o - gt)) + U * np.abs(g)
        dg = dg + U * dg
        weight = W03
    gws = -(g * bg).sum(1)
    dgws = (np.abs(bg) * dg).sum(1) + C * U * ((np.abs(g) + dg) * np.abs(bg)).sum(1)
    return g, gws, dg, dgws, weight


def gradient_reference(i, form, out_written=None, C=None):
    """(reference, bar) of grad_sigmas [M] and grad_rgbs [M, C].  Rows no marched ray owns: NaN in the plain form (the
    kernel must leave the caller's buffer alone), zero in the others (the dropped ray's reservation and [counter, M);
    with `counter` inside the dropped reservation these cover every such row)."""
    c = make_case(i, C)
    _, recs = forward_reference(i, C)
    g, gws, dg, dgws, weight = upstream(c, form, out_written)
    fill = np.nan if form == "plain" else 0.0
    gs, Egs = np.full(c["M"], fill), np.zeros(c["M"])
    gr, Egr = np.full((c["M"], c["C"]), fill), np.zeros((c["M"], c["C"]))
    for n, r in enumerate(recs):
        if r is None:
            continue
        idx, off, cnt = (int(v) for v in c["rays"][n])
        gs[off:off + cnt], Egs[off:off + cnt], gr[off:off + cnt], Egr[off:off + cnt] = \
            gradients_ray(r, g[idx], gws[idx], dg[idx], dgws[idx], weight)
    return dict(gs=(gs, Egs), gr=(gr, Egr))


def weight_reference(unweighted, weight=W03):
    """A weighted call's gradients are fl(weight * the unweighted call's): (reference, bar) from the unweighted result."""
    ref = weight * unweighted.astype(np.float64)
    return ref, U * np.abs(ref) + ETA


def row_families(c):
    """Family of the ray that owns each sample row ('' for unowned rows), and by ray id."""
    rows = np.array([""] * c["M"], dtype=object)
    by_id = np.array([""] * c["N"], dtype=object)
    for n in range(c["N"]):
        idx, off, cnt = (int(v) for v in c["rays"][n])
        rows[off:min(off + cnt, c["M"])] = c["fam"][n]
        by_id[idx] = c["fam"][n]
    return rows, by_id


# ------------------------------------------------------------------------------------------------------------ the comparator
def ratios(ref, bar, got):
    """|got - ref| / bar elementwise.  bar == 0: 0 where got equals ref (NaN equals NaN: an untouched sentinel), inf else;
    a NaN or inf where a number is expected: inf."""
    ref, bar, got = np.asarray(ref, np.float64), np.asarray(bar, np.float64), np.asarray(got, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        same = (got == ref) | (np.isnan(got) & np.isnan(ref))
        r = np.where(bar > 0, np.abs(got - ref) / np.where(bar > 0, bar, 1.0), np.where(same, 0.0, np.inf))
    return np.where(np.isfinite(got) | same, r, np.inf)


class Worst:
    """Collects the worst error / bar per output and per family over any number of compare() calls."""

    def __init__(self):
        self.worst = {}
        self.fails = []

    def compare(self, what, output, ref_bar, got, families):
        ref, bar = ref_bar
        r = ratios(ref, bar, got)
        fam = np.asarray(families, dtype=object)
        fam = np.broadcast_to(fam.reshape(fam.shape + (1,) * (r.ndim - fam.ndim)), r.shape)
        for f in np.unique(fam.astype(str)):
            v = float(r[fam == f].max())
            key = (output, f)
            self.worst[key] = max(self.worst.get(key, 0.0), v)
            if not v < 1.0:
                at = int(np.argmax(np.where(fam == f, r, -1.0)))
                self.fails.append(f"{what}: {output} [{f or 'unowned'}] error / bar = {v:.3g} at flat index {at}")
        return r

    def per_output(self):
        out = {}
        for (o, _), v in self.worst.items():
            out[o] = max(out.get(o, 0.0), v)
        return out

    def report(self, title):
        fams = sorted({f for _, f in self.worst})
        lines = [title]
        for o, v in sorted(self.per_output().items()):
            per = ", ".join(f"{f or 'unowned'} {self.worst[(o, f)]:.3g}" for f in fams if (o, f) in self.worst)
            lines.append(f"  {o}: worst error / bar = {v:.3g}   ({per})")
        return "\n".join(lines)


def check_run(W, what, i, form, got, unweighted=None):
    """Every output of one run (forward, blend, gradients of `form`) against the reference; frame forms also against
    fl(weight * the unweighted run).  The GPU test feeds the kernels' outputs through this same function."""
    c = make_case(i)
    rows, by_id = row_families(c)
    fwd, _ = forward_reference(i)
    for name in ("ws", "depth", "image", "out"):
        if name in got:
            W.compare(what, name, fwd[name], got[name], by_id)
    if "gs" in got:
        ref = gradient_reference(i, form, got.get("out"))
        W.compare(what, "grad_sigmas", ref["gs"], got["gs"], rows)
        W.compare(what, "grad_rgbs", ref["gr"], got["gr"], rows)
    if unweighted is not None:
        W.compare(what, "grad_sigmas vs weight 1", weight_reference(unweighted["gs"]), got["gs"], rows)
        W.compare(what, "grad_rgbs vs weight 1", weight_reference(unweighted["gr"]), got["gr"], rows)


# --------------------------------------------------------------- the kernels' scan order, stated in numpy fp32 (csrc/common.h)
_LANE = np.arange(64)
_ROW_SHR = {n: (_LANE % 16 >= n, np.maximum(_LANE - n, 0)) for n in (1, 2, 4, 8)}
DEFECTS = ["no_T_carry", "no_colour_carry", "no_ws_carry", "Tpre_in_dsigma", "delta1_in_alpha", "no_delta0_in_dsigma",
           "bg_sign", "weight_folded_into_g", "no_row_bcast15", "drop_rule_gt"]


def wave_scan(v, op, identity, skip_bcast15=False):
    """wave_incl_scan_add / _mul: Hillis-Steele steps 1, 2, 4, 8 inside each 16-lane row (a lane without a source takes
    the identity), lane 15 of rows 0 / 2 into rows 1 / 3, lane 31 into rows 2 and 3; every operation rounds to fp32."""
    v = v.astype(F32)
    ident = F32(identity)
    for n in (1, 2, 4, 8):
        has, src = _ROW_SHR[n]
        v = op(v, np.where(has, v[src], ident)).astype(F32)
    if not skip_bcast15:
        t = np.full(64, ident, F32)
        t[16:32], t[48:64] = v[15], v[47]
        v = op(v, t).astype(F32)
    t = np.full(64, ident, F32)
    t[32:64] = v[31]
    return op(v, t).astype(F32)


def _chunks(c, off, cnt, defect):
    """comp_chunk over one ray: yields (rows, active, dl0, rgb, w, Tpre, Tpost, c_i, ws_i) per chunk; the last carry is
    returned through the dict `fin`."""
    C = c["C"]
    one, zero = F32(1.0), F32(0.0)
    kT, kt, kc, kws, kd = one, zero, np.zeros(C, F32), zero, zero
    add, mul = np.add, np.multiply
    skip = defect == "no_row_bcast15"
    for s0 in range(0, cnt, 64):
        act = s0 + _LANE < cnt
        p = off + np.where(act, s0 + _LANE, 0)
        sig, dl0, dl1, rgb = c["sigmas"][p], c["deltas"][p, 0], c["deltas"][p, 1], c["rgbs"][p]
        arg = -sig * (dl1 if defect == "delta1_in_alpha" else dl0)
        alpha = np.where(act, one - np.exp(arg.astype(F32)).astype(F32), zero).astype(F32)
        P = wave_scan(one - alpha, mul, 1.0, skip)
        Pex = np.concatenate([[one], P[:-1]]).astype(F32)
        Tpre = (kT * Pex).astype(F32)
        w = (alpha * Tpre).astype(F32)
        Tpost = (kT * P).astype(F32)
        tt = (kt + wave_scan(np.where(act, dl1, zero), add, 0.0, skip)).astype(F32)
        c_i = np.stack([(kc[q] + wave_scan((w * rgb[:, q]).astype(F32), add, 0.0, skip)).astype(F32) for q in range(C)], 1)
        ws_i = (kws + wave_scan(w, add, 0.0, skip)).astype(F32)
        d_i = (kd + wave_scan((w * tt).astype(F32), add, 0.0, skip)).astype(F32)
        yield p, act, dl0, rgb, w, Tpre, Tpost, c_i, ws_i
        kT = one if defect == "no_T_carry" else Tpost[63]
        kt, kd = tt[63], d_i[63]
        kc = np.zeros(C, F32) if defect == "no_colour_carry" else c_i[63].copy()
        kws = zero if defect == "no_ws_carry" else ws_i[63]
    yield dict(ws=kws, depth=kd, image=kc)


def kernel_statement(i, form, defect=None, weight=W03, C=None):
    """What k_composite_train_fwd (+ blend) and k_composite_train_bwd / the fused kernel's tails compute, in their order,
    in numpy fp32, with one of DEFECTS seeded on request.  -> ws, depth, image, out by ray id; gs [M], gr [M, C]."""
    c = make_case(i, C)
    N, M, Cc = c["N"], c["M"], c["C"]
    nan = lambda *s: np.full(s, np.nan, F32)
    o = dict(ws=nan(N), depth=nan(N), image=nan(N, Cc), out=nan(N, Cc), gs=nan(M), gr=nan(M, Cc))
    fused = form != "plain"
    if fused:
        o["gs"][c["counter"]:], o["gr"][c["counter"]:] = 0.0, 0.0
    for n in range(N):
        idx, off, cnt = (int(v) for v in c["rays"][n])
        bg = c["bg_rows"][idx]
        if not marched(c, n, defect == "drop_rule_gt"):
            o["ws"][idx], o["depth"][idx], o["image"][idx], o["out"][idx] = 0.0, 0.0, 0.0, bg
            if fused and cnt and off < M:
                o["gs"][off:], o["gr"][off:] = 0.0, 0.0
            continue
        *_, fin = _chunks(c, off, cnt, defect)
        o["ws"][idx], o["depth"][idx], o["image"][idx] = fin["ws"], fin["depth"], fin["image"]
        rest = F32(1.0) - fin["ws"]
        out = (fin["image"] + (rest * bg).astype(F32)).astype(F32)
        o["out"][idx] = out
        if form == "plain":
            g, gws = c["g_image"][idx], c["g_ws"][idx]
        else:
            if form == "mse":
                tg, sc = c["target"][idx], F32(c["grad_scale"])
            else:
                px, sc = c["pixels"][idx], F32(c["frame_scale"])
                if form == "frames_alpha":
                    a = px[Cc]
                    tg = ((px[:Cc] * a).astype(F32) + (bg * (F32(1.0) - a)).astype(F32)).astype(F32)
                else:
                    tg = px[:Cc]
            g = ((out - tg).astype(F32) * sc).astype(F32)
            if form != "mse" and defect == "weight_folded_into_g":
                g = (F32(weight) * g).astype(F32)
            dot = F32(0.0)
            for q in range(Cc):
                dot = (g[q] * bg[q]).astype(F32) if q == 0 else (dot + (g[q] * bg[q]).astype(F32)).astype(F32)
            gws = dot if defect == "bg_sign" else -dot
        for ch in _chunks(c, off, cnt, defect):
            if isinstance(ch, dict):
                break
            p, act, dl0, rgb, w, Tpre, Tpost, c_i, ws_i = ch
            T = Tpre if defect == "Tpre_in_dsigma" else Tpost
            acc = None
            for q in range(Cc):
                term = (g[q] * ((T * rgb[:, q]).astype(F32) - (fin["image"][q] - c_i[:, q]).astype(F32)).astype(F32)).astype(F32)
                acc = term if acc is None else (acc + term).astype(F32)
            acc = (acc + (gws * (T - (fin["ws"] - ws_i).astype(F32)).astype(F32)).astype(F32)).astype(F32)
            gs = acc if defect == "no_delta0_in_dsigma" else (dl0 * acc).astype(F32)
            gr = (g[None, :] * w[:, None]).astype(F32)
            if form not in ("plain", "mse") and defect != "weight_folded_into_g":
                gs, gr = (F32(weight) * gs).astype(F32), (F32(weight) * gr).astype(F32)
            o["gs"][p[act]], o["gr"][p[act]] = gs[act], gr[act]
    return o


# ------------------------------------------------------------------------------------------------------ inference compositing
INFER_STOP = 1e-5
INFER_N = 256


def infer_ray_samples(kind, n, rng):
    """Samples of one inference ray.  T stays above 1e-3 until one opaque sample at `kind` (an index, or None: the ray
    never stops) takes it below 1e-6 in one step, so the fp32 comparison with 1e-5 is far from both sides."""
    d = rng.uniform(1e-3, 2e-2, (n, 2)).astype(F32)
    d0 = d[:, 0].astype(np.float64)
    x = rng.uniform(0.0, 5.0 / n, n) * (rng.random(n) < 0.8)
    s = x / d0
    if kind is not None:
        s[kind] = rng.uniform(15.0, 30.0) / d0[kind]
    return s.astype(F32), d


def infer_sequence(S0, D0, I0, t0, sig, dl, rgb):
    """The recurrence of k_composite_rays over the given samples in fp64 with its bars, from exact fp32 starting values:
    stops at delta0 == 0 (before the sample) and after the sample whose pre-sample T is below 1e-5.
    -> dict(S, D, I, t, steps, stopped, near_threshold) and bars E_S, E_D, E_I."""
    S, D, I, t = float(S0), float(D0), I0.astype(np.float64).copy(), float(t0)
    ES, ED, EI, Et = 0.0, 0.0, np.zeros_like(I), 0.0
    near, stopped, k = False, False, 0
    while k < len(sig):
        d0, d1 = float(dl[k, 0]), float(dl[k, 1])
        if d0 == 0.0:
            stopped = True
            break
        x = float(sig[k]) * d0
        a, om = -np.expm1(-x), np.exp(-x)
        da = U * (3.0 * x * om + 2.0 * om + a)
        T = 1.0 - S
        That = abs(T) + ES + U * (abs(T) + ES)
        ETk = ES + U * That
        near = near or abs(T - INFER_STOP) <= max(1e-8, ETk)
        w = a * T
        e = (a + da) * ETk + abs(T) * da
        Ew = e + U * (abs(w) + e) + ETA
        what = abs(w) + Ew
        S2 = S + w
        ES = ES * (om + da) + (a + da) * U * That + abs(T) * da + U * (what + abs(S2) + ES) + ETA
        S = S2
        t += d1
        Et += U * abs(t)
        c = rgb[k].astype(np.float64)
        D = D + w * t
        ED = ED + Ew * abs(t) + what * Et
        ED += U * (abs(D) + ED)
        I = I + w * c
        EI = EI + Ew * c
        EI += U * (np.abs(I) + EI)
        k += 1
        if T < INFER_STOP:
            stopped = True
            break
    return dict(S=S, D=D, I=I, t=t, consumed=k, stopped=stopped, near=near, ES=ES, ED=ED, EI=EI)


INFER_COUNTS = [1, 7, 8, 9, 13, 16, 24, 40]
INFER_STEPS = (8, 16)                                          # samples per ray in the two rounds of composite_rays
INFER_FIXED = [(40, 2), (40, 6), (40, 7), (24, 22), (24, 23), (16, 14), (16, 15), (8, 6), (8, 7), (9, 7), (9, 8), (1, 0),
               (40, None), (7, None), (13, 11), (13, 12)]       # (count, index of the opaque sample): the ray stops one later


@functools.lru_cache(maxsize=None)
def infer_case(C, seed=7):
    """INFER_N rays for the two inference kernels, contiguous samples, permuted ids.  The opaque sample sits so that rays
    stop in the first group of eight, on a group's last and next group's first sample, on their last sample, past it
    (never: T is tiny but no sample follows) and not at all; ten rays decay gradually through 1e-5 instead."""
    rng = np.random.default_rng([SEED, seed, C])
    N = INFER_N
    spec = list(INFER_FIXED)
    while len(spec) < N - 10:
        n = INFER_COUNTS[int(rng.integers(0, len(INFER_COUNTS)))]
        spec.append((n, int(rng.integers(0, n)) if rng.random() < 0.8 else None))
    spec += [(40, "gradual")] * 10
    sig, dl = [], []
    for n, p in spec:
        if p == "gradual":
            d = rng.uniform(1e-3, 2e-2, (n, 2)).astype(F32)
            s = (rng.uniform(0.3, 1.5, n) / d[:, 0].astype(np.float64)).astype(F32)
        else:
            s, d = infer_ray_samples(p, n, rng)
        sig.append(s), dl.append(d)
    counts = np.array([n for n, _ in spec])
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]])
    M = int(counts.sum()) + 1
    sigmas = np.concatenate(sig + [np.ones(1, F32)])
    deltas = np.concatenate(dl + [np.full((1, 2), 0.01, F32)])
    rgbs = rng.uniform(0.0, 1.0, (M, C)).astype(F32)
    order = rng.permutation(N)
    rays = np.stack([rng.permutation(N), offs[order], counts[order]], 1).astype(np.int32)
    nears = rng.uniform(0.2, 1.0, N).astype(F32)
    fars = (nears + rng.uniform(1.0, 3.0, N)).astype(F32)
    return dict(N=N, C=C, M=M, rays=rays, sigmas=sigmas, deltas=deltas, rgbs=rgbs, nears=nears, fars=fars,
                bg=rng.uniform(0.0, 1.0, (N, C)).astype(F32), spec=[spec[k] for k in order])


def infer_frame_reference(c):
    """composite_rays_frame in fp64: weights_sum, depth (normalised), image (blended), by ray id, with bars; `keep` marks
    the rays whose T stays clear of the stop threshold; used = the samples consumed."""
    N, C = c["N"], c["C"]
    ws, dp, im = np.zeros((2, N)), np.zeros((2, N)), np.zeros((2, N, C))
    keep, used = np.ones(N, bool), np.zeros(N, np.int64)
    for n in range(N):
        idx, off, cnt = (int(v) for v in c["rays"][n])
        near, far = float(c["nears"][idx]), float(c["fars"][idx])
        r = infer_sequence(0.0, 0.0, np.zeros(C), near, c["sigmas"][off:off + cnt], c["deltas"][off:off + cnt],
                           c["rgbs"][off:off + cnt])
        keep[idx], used[idx] = not r["near"], r["consumed"]
        bg = c["bg"][idx].astype(np.float64)
        rest = abs(1.0 - r["S"]) + r["ES"]
        ws[:, idx] = r["S"], r["ES"]
        out = r["I"] + (1.0 - r["S"]) * bg
        e = r["EI"] + bg * (r["ES"] + U * rest) + U * bg * rest
        im[:, idx] = out, e + U * (np.abs(out) + e)
        num = max(r["D"] - near, 0.0)
        depth = num / (far - near)
        dp[:, idx] = depth, (r["ED"] + U * (abs(r["D"] - near) + r["ED"])) / (far - near) * (1 + 2 * U) + 2 * U * depth + ETA
    return dict(ws=ws, depth=dp, image=im, keep=keep, used=used)


def infer_round_inputs(c, rnd, alive_rows):
    """The [n_alive, n_step] sample blocks of round `rnd` for the table rows `alive_rows`: the ray's samples
    [start, start + n_step), zero rows (the delta == 0 terminator) where the ray has no more."""
    C, n_step = c["C"], INFER_STEPS[rnd]
    start = sum(INFER_STEPS[:rnd])
    A = len(alive_rows)
    sig, dl, rgb = np.zeros((A, n_step), F32), np.zeros((A, n_step, 2), F32), np.zeros((A, n_step, C), F32)
    for a, n in enumerate(alive_rows):
        _, off, cnt = (int(v) for v in c["rays"][n])
        m = max(0, min(n_step, cnt - start))
        sl = slice(off + start, off + start + m)
        sig[a, :m], dl[a, :m], rgb[a, :m] = c["sigmas"][sl], c["deltas"][sl], c["rgbs"][sl]
    return sig, dl, rgb


def infer_round_reference(c, rnd, alive_rows, rays_t, ws, depth, image):
    """One round of composite_rays in fp64 from the fp32 state it starts from (by ray id; rays_t by alive slot).
    -> (reference, bar) of rays_t [A] (-1: the ray ended), and of ws, depth, image at the alive rays' ids; keep [A]."""
    sig, dl, rgb = infer_round_inputs(c, rnd, alive_rows)
    A, C = len(alive_rows), c["C"]
    o = dict(t=np.zeros((2, A)), ws=np.zeros((2, A)), depth=np.zeros((2, A)), image=np.zeros((2, A, C)))
    keep = np.ones(A, bool)
    for a, n in enumerate(alive_rows):
        idx = int(c["rays"][n, 0])
        r = infer_sequence(ws[idx], depth[idx], image[idx], rays_t[a], sig[a], dl[a], rgb[a])
        keep[a] = not r["near"]
        o["t"][:, a] = (-1.0, 0.0) if r["stopped"] else (r["t"], INFER_STEPS[rnd] * U * abs(r["t"]))
        o["ws"][:, a], o["depth"][:, a], o["image"][:, a] = (r["S"], r["ES"]), (r["D"], r["ED"]), (r["I"], r["EI"])
    return o, keep
