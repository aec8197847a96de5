"""fp64 statement, error model and checker for the background model (csrc/background.hip: k_bg_fwd, k_bg_bwd; the torch
statement is NeRFNetwork.background behind raymarching.polar_from_ray).  numpy only.

The operation, per ray (nerf/network.py, nerf/renderer.py of the reference; weights without bias):
    p     = polar coordinates of the ray's exit from the sphere of radius R          polar64
    grid  = 2-D multiresolution grid (level_dim 2, L levels) of (p + 1) / 2          cells + features
    x     = [SH16(d) or zeros | grid]                                                K = 16 + 2L columns
    bg    = sigmoid(W1 relu(W0 x))                                                   W0 [64, K], W1 [C, 64]
and its backward for g_bg = (1 - weights_sum) * grad_image:
    d o = g_bg * bg (1 - bg),  dW1 = d o^T relu(h),  d h = (h > 0) * (d o W1),  dW0 = d h^T x,  d x = d h W0,
    dE[row] += corner weight * d x[grid column]   for the four corners of every level's cell.

Which cell a point falls into, and its four corner weights, are taken as the fp32 arithmetic of the encoder makes them
(cells(): every step -- (p + 1) * 0.5, fma(in, scale, 0.5), floor, the fractional part, the weight products -- is one
correctly rounded fp32 operation that numpy repeats bit for bit), so the reference and the kernel interpolate the same
corners with the same weights and what is left to bound is summation error.  A reference "from rays" rounds its fp64 polar
pair to fp32 first and goes on from there; polar_bar() bounds the polar pair itself.

Error model (u = 2^-24, gamma(n) = n u / (1 - n u): a sum of n products in fp32, ANY order, errs by at most gamma(n) times
the sum of the products' magnitudes).  Given the input row x (exact: the kernel's own row, or the statement's):
    h   = W0 x            e_h  = gamma(K) |W0| |x|
    a   = relu(h)         e_a  = e_h where h > 0, else 0        (rays with 0 inside [h - e_h, h + e_h]: see below)
    o   = W1 a            e_o  = (1 + gamma(64)) |W1| e_a + gamma(64) |W1| a
    bg  = sigmoid(o)      e_bg = e_o / 4 + 8 u bg               (slope <= 1/4; expf, the add and the division: <= 8 u)
    s   = bg (1 - bg)     e_s  = e_bg + 3 u s                   (|d s / d bg| <= 1)
    d o = (f g) s         e_do = |f g| e_s + 4 u |f g| s        (f = 1 - weights_sum and f g: one rounding each)
    dW1 = sum_n d o a     bar  = (1 + gamma(N)) sum_n (e_do a + |d o| e_a) + gamma(N + 1) sum_n |d o| a
    d h = m (d o W1)      e_dh = m ((1 + gamma(3)) e_do |W1| + gamma(3) |d o| |W1|)
    dW0 = sum_n d h x     bar  = (1 + gamma(N)) sum_n e_dh |x| + gamma(N + 1) sum_n |d h| |x|
    d x = d h W0          e_dx = (1 + gamma(64)) e_dh |W0| + gamma(64) |d h| |W0|
    dE  = sum w d x       bar  = (1 + gamma(m)) sum w e_dx + gamma(m + 1) sum w |d x|,  m = contributions of the row
Every entry must lie inside its bar: no quantile, no entry left out, a zero bar asks for the exact value (rows of the
table no ray touches).  The one exception: a ray with a hidden unit whose fp64 pre-activation has zero inside its forward
interval (|h| <= e_h, other than h = e_h = 0) is `undecided` -- the ReLU branch the fp32 forward takes is not determined
-- and takes no part in the backward value checks: mask_undecided() zeroes its grad_image row for the code under test
and the reference alike.  At most MAX_UNDECIDED of the rays may be (assert_decided()).

`defect=` seeds one wrong step into the fp64 statement; tests/test_background_ref.py shows the bars reject each.
"""
import numpy as np

U = 2.0 ** -24
MAX_UNDECIDED = 0.01
HIDDEN = 64
DEFECTS = ("grid_sh_order", "theta_phi_swapped", "no_weights_sum", "no_sigmoid_derivative", "no_relu_mask", "hash_prime",
           "corner_weights_swapped")
OUTPUTS = ("bg", "dW1", "dW0", "dE")


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------------------------------------ geometry
def geometry(num_levels=4, base_resolution=16, desired_resolution=2048, log2_hashmap_size=19, gridtype="hash"):
    """Level geometry as GridEncoder makes it (gridencoder.py: level_offsets) and as the kernels derive it from (S, H):
    scale = exp2f(l S) H - 1 in fp32, resolution = ceil(scale) + 1."""
    per_level_scale = np.exp2(np.log2(desired_resolution / base_resolution) / (num_levels - 1)) if num_levels > 1 else 2.0
    offsets, off = [], 0
    for i in range(num_levels):
        res = int(np.ceil(base_resolution * per_level_scale ** i))
        n = min(2 ** log2_hashmap_size, (res + 1) ** 2)
        offsets.append(off)
        off += int(np.ceil(n / 8) * 8)
    offsets.append(off)
    S = np.float32(np.log2(per_level_scale))
    scale = np.array([np.float32(np.exp2(np.float32(l) * S)) * np.float32(base_resolution) - np.float32(1.0)
                      for l in range(num_levels)], dtype=np.float32)
    return dict(L=num_levels, S=float(S), H=int(base_resolution), per_level_scale=float(per_level_scale),
                offsets=np.array(offsets, dtype=np.int64), scale=scale,
                resolution=np.ceil(scale.astype(np.float64)).astype(np.int64) + 1,
                gridtype_id={"hash": 0, "tiled": 1}[gridtype], log2_hashmap_size=log2_hashmap_size)


def _level_rows(px, py, size, res, gridtype_id, prime=2654435761):
    """Row of the vertices (px, py) inside a level of `size` rows (gridencoder.cu:60-84 for D = 2), uint32 arithmetic."""
    M = 0xFFFFFFFF
    stride, strides, max_index = 1, [0, 0], 0
    for d in range(2):
        if stride <= size:
            strides[d] = stride
            max_index += res * stride
            stride = (stride * (res + 1)) & M
    hashed = gridtype_id == 0 and stride > size
    px, py = px.astype(np.uint64) & M, py.astype(np.uint64) & M
    if hashed:
        index = (px ^ ((py * prime) & M)) & M
    else:
        index = (px * strides[0] + py * strides[1]) & M
    return (index % size).astype(np.int64), hashed


def cells(p32, geo, defect=None):
    """fp32 polar pairs [N, 2] -> (rows [N, L, 4] int64: absolute table rows of the four corners, corner idx adding bit d of
    idx to coordinate d; w [N, L, 4] float32: their weights; inside [N] bool: (p + 1) / 2 within [0, 1], else the encoder
    writes zeros and scatters nothing; hashed [L]).  Bit for bit the encoder's own fp32 arithmetic."""
    p32 = np.asarray(p32, dtype=np.float32)
    N, L = p32.shape[0], geo["L"]
    x = (p32 + np.float32(1.0)) * np.float32(0.5)
    inside = ~((x < 0) | (x > 1)).any(axis=1)
    rows = np.zeros((N, L, 4), dtype=np.int64)
    w = np.zeros((N, L, 4), dtype=np.float32)
    hashed = np.zeros(L, dtype=bool)
    xs = np.where(inside[:, None], x, np.float32(0.0))
    for l in range(L):
        scale = np.float64(geo["scale"][l])
        pos = (xs.astype(np.float64) * scale + 0.5).astype(np.float32)              # fmaf(in, scale, 0.5)
        pg = np.floor(pos)
        frac = (pos - pg).astype(np.float32)
        pg = pg.astype(np.int64)
        size = int(geo["offsets"][l + 1] - geo["offsets"][l])
        prime = 805459861 if defect == "hash_prime" else 2654435761
        for idx in range(4):
            wi = np.ones(N, dtype=np.float32)
            for d in range(2):
                hi = bool(idx & (1 << d))
                if defect == "corner_weights_swapped" and d == 0:
                    hi = not hi
                wi = (wi * (frac[:, d] if hi else (np.float32(1.0) - frac[:, d]).astype(np.float32))).astype(np.float32)
            r, hashed[l] = _level_rows(pg[:, 0] + (idx & 1), pg[:, 1] + ((idx >> 1) & 1), size, int(geo["resolution"][l]),
                                       geo["gridtype_id"], prime)
            rows[:, l, idx] = geo["offsets"][l] + r
            w[:, l, idx] = wi
    return rows, w, inside, hashed


# --------------------------------------------------------------------------------------------------------------- stages
def polar64(rays_o, rays_d, radius, defect=None):
    """raymarching.cu:165-200 in fp64 -> p [N, 2]."""
    o, d = np.asarray(rays_o, np.float64), np.asarray(rays_d, np.float64)
    A = (d * d).sum(-1)
    B = (o * d).sum(-1)
    C = (o * o).sum(-1) - float(radius) ** 2
    t = (-B + np.sqrt(B * B - A * C)) / A
    q = o + t[:, None] * d
    theta = np.arctan2(np.sqrt(q[:, 0] ** 2 + q[:, 2] ** 2), q[:, 1])
    phi = np.arctan2(q[:, 2], q[:, 0])
    p = np.stack([2 * theta / np.pi - 1, phi / np.pi], -1)
    return p[:, ::-1].copy() if defect == "theta_phi_swapped" else p


def polar_bar(rays_o, rays_d, radius):
    """Bound on |fp32 polar pair - polar64| for unit directions and origins inside 0.8 R.  There A = 1, |B| <= 0.8 R and
    B^2 - A C >= 0.36 R^2, so -B + sqrt(.) >= 0.2 R while its terms are at most 1.8 R: t carries the few roundings of A, B,
    C, the square root and the division (<= 8 u) amplified 9 times at the worst, the hit point q = o + t d (|q| = R,
    t <= 1.8 R) then errs by at most 1.8 * 72 u R + 2 u R < 136 u R.  theta is the angle of (rho, y), |(rho, y)| = R: it
    moves by at most 136 u sqrt(2) + 4 u (atan2f, sqrtf) < 200 u radians, times 2 / pi, plus one rounding of the result
    (|p0| <= 1): 130 u.  phi is the angle of (x, z), whose length is rho: 136 u sqrt(2) R / rho + 4 u pi, over pi."""
    o, d = np.asarray(rays_o, np.float64), np.asarray(rays_d, np.float64)
    B = (o * d).sum(-1)
    t = -B + np.sqrt(B * B - ((o * o).sum(-1) - float(radius) ** 2))
    q = o + t[:, None] * d
    rho = np.sqrt(q[:, 0] ** 2 + q[:, 2] ** 2)
    return np.stack([np.full_like(rho, 130 * U), 136 * np.sqrt(2) * U * float(radius) / np.maximum(rho, 1e-300) / np.pi
                     + 6 * U], -1)


def sh64(d):
    """The 16 real spherical harmonics of degree < 4 (shencoder.cu's polynomials) in fp64."""
    d = np.asarray(d, np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xy, yz, xz, x2, y2, z2 = x * y, y * z, x * z, x * x, y * y, z * z
    return np.stack([
        np.full_like(x, 0.28209479177387814), -0.48860251190291987 * y, 0.48860251190291987 * z,
        -0.48860251190291987 * x, 1.0925484305920792 * xy, -1.0925484305920792 * yz,
        0.94617469575755997 * z2 - 0.31539156525251999, -1.0925484305920792 * xz,
        0.54627421529603959 * x2 - 0.54627421529603959 * y2, 0.59004358992664352 * y * (-3.0 * x2 + y2),
        2.8906114426405538 * xy * z, 0.45704579946446572 * y * (1.0 - 5.0 * z2),
        0.3731763325901154 * z * (5.0 * z2 - 3.0), 0.45704579946446572 * x * (1.0 - 5.0 * z2),
        1.4453057213202769 * z * (x2 - y2), 0.59004358992664352 * x * (-x2 + 3.0 * y2)], -1)


def sh_bar(d):
    """|fp32 SH - sh64|: polynomials of degree <= 3 in |d| <= 1 from recurrences of at most ~10 fp32 operations whose
    intermediate magnitudes stay below 16 (the normalised degree-3 terms): 10 * 16 u."""
    return np.full((np.asarray(d).shape[0], 16), 160 * U)


def features(cell, table, L):
    """Bilinear interpolation in fp64 -> (grid [N, 2L], bar [N, 2L]: four fused multiply-adds, gamma(4) sum w |e|)."""
    rows, w, inside = cell[:3]
    E = np.asarray(table, np.float64)
    w64 = w.astype(np.float64) * inside[:, None, None]
    f = (w64[..., None] * E[rows]).sum(2)                                   # [N, L, 2]
    m = (w64[..., None] * np.abs(E[rows])).sum(2)
    N = rows.shape[0]
    return f.reshape(N, 2 * L), (gamma(4) * m).reshape(N, 2 * L)


def input_row(p32, rays_d, table, geo, use_dirs=True, defect=None):
    """-> (x [N, 16 + 2L] fp64, the cells) from an fp32 polar pair."""
    cell = cells(p32, geo, defect)
    grid, _ = features(cell, table, geo["L"])
    sh = sh64(rays_d) if use_dirs else np.zeros((grid.shape[0], 16))
    x = np.concatenate([grid, sh], -1) if defect == "grid_sh_order" else np.concatenate([sh, grid], -1)
    return x, cell


# ------------------------------------------------------------------------------------------------------------ statement
def forward(x, W0, W1):
    """-> dict(h, a, o, bg, e_h, e_a, e_o, e_bg, undecided [N] bool) from the input rows x [N, K]."""
    x, W0, W1 = (np.asarray(t, np.float64) for t in (x, W0, W1))
    K = x.shape[1]
    h = x @ W0.T
    e_h = gamma(K) * (np.abs(x) @ np.abs(W0).T)
    undecided = ((np.abs(h) <= e_h) & ~((h == 0) & (e_h == 0))).any(-1)
    a = np.maximum(h, 0.0)
    e_a = np.where(h > 0, e_h, 0.0)
    o = a @ W1.T
    e_o = (1 + gamma(HIDDEN)) * (e_a @ np.abs(W1).T) + gamma(HIDDEN) * (a @ np.abs(W1).T)
    bg = 1.0 / (1.0 + np.exp(-o))
    e_bg = e_o / 4 + 8 * U * bg
    return dict(h=h, a=a, o=o, bg=bg, e_h=e_h, e_a=e_a, e_o=e_o, e_bg=e_bg, undecided=undecided)


def mask_undecided(grad_image, undecided):
    """grad_image with the rows of the undecided rays zeroed (module docstring: they take no part in the backward)."""
    g = np.array(grad_image, copy=True)
    g[undecided] = 0
    return g


def assert_decided(undecided):
    share = float(np.mean(undecided)) if undecided.size else 0.0
    assert share <= MAX_UNDECIDED, f"{share:.4f} of the rays have an undecided ReLU branch"
    return share


def reference(x, W0, W1, grad_image=None, weights_sum=None, cell=None, table_rows=0, defect=None):
    """The fp64 statement from the input rows x [N, K] -> dict(bg, dW1, dW0, dE [table_rows, 2], bar{...}, undecided, ...).
    Backward only with grad_image [N, C] (rows of undecided rays must already be zero: mask_undecided); `cell` = cells()
    of the rays' polar pairs places the table gradient."""
    x, W0, W1 = (np.asarray(t, np.float64) for t in (x, W0, W1))
    N, K = x.shape
    C = W1.shape[0]
    r = forward(x, W0, W1)
    r["bar"] = dict(bg=r["e_bg"])
    if grad_image is None:
        return r
    g = np.asarray(grad_image, np.float64).reshape(N, C)
    assert defect is not None or not np.any(g[r["undecided"]]), "zero the undecided rays' grad_image rows (mask_undecided)"
    f = np.ones(N) if weights_sum is None or defect == "no_weights_sum" else 1.0 - np.asarray(weights_sum, np.float64)
    fg = f[:, None] * g
    bg, a, h = r["bg"], r["a"], r["h"]
    s = bg * (1 - bg)
    e_s = r["e_bg"] + 3 * U * s
    if defect == "no_sigmoid_derivative":
        s = np.ones_like(s)
    do = fg * s
    e_do = np.abs(fg) * e_s + 4 * U * np.abs(fg) * s
    dW1 = do.T @ a
    bar_W1 = (1 + gamma(N)) * (e_do.T @ a + np.abs(do).T @ r["e_a"]) + gamma(N + 1) * (np.abs(do).T @ a)
    m = np.ones_like(h) if defect == "no_relu_mask" else (h > 0).astype(np.float64)
    dh = m * (do @ W1)
    e_dh = m * ((1 + gamma(3)) * (e_do @ np.abs(W1)) + gamma(3) * (np.abs(do) @ np.abs(W1)))
    dW0 = dh.T @ x
    bar_W0 = (1 + gamma(N)) * (e_dh.T @ np.abs(x)) + gamma(N + 1) * (np.abs(dh).T @ np.abs(x))
    dx = dh @ W0
    e_dx = (1 + gamma(HIDDEN)) * (e_dh @ np.abs(W0)) + gamma(HIDDEN) * (np.abs(dh) @ np.abs(W0))
    r.update(do=do, dh=dh, dx=dx, dW1=dW1, dW0=dW0)
    r["bar"].update(dW1=bar_W1, dW0=bar_W0)
    if cell is not None:
        rows, w, inside = cell[:3]
        L = rows.shape[1]
        w64 = w.astype(np.float64) * inside[:, None, None]                       # [N, L, 4]
        gx = dx[:, 16:16 + 2 * L].reshape(N, L, 1, 2)
        egx = e_dx[:, 16:16 + 2 * L].reshape(N, L, 1, 2)
        flat = rows.reshape(-1)
        dE = np.zeros((table_rows, 2))
        mag = np.zeros((table_rows, 2))
        err = np.zeros((table_rows, 2))
        val, vm, ve = (w64[..., None] * gx), (w64[..., None] * np.abs(gx)), (w64[..., None] * egx)
        for c in range(2):
            np.add.at(dE[:, c], flat, val[..., c].reshape(-1))
            np.add.at(mag[:, c], flat, vm[..., c].reshape(-1))
            np.add.at(err[:, c], flat, ve[..., c].reshape(-1))
        count = np.bincount(flat[np.broadcast_to(inside[:, None, None], (N, L, 4)).reshape(-1)], minlength=table_rows)
        cnt = count[:, None].astype(np.float64)
        r.update(dE=dE, touched=count > 0)
        r["bar"]["dE"] = (1 + gamma(cnt)) * err + gamma(cnt + 1) * mag
    return r


def reference_from_rays(rays_o, rays_d, radius, table, geo, W0, W1, use_dirs=True, grad_image=None, weights_sum=None,
                        defect=None, p32=None):
    """The statement from the rays: polar64 rounded to fp32 (or the given fp32 pair), the input row, then reference().
    Without grad_image the forward only."""
    if p32 is None:
        p32 = polar64(rays_o, rays_d, radius, defect).astype(np.float32)
    x, cell = input_row(p32, rays_d, table, geo, use_dirs, defect)
    r = reference(x, W0, W1, grad_image, weights_sum, cell, np.asarray(table).shape[0], defect)
    r.update(p32=p32, x=x, cell=cell)
    return r


# -------------------------------------------------------------------------------------------------------------- checker
def ratios(ref, got):
    """Worst err / bar of every output in `got` (a dict over OUTPUTS, any subset); a zero bar asks for the exact value and
    anything not finite is over every bar."""
    out = {}
    for k in [k for k in OUTPUTS if k in got]:
        v = np.asarray(got[k], np.float64)
        want, bar = ref[k], ref["bar"][k]
        assert v.shape == want.shape, (k, v.shape, want.shape)
        err = np.abs(v - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(bar > 0, err / np.maximum(bar, 1e-300), np.where(err == 0, 0.0, np.inf))
        q = np.where(np.isfinite(v), q, np.inf)
        out[k] = float(q.max()) if q.size else 0.0
    return out


def check(ref, got, what):
    """Prints the worst err / bar per output and asserts that none exceeds 1."""
    q = ratios(ref, got)
    print(f"err / bar [{what}]: " + "  ".join(f"{k} {v:.3f}" for k, v in q.items()))
    bad = {k: v for k, v in q.items() if not v <= 1.0}
    assert not bad, (what, bad)
    return q


# --------------------------------------------------------------------------------------------------------------- inputs
def make_rays(N, radius, seed):
    """Unit directions and origins inside 0.8 R, fp32."""
    g = np.random.default_rng(seed)
    d = g.standard_normal((N, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = g.standard_normal((N, 3))
    o *= (0.8 * radius * g.random((N, 1)) ** (1 / 3)) / np.linalg.norm(o, axis=1, keepdims=True)
    d = d.astype(np.float32)
    d /= np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True).astype(np.float32)
    return o.astype(np.float32), d.astype(np.float32)


def make_params(geo, C, seed, table_amplitude=0.5):
    """table [rows, 2] uniform in +-amplitude (large enough for the grid columns to matter to every output), W0 / W1 as
    nn.Linear initialises them (uniform, bound 1 / sqrt(fan_in)); fp32."""
    g = np.random.default_rng(seed)
    K = 16 + 2 * geo["L"]
    table = ((g.random((int(geo["offsets"][-1]), 2)) * 2 - 1) * table_amplitude).astype(np.float32)
    W0 = ((g.random((HIDDEN, K)) * 2 - 1) / np.sqrt(K)).astype(np.float32)
    W1 = ((g.random((C, HIDDEN)) * 2 - 1) / np.sqrt(HIDDEN)).astype(np.float32)
    return table, W0, W1
