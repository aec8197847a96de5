"""fp64 reference, error model and checker for the hash table's optimizer pass (csrc/gridencoder.hip: k_grid_bwd_bin,
k_grid_bwd_tile, k_grid_bwd, k_grid_tile_adam; reached through enerf_grid_encode_backward_ex(defer) and
enerf_grid_adam_from_records[_ex]).  Plain numpy, float64; nothing of the package is imported -- the level scale alone
comes from the CPU oracle (oracle.grid_level_params: one fp32 exp2f per level, the value the kernels are built on).

The operation
    per sample b inside [0, 1]^D and level l:  pos = fl32(fma(x, scale_l, 0.5)), cell = floor(pos), frac = pos - cell (exact),
    corner idx (bit d of idx: +1 in dimension d) gets  w = prod_d (bit ? frac_d : 1 - frac_d)  and row = the oracle's
    orc_get_grid_index (dense / tiled: sum_d p_d stride_d; hashed: xor_d p_d prime_d; both uint32, then % level size);
    G[row, c] = sum w * g[b, l, c];   Adam (torch.optim.Adam, no weight decay, no amsgrad) on p / m / v with that G.
Everything after the fp32 `pos` and `frac` is float64 here.

Error model (u = 2^-24, one fp32 rounding to nearest; gamma(k) = k u / (1 - k u) bounds k compounded roundings).
Counted in the kernels' statements (corner_contrib, aggregate_runs, k_grid_bwd_bin / k_grid_tile_adam, scatter_add):
  * a record w * g:  D subtractions (1 - frac_d), D - 1 products of the factors (the first is 1 * f, exact), 1 product
    with g                                                                                   -> 2 D roundings
  * in-wave run aggregation (aggregate_runs): a suffix sum inside each 16-lane row in four doubling steps (run_step<1>,
    <2>, <4>, <8>: one fma(1, other, mine) = one rounded add each; fma(0, other, mine) is exact), then at most three adds
    of the following rows' first lanes.  Every record passes through at most 4 + 3 adds and each add errs by u times the
    magnitude of the partial sum it forms                                                    -> 7
    (run sequentially the 64 lanes of a wavefront would cost 63; the statements give a tree of depth 7)
    so every value that reaches a list or an atomic is within gamma(2 D + 7) * |its terms| of the exact one:  K0 = 2 D + 7
  * path "tile" (binned level, one list per tile, deferred flush): the list is summed in fp64 (2^-53: not counted) and
    rounded to fp32 once -> u |G|; added to a dense gradient of 0.0f exactly
  * path "atomic" (levels too large to bin, batches below the binning threshold): every record is one fp32 atomic add into
    the running sum, at most N of them, each rounding at most u (|base| + A)                 -> adds = N
  * path "spill" (a tile whose list overflowed): part of the records sits in the list (fp64, rounded once: <= u A), the
    rest went into the dense gradient by atomics (< N adds), the two are added once          -> adds = N + 1
  * a value that is added onto an existing fp32 `base` (the owner-range protocol: what the reduce-scatter delivered; pass
    B's flush `o += (float)acc`, its replica lists' atomics, k_grid_tile_adam's `dense + (float)acc`): `adds` more
    roundings of at most u (|base| + A) each -- the caller says how many (1, or the number of replica lists)
    |g_kernel - G| <= gamma(K0) A + u |G| + adds u (|base| + A)       (second-order terms kept: see grad_error_bound)
Multiplications by rec_scale = 0.5 and 1 / scale = 2^-10 are exact (the tests use powers of two only).

Adam's own arithmetic (tile_adam1; -ffp-contract=off, IEEE sqrt and divide), against adam_ref evaluated with the fp32
VALUES of lr, beta1, beta2, eps the kernel receives (1 - beta in fp32 is exact for 0.9f and 0.99f):
  m = fma(g - m, 1 - b1, m): fl(g - m) errs by u |g - m| = 10 u |m' - m|, times 0.1, plus the fma's u |m'|  <= 3 u max(|m|, |m'|)
  v = fma((1 - b2) g, g, v b2): three roundings of non-negative terms                                        <= 3 u v'
  p = p - step_size * (m / (sqrt(v) * inv_bc2_sqrt + eps)): seven roundings inside the update D (step_size and
      inv_bc2_sqrt are rounded on the host), |D| <= 2.5 lr whatever the gradient (|m^| / sqrt(v^) is bounded for
      betas (0.9, 0.99)), so 7 u |D| + the moments' own 3 u each <= 0.5 u at lr <= 1e-2, and the subtraction's u |p'|:
      within 4 ulp of p as long as |p| >= 0.25, which the tests' initial parameters guarantee (|p| in [0.25, 1)).
One ulp of x is at least u |x|, so "4 ulp of max(|old|, |new|)" covers each of the three with room to spare; the gradient's
own error is carried through by evaluating adam_ref at G - dG, G and G + dG (adam_bounds)."""
import numpy as np

U = 2.0 ** -24
PRIMES = (1, 2654435761, 805459861, 3674653429, 2097192037, 1434869437, 2165219737)
M32 = np.uint64(0xFFFFFFFF)
TILE_ELEMS = 4096                    # elements of one table tile (rows per tile R = TILE_ELEMS / C)
MAX_BINS = 512                       # record lists per level the cursor array holds


def level_params(level, S, H):
    """(fp32 scale as float, resolution) of a level: the CPU oracle's values."""
    from oracle import oracle as O
    return O.grid_level_params(level, S, H)


def corners(x, offsets, D, S, H, gridtype):
    """Per level: dict(valid [B] bool, cell [B] int64 (one number per cell), rows [B, 2^D] int64 within the level,
    w [B, 2^D] float64).  x: [B, D] float32."""
    x32 = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, D)
    valid = ~((x32 < 0) | (x32 > 1)).any(axis=1)            # out-of-range points contribute nothing
    out = []
    for level in range(len(offsets) - 1):
        scale, res = level_params(level, S, H)
        size = int(offsets[level + 1]) - int(offsets[level])
        # fma(x, scale, 0.5) rounded once: x * scale is exact in fp64 (24 + 24 bits) and so is the sum as long as
        # x * scale >= 2^-6 (its last bit then lies at or above 2^-53, the last bit of a double in [0.5, 1)); the
        # generated inputs keep x >= 0.01 > 2^-6 / 7, 7 being the smallest scale
        pos = (x32.astype(np.float64) * np.float64(np.float32(scale)) + 0.5).astype(np.float32)
        fl = np.floor(pos)
        frac = (pos - fl).astype(np.float64)                # fp32 subtraction, exact
        pg = np.where(valid[:, None], fl, 0).astype(np.uint64)
        # strides of the dimensions the index loop folds in (uint32 arithmetic, as in orc_get_grid_index)
        strides, stride = [], 1
        for d in range(D):
            if stride <= size:
                strides.append(stride)
                stride = (stride * (res + 1)) & 0xFFFFFFFF
            else:
                strides.append(None)
        hashed = gridtype == 0 and stride > size
        rows = np.empty((x32.shape[0], 1 << D), np.int64)
        w = np.ones((x32.shape[0], 1 << D), np.float64)
        for idx in range(1 << D):
            index = np.zeros(x32.shape[0], np.uint64)
            for d in range(D):
                bit = (idx >> d) & 1
                w[:, idx] *= frac[:, d] if bit else 1.0 - frac[:, d]
                p = pg[:, d] + np.uint64(bit)
                if hashed:
                    index ^= (p * np.uint64(PRIMES[d])) & M32
                elif strides[d] is not None:
                    index = (index + p * np.uint64(strides[d])) & M32
            rows[:, idx] = (index % np.uint64(size)).astype(np.int64)
        cell = np.zeros(x32.shape[0], np.int64)
        for d in range(D):
            cell = cell * (res + 2) + pg[:, d].astype(np.int64)
        out.append({"valid": valid, "cell": cell, "rows": rows, "w": w})
    return out


def grid_grad_ref(x, g, offsets, D, C, S, H, gridtype, cs=None):
    """x [B, D] fp32, g [L, B, C] (fp32 values) -> (G, A [rows, C] float64, N [rows] int64): per table element the sum of
    all corner contributions w * g, of their magnitudes, and their number."""
    L = len(offsets) - 1
    g = np.asarray(g, dtype=np.float64).reshape(L, -1, C)
    total = int(offsets[-1])
    G = np.zeros((total, C)); A = np.zeros((total, C)); N = np.zeros(total, np.int64)
    cs = cs if cs is not None else corners(x, offsets, D, S, H, gridtype)
    for level, c in enumerate(cs):
        ok = c["valid"]
        lo, hi = int(offsets[level]), int(offsets[level + 1])
        rows = c["rows"][ok].reshape(-1)
        N[lo:hi] += np.bincount(rows, minlength=hi - lo)
        for ch in range(C):
            t = (c["w"][ok] * g[level, ok, ch][:, None]).reshape(-1)
            G[lo:hi, ch] += np.bincount(rows, weights=t, minlength=hi - lo)
            A[lo:hi, ch] += np.bincount(rows, weights=np.abs(t), minlength=hi - lo)
    return G, A, N


def adam_ref(p, m, v, g, lr, b1, b2, eps, t):
    """torch.optim.Adam's update (no weight decay, no amsgrad) in float64 -> (p, m, v)."""
    p, m, v, g = (np.asarray(a, np.float64) for a in (p, m, v, g))
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    step_size = lr / (1.0 - b1 ** t)
    denom = np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps
    return p - step_size * (m / denom), m, v


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


def grad_error_bound(A, N, G, path, D=3, base=None, adds=0):
    """A-priori bound on |g_kernel - G| per element (module docstring).  A, G: [rows, C]; N: [rows]; path: "tile",
    "atomic" or "spill"; base: fp32 values the sum is added onto (None: zeros), with `adds` (scalar or [rows]) roundings."""
    A = np.asarray(A, np.float64); G = np.abs(np.asarray(G, np.float64))
    Nc = np.asarray(N, np.float64)[:, None]
    e0 = gamma(2 * D + 7) * A                     # K0 = 2 D + 7: weight product, w * g, run aggregation
    A1 = A + e0                                   # magnitudes of the values as the kernel holds them
    b = 0.0 if base is None else np.abs(np.asarray(base, np.float64))
    n_adds = np.asarray(adds, np.float64)
    n_adds = n_adds[:, None] if n_adds.ndim == 1 else n_adds
    if path == "tile":                            # K = 2 D + 7, one rounding of the fp64 list sum
        pass
    elif path == "atomic":                        # K = 2 D + 7 + N: N sequential fp32 adds
        n_adds = n_adds + Nc
    elif path == "spill":                         # K = 2 D + 7 + N + 1: list part rounded once, < N atomics, one add
        n_adds = n_adds + Nc + 1.0
    else:
        raise ValueError(path)
    return e0 + U * (G + e0) + gamma(n_adds) * (b + A1)


def ulp32(x):
    """One unit in the last place of fp32 at |x| (normal range)."""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


def adam_bounds(p, m, v, G, dG, lr, b1, b2, eps, t):
    """Reference update at G with the tolerances the gradient's bound dG leaves: -> dict name -> (ref, tol), tol = the spread of
    adam_ref over G - dG, G, G + dG plus 4 ulp of fp32 for the kernel's own arithmetic (module docstring)."""
    c = adam_ref(p, m, v, G, lr, b1, b2, eps, t)
    lo = adam_ref(p, m, v, G - dG, lr, b1, b2, eps, t)
    hi = adam_ref(p, m, v, G + dG, lr, b1, b2, eps, t)
    out = {}
    for name, old, k in (("p", p, 0), ("m", m, 1), ("v", v, 2)):
        spread = np.maximum(np.abs(lo[k] - c[k]), np.abs(hi[k] - c[k]))
        out[name] = (c[k], spread + 4.0 * ulp32(np.maximum(np.abs(np.asarray(old, np.float64)), np.abs(c[k]))))
    return out


def close(got, ref_tol):
    """Elementwise: |got - ref| <= tol -> bool array."""
    ref, tol = ref_tol
    return np.abs(np.asarray(got, np.float64) - ref) <= tol


def compare_step(got, p, m, v, G, dG, lr, b1, b2, eps, t, family, what=""):
    """The GPU tests' comparison of one optimizer step.  got = (p, m, v) after the step, p / m / v before it (the
    kernel's own fp32 values), G / dG the reference gradient and its bound.  family "one": p, m, v held at every element;
    "signed": m and v at every element, p wherever dG <= 1e-3 |G| and elsewhere to |dp| <= 2.5 lr.
    -> list of failure descriptions (empty: passed)."""
    b = adam_bounds(p, m, v, G, dG, lr, b1, b2, eps, t)
    fails = []
    for k, name in ((1, "m"), (2, "v")):
        ok = close(got[k], b[name])
        if not ok.all():
            i = int(np.argmax(np.abs(np.asarray(got[k], np.float64) - b[name][0]) / b[name][1]))
            fails.append(f"{what}{name}: {int((~ok).sum())} elements off, worst at {i}: got {np.ravel(got[k])[i]!r} "
                         f"ref {np.ravel(b[name][0])[i]!r} tol {np.ravel(b[name][1])[i]!r}")
    okp = close(got[0], b["p"])
    if family == "signed":
        loose = dG > 1e-3 * np.abs(G)
        okp = np.where(loose, np.abs(np.asarray(got[0], np.float64) - b["p"][0]) <= 2.5 * lr, okp)
    if not okp.all():
        i = int(np.argmax(np.where(okp, 0.0, np.abs(np.asarray(got[0], np.float64) - b["p"][0]))))
        fails.append(f"{what}p: {int((~okp).sum())} elements off, worst at {i}: got {np.ravel(got[0])[i]!r} "
                     f"ref {np.ravel(b['p'][0])[i]!r} tol {np.ravel(b['p'][1])[i]!r}")
    return fails


# ---- table geometry as the kernels derive it from `offsets` (bin_plan, bin_cap) ------------------------------------
def bins_limit(R):
    q = (1 << 19) // R
    return 256 if q <= 256 else min(q, MAX_BINS)


def bin_plan(offsets, level, C, min_tiles):
    """-> (tiles, replicas, bins); bins == 0: the level is not binned (atomic kernel + dense gradient)."""
    R = TILE_ELEMS // C
    tiles = -(-(int(offsets[level + 1]) - int(offsets[level])) // R)
    replicas = 1 if tiles >= min_tiles else -(-min_tiles // tiles)
    bins = tiles * replicas if tiles * replicas <= bins_limit(R) else 0
    return tiles, replicas, bins


def bin_cap(D, reserve_B, bins):
    """Records one list holds: cap = ((2 * 2^D * reserve_B) / bins) & ~1."""
    return ((2 * (1 << D) * reserve_B) // bins) & ~1


def tile_of_element(offsets, C):
    """Per table row: (level, tile within the level)."""
    R = TILE_ELEMS // C
    level = np.zeros(int(offsets[-1]), np.int64); tile = np.zeros(int(offsets[-1]), np.int64)
    for l in range(len(offsets) - 1):
        lo, hi = int(offsets[l]), int(offsets[l + 1])
        level[lo:hi] = l
        tile[lo:hi] = np.arange(hi - lo) // R
    return level, tile


def tile_records(cs, offsets, C, heads_only=False):
    """Per level: records per tile.  heads_only=False: an upper bound (every corner of every valid sample, no run
    aggregated); True: a lower bound (2^D per valid sample whose cell differs from the previous sample's -- such a sample
    heads a run whatever the wavefront boundaries)."""
    R = TILE_ELEMS // C
    out = []
    for l, c in enumerate(cs):
        tiles = -(-(int(offsets[l + 1]) - int(offsets[l])) // R)
        take = c["valid"].copy()
        if heads_only:
            prev_same = np.zeros_like(take)
            prev_same[1:] = (c["cell"][1:] == c["cell"][:-1]) & c["valid"][:-1]
            take &= ~prev_same
        out.append(np.bincount((c["rows"][take] // R).reshape(-1), minlength=tiles))
    return out


# ---- the tests' inputs ----------------------------------------------------------------------------------------------
def make_samples(rng, B, D, slab=None):
    """B samples (fp32): half uniform in [0.01, 1)^D, half rays of 64 closely spaced samples in ray order, one sample
    outside [0, 1].  slab = (lo, hi): every sample's last coordinate uniform in [lo, hi), random order (the spill case)."""
    if slab is not None:
        x = rng.uniform(0.01, 1.0, (B, D))
        x[:, D - 1] = rng.uniform(slab[0], slab[1], B)
    else:
        nray = (B // 2) // 64
        o = rng.uniform(0.05, 0.6, (nray, 1, D))
        d = rng.normal(size=(nray, 1, D))
        d /= np.linalg.norm(d, axis=2, keepdims=True)
        t = np.arange(64)[None, :, None] * (0.35 / 64 / 16)          # a ray spans ~0.02: runs on every level
        rays = np.clip(o + np.abs(d) * t, 0.01, 0.999).reshape(-1, D)
        x = np.concatenate([rng.uniform(0.01, 1.0, (B - rays.shape[0], D)), rays])
    x = x.astype(np.float32)
    x = np.maximum(x, np.float32(0.01))
    x[x >= 1.0] = np.float32(0.999)
    if slab is None:
        x[B // 3, 0] = np.float32(1.5)                                # the out-of-range sample
    return x


def make_grads(rng, family, B, L, C, step):
    """[L, B, C] fp32.  "one": g = s(channel, step) * uniform(0.5, 1.5) (A == |G|); "signed": N(0, 1)."""
    if family == "one":
        s = np.where((np.arange(C) + step) % 2 == 0, 1.0, -1.0)
        return (s[None, None, :] * rng.uniform(0.5, 1.5, (L, B, C))).astype(np.float32)
    return rng.normal(size=(L, B, C)).astype(np.float32)


def make_params(rng, shape):
    """Non-zero start: |p| in [0.25, 1), random sign (the p tolerance relies on |p| >= 0.25)."""
    return (rng.uniform(0.25, 1.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def compare_identical(got, before, keep, what=""):
    """Bit-identity of fp32 arrays where `keep` (bool, broadcastable) is set -> list of failure descriptions."""
    fails = []
    for name, a, b in zip(("p", "m", "v"), got, before):
        a = np.ascontiguousarray(a, np.float32).view(np.uint32)
        b = np.ascontiguousarray(b, np.float32).view(np.uint32)
        bad = (a != b) & keep
        if bad.any():
            fails.append(f"{what}{name}: {int(bad.sum())} elements changed that must be bit-identical, first at "
                         f"{int(np.argmax(bad.reshape(-1)))}")
    return fails


def compare_range_step(got, p, m, v, G, dG, lo, hi, lr, b1, b2, eps, t, family, what=""):
    """Owner range: flat elements [lo, hi) follow the reference at gradient G (the caller has applied rec_scale),
    everything outside is bit-identical to before."""
    inside = np.zeros(np.asarray(p).size, bool)
    inside[lo:hi] = True
    inside = inside.reshape(np.asarray(p).shape)
    sel = [np.asarray(a).reshape(-1)[lo:hi] for a in (*got, p, m, v, G, dG)]
    fails = compare_step(sel[0:3], sel[3], sel[4], sel[5], sel[6], sel[7], lr, b1, b2, eps, t, family, what + "range ")
    return fails + compare_identical(got, (p, m, v), ~inside, what + "outside ")


def compare_small(got, p, m, v, g, lr, b1, b2, eps, t, what=""):
    """A small tensor: dense fp32 gradient, no gradient error -- the 4 ulp of Adam's own arithmetic alone."""
    return compare_step(got, p, m, v, np.asarray(g, np.float64), np.zeros(np.asarray(g).shape), lr, b1, b2, eps, t, "one",
                        what)


# ---- the cases: shared by the host conditions (tests/test_table_adam_ref.py) and the GPU tests -----------------------
S_LOG2, H_BASE = 1.0, 8              # per_level_scale = 2, base_resolution = 8
B1, B2, EPS = float(np.float32(0.9)), float(np.float32(0.99)), float(np.float32(1e-15))
SMALL_SIZES = (1, 7, 64, 2049, 4096, 33, 1024, 3)
GEOMS = {
    # rows 736, 4920, 35944, 274632, 2^19, 2^19: 1, 3, 18, 135, 256, 256 tiles of 2048 rows, short last tiles on levels 0-3
    "A": dict(num_levels=6, log2_hashmap_size=19, C=2, D=3),
    # last level 2^20 rows = 512 tiles > 256 lists: not binned
    "B": dict(num_levels=5, log2_hashmap_size=20, C=2, D=3),
    "C1": dict(num_levels=4, log2_hashmap_size=17, C=1, D=3),     # R = 4096: 1, 2, 9, 32 tiles (last level hashed)
    "C4": dict(num_levels=4, log2_hashmap_size=17, C=4, D=3),     # R = 1024: 1, 5, 36, 128 tiles
    "C8": dict(num_levels=4, log2_hashmap_size=19, C=8, D=3),     # R = 512: 2, 10, 71, 537 tiles (537 > 512 lists: atomics)
    "D2": dict(num_levels=4, log2_hashmap_size=12, C=2, D=2),     # rows 88, 296, 1096, 4096 (hashed, 2 tiles)
}
FULL = 8192


def lr_of(step):
    """The table's learning rate at optimizer step `step` (0-based): 1e-2 falling, as the fp32 value the kernel gets."""
    return float(np.float32(1e-2 * 0.8 ** step))


# steps: per optimizer step the batch sizes of the backward calls that join its flush ([]: nothing pending -- the pass
# runs over a dense gradient the test wrote itself)
CASES = {
    "A_min1": dict(geom="A", min_tiles=1, steps=[[FULL], [], [FULL]], layout=1, seed=101),
    "A_min8": dict(geom="A", min_tiles=8, steps=[[FULL, FULL], [FULL, 1000], [FULL]], layout=1, seed=102),
    "B": dict(geom="B", min_tiles=8, steps=[[FULL]] * 3, layout=0, seed=103),
    "C1": dict(geom="C1", min_tiles=8, steps=[[FULL]] * 3, layout=1, seed=104),
    "C4": dict(geom="C4", min_tiles=8, steps=[[FULL]] * 3, layout=1, seed=105),
    "C8": dict(geom="C8", min_tiles=8, steps=[[FULL]] * 3, layout=1, seed=106),
    "D2": dict(geom="D2", min_tiles=8, steps=[[FULL]] * 3, layout=1, seed=107),
    "D2_tiled": dict(geom="D2", min_tiles=1, steps=[[FULL]] * 3, layout=1, seed=108, gridtype=1),
    # every sample's z inside level-2 cell 12 (z * 31 + 0.5 in [12, 13)): levels 2 and 3 receive all their records in two
    # or three tiles and must overflow; on level 1 the two z layers (6 and 7) lie on either side of the first tile's end,
    # so neither of its lists overflows and the level keeps the tile path beside the spilled ones
    "spill": dict(geom="A", min_tiles=1, steps=[[FULL]] * 3, layout=1, seed=109, slab=(11.7 / 31, 12.3 / 31)),
    "small8": dict(geom="A", min_tiles=8, steps=[[FULL]] * 3, layout=1, seed=110, n_small=8),
    "small5": dict(geom="A", min_tiles=8, steps=[[FULL]] * 3, layout=1, seed=111, n_small=5),
    "small1": dict(geom="A", min_tiles=8, steps=[[FULL]] * 3, layout=1, seed=112, n_small=1),
    "amp": dict(geom="A", min_tiles=8, steps=[[FULL]] * 3, layout=1, seed=113, n_small=2),
    "range": dict(geom="A", min_tiles=8, steps=[[FULL]] * 3, layout=1, seed=114),
}
FAMILIES = ("one", "signed")


def geometry(name):
    """-> (offsets int32 [L + 1], L, C, D) of a GEOMS entry."""
    from oracle import oracle as O
    g = GEOMS[name]
    offsets, _ = O.grid_offsets(input_dim=g["D"], num_levels=g["num_levels"], level_dim=g["C"], per_level_scale=2.0,
                                base_resolution=H_BASE, log2_hashmap_size=g["log2_hashmap_size"])
    return offsets, g["num_levels"], g["C"], g["D"]


def bin_pts(C):
    """Samples per workgroup of the binning pass (a sample's replica list is (b // bin_pts) % replicas)."""
    return 512 if C <= 4 else 256


def step_inputs(case, family, step):
    """The backward calls of one optimizer step -> list of (x [B, D] fp32, g [L, B, C] fp32); deterministic."""
    c = CASES[case]
    _, L, C, D = geometry(c["geom"])
    out = []
    for k, B in enumerate(c["steps"][step]):
        rng = np.random.default_rng([c["seed"], FAMILIES.index(family), step, k])
        out.append((make_samples(rng, B, D, c.get("slab")), make_grads(rng, family, B, L, C, step)))
    return out


def dense_step_gradient(case, family, step):
    """The dense gradient of a step with nothing pending: fp32 [rows, C], a third of the rows non-zero."""
    c = CASES[case]
    offsets, L, C, D = geometry(c["geom"])
    rng = np.random.default_rng([c["seed"], FAMILIES.index(family), step, 99])
    g = make_grads(rng, family, int(offsets[-1]), 1, C, step)[0]
    g[rng.uniform(size=g.shape[0]) > 1.0 / 3.0] = 0.0
    return g


def step_reference(case, family, step, min_tiles=None, binned=True):
    """Reference gradient of one optimizer step and its a-priori bound.
    -> dict(G, A, N, dG, path [rows] (0 tile, 1 atomic, 2 spill), records_hi / records_lo (per level, per list / per tile),
            caps (per level; 0: not binned), plans).  binned=False: the whole gradient went through the atomic kernel."""
    c = CASES[case]
    offsets, L, C, D = geometry(c["geom"])
    min_tiles = c["min_tiles"] if min_tiles is None else min_tiles
    calls = step_inputs(case, family, step)
    total = int(offsets[-1])
    G = np.zeros((total, C)); A = np.zeros((total, C)); N = np.zeros(total, np.int64)
    plans = [bin_plan(offsets, l, C, min_tiles) if binned else (0, 1, 0) for l in range(L)]
    reserve = sum(x.shape[0] for x, _ in calls)
    caps = [bin_cap(D, reserve, pl[2]) if pl[2] else 0 for pl in plans]
    R = TILE_ELEMS // C
    rec_hi = [np.zeros((max(pl[0], 1), pl[1]), np.int64) for pl in plans]
    rec_lo = [np.zeros(max(pl[0], 1), np.int64) for pl in plans]
    for x, g in calls:
        cs = corners(x, offsets, D, S_LOG2, H_BASE, c.get("gridtype", 0))
        g1, a1, n1 = grid_grad_ref(x, g, offsets, D, C, S_LOG2, H_BASE, c.get("gridtype", 0), cs=cs)
        G += g1; A += a1; N += n1
        chunk = np.arange(x.shape[0]) // bin_pts(C)
        for l, cl in enumerate(cs):
            tiles, replicas, bins = plans[l]
            if not bins:
                continue
            ok = cl["valid"]
            lists = (cl["rows"][ok] // R) * replicas + (chunk[ok] % replicas)[:, None]
            rec_hi[l] += np.bincount(lists.reshape(-1), minlength=tiles * replicas).reshape(tiles, replicas)
            rec_lo[l] += tile_records([cl], offsets[l:l + 2], C, heads_only=True)[0]
    path = np.zeros(total, np.int64)
    for l in range(L):
        lo, hi = int(offsets[l]), int(offsets[l + 1])
        if not plans[l][2]:
            path[lo:hi] = 1
        else:
            over = (rec_hi[l] > caps[l]).any(axis=1)                 # a list of the tile may have overflowed
            path[lo:hi] = np.where(over[np.arange(hi - lo) // R], 2, 0)
    bounds = [grad_error_bound(A, N, G, p, D=D) for p in ("tile", "atomic", "spill")]
    dG = np.choose(path[:, None], bounds)
    return dict(G=G, A=A, N=N, dG=dG, path=path, records_hi=rec_hi, records_lo=rec_lo, caps=caps, plans=plans,
                offsets=offsets, C=C, D=D, L=L)


# ---- owner range (the sharded data-parallel tail) ------------------------------------------------------------------------
REC_SCALE = 0.5
# flat element ranges [lo, hi) of geometry A (C = 2: element = 2 * row + channel), all multiples of 4
RANGES = {
    "inside": (2 * (41600 + 10 * 2048 + 100), 2 * (41600 + 10 * 2048 + 1500)),       # strictly inside tile 10 of level 3
    "across": (2 * (5656 + 5 * 2048 + 1000), 2 * (316232 + 7 * 2048 + 1024)),         # mid tile 5 of level 2 .. mid tile 7 of level 4
    "level0": (0, 2 * 736),                                                           # level 0 alone: its replica lists are "mine"
    "dense": (2 * (5656 + 5 * 2048 + 1000), 2 * (316232 + 7 * 2048 + 1024)),          # same, batch below the binning threshold
}


def range_p0(family, step):
    """What the reduce-scatter delivered: fp32 [rows, C]; the one-signed family keeps the gradients' sign per channel."""
    offsets, L, C, D = geometry(CASES["range"]["geom"])
    rng = np.random.default_rng([CASES["range"]["seed"], FAMILIES.index(family), step, 77])
    return make_grads(rng, family, int(offsets[-1]), 1, C, step)[0]


def range_reference(name, family, step):
    """step_reference of the "range" case plus the owner-range protocol's expectations: P0, `whole` (elements of binned
    tiles wholly inside the range: their lists wait for the optimizer pass), the dense buffer after the backward
    (dense, d_dense) and the gradient Adam must see inside the range (G_adam = rec_scale * (P0 + G), dG_adam)."""
    r = step_reference("range", family, step, binned=name != "dense")
    lo, hi = RANGES[name]
    offsets, C, D = r["offsets"], r["C"], r["D"]
    R = TILE_ELEMS // C
    P0 = range_p0(family, step)
    total = int(offsets[-1])
    whole = np.zeros(total, bool)
    adds = np.ones(total)
    for l in range(r["L"]):
        o0, o1 = int(offsets[l]), int(offsets[l + 1])
        tiles, replicas, bins = r["plans"][l]
        if not bins:
            adds[o0:o1] = 0                                   # (atomic path: its N adds already count the base)
            continue
        adds[o0:o1] = replicas                                # pass B flushes replica lists with one atomic each
        for t in range(tiles):
            t_lo, t_hi = (o0 + t * R) * C, min(o0 + (t + 1) * R, o1) * C
            if t_lo >= lo and t_hi <= hi:
                whole[o0 + t * R:min(o0 + (t + 1) * R, o1)] = True
    adds[whole] = 1                                           # k_grid_tile_adam: dense + (float)acc, once
    bounds = [grad_error_bound(r["A"], r["N"], r["G"], p, D=D, base=P0, adds=adds) for p in ("tile", "atomic", "spill")]
    d = np.choose(r["path"][:, None], bounds)
    tot = P0.astype(np.float64) + r["G"]
    r.update(P0=P0, whole=whole, dense=np.where(whole[:, None], P0.astype(np.float64), tot),
             d_dense=np.where(whole[:, None], 0.0, d), G_adam=REC_SCALE * tot, dG_adam=REC_SCALE * d, lo=lo, hi=hi)
    return r
