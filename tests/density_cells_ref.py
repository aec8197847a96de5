"""Exact host statement of which cells a density-grid update evaluates and where it queries them
(csrc/density_update.hip: enerf_density_grid_cells; csrc/sweep_points.h).  Plain numpy; nothing of the package is
imported and no source of the library is compiled for the host -- the statement is written from the documented
semantics, so that comparing the kernels with it does not compare the code with itself.

Nothing in the pass is random once the seed is given:

  generator   mix64 is the splitmix64 finaliser; with G = 0x9e3779b97f4a7c15 and all sums modulo 2^64
                  a = mix64(seed + G (2 c + 1)),  b = mix64(a + G (2 c + 2) + seed)
              rand4(seed, c) = (a mod 2^32, a >> 32, b mod 2^32, b >> 32)
  occupied    per cascade, the cell indices (Morton order: the grid's own) with density > 0, ascending; -1 (untrained), 0,
              -0.0 and NaN are not occupied, a positive denormal and +inf are
  partial     point i of C * 2 n: cascade i // 2n, j = i % 2n, words of rand4(seed ^ 0x5bd1e995, i); the uniform cell is
              w0 & (H^3 - 1); for j >= n in a cascade with cnt > 0 occupied cells, occupied cell number (w1 * cnt) >> 32
              instead; key = cascade << 3 log2 H | cell.  The keys are sorted ascending; sorted point p is jittered
              with rand4(seed, p) -- the counter AFTER the sort
  full sweep  point p of C * H^3: cascade p // H^3, cell p % H^3 with x fastest; Morton index of (x, y, z); rand4(seed, p)
  position    per axis, in float32, every operation rounded on its own (the library is built without contraction and with
              correctly rounded division):  inv = 1 / (H - 1);  u = (w >> 8) * 2^-24;
                  ((2 * x) * inv - 1) * span + (u * 2 - 1) * half
              axis a takes word a.  bound_c = min(2^cascade, bound), half = bound_c / H and span = bound_c - half are
              formed in double and rounded to float32 once (nerf/renderer.py:498-501 of the reference)
  sort        buckets of 2^low consecutive key values: key_bits = 3 log2 H + ceil(log2 C), low = max(12, key_bits - 12)
              (at most 14), nb = ceil(C H^3 / 2^low) <= 4096 buckets.  The geometry does not change the answer -- np.sort is
              the statement -- it says which branch of the sort a case reaches (`sort_geometry`).

`CASES` are the shapes tests/test_gpu_density_cells_exact.py runs, each with the precondition that makes it reach its
branch; tests/test_density_cells_ref.py asserts those preconditions on the statement alone."""
import numpy as np

G64 = np.uint64(0x9E3779B97F4A7C15)
SELECT_XOR = 0x5BD1E995
OCC_BLOCK = 4096            # cells per workgroup of the occupied-list passes
SORT_CHUNK = 8192           # keys per workgroup of the sort's count / scatter passes
SORT_MAX_BUCKETS = 4096
SORT_MAX_LOW = 14
HEAVY_ABOVE = 64            # a value that occurs more often is written by the whole workgroup ...
HEAVY_SLOTS = 64            # ... while the table of such values has room
IDX_SENTINEL = -0x5A5A5A5B  # what the tests fill the index buffer with (never a Morton index)
PAD = 64                    # elements both output buffers are over-allocated by


def _u64(v):
    return np.asarray(v, dtype=np.uint64)


def mix64(z):
    """splitmix64 finaliser on uint64, modulo 2^64 (a scalar comes back as an array of one)."""
    z = np.atleast_1d(_u64(z)).copy()
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def rand4(seed, counter):
    """-> uint32 [n, 4]: the four words of every counter."""
    c = _u64(counter).reshape(-1)
    s = np.uint64(int(seed) & (2 ** 64 - 1))
    with np.errstate(over="ignore"):
        a = mix64(s + G64 * (np.uint64(2) * c + np.uint64(1)))
        b = mix64(a + G64 * (np.uint64(2) * c + np.uint64(2)) + s)
    m = np.uint64(0xFFFFFFFF)
    return np.stack([a & m, a >> np.uint64(32), b & m, b >> np.uint64(32)], axis=1).astype(np.uint32)


def log2_exact(H):
    l = int(H).bit_length() - 1
    assert H == 1 << l, H
    return l


def morton3(x, y, z):
    """bit k of x -> bit 3k, of y -> 3k + 1, of z -> 3k + 2."""
    x, y, z = (np.asarray(v, np.uint32) for v in (x, y, z))
    out = np.zeros(x.shape, np.uint32)
    for k in range(10):
        out |= ((x >> np.uint32(k)) & np.uint32(1)) << np.uint32(3 * k)
        out |= ((y >> np.uint32(k)) & np.uint32(1)) << np.uint32(3 * k + 1)
        out |= ((z >> np.uint32(k)) & np.uint32(1)) << np.uint32(3 * k + 2)
    return out


def morton3_invert(idx):
    idx = np.asarray(idx, np.uint32)
    x, y, z = (np.zeros(idx.shape, np.uint32) for _ in range(3))
    for k in range(10):
        x |= ((idx >> np.uint32(3 * k)) & np.uint32(1)) << np.uint32(k)
        y |= ((idx >> np.uint32(3 * k + 1)) & np.uint32(1)) << np.uint32(k)
        z |= ((idx >> np.uint32(3 * k + 2)) & np.uint32(1)) << np.uint32(k)
    return x, y, z


def cascade_geometry(cas, bound, H):
    """(span, half) as float32, each formed in double and rounded once."""
    b = min(float(2 ** cas), float(np.float32(bound)))
    half = b / float(H)
    return np.float32(b - half), np.float32(half)


def positions(cas, x, y, z, words, bound, H, word_of_axis=(0, 1, 2)):
    """float32 [n, 3] query positions of cells (x, y, z) of cascades `cas` (array), jittered by `words` [n, 4]."""
    f = np.float32
    cas = np.asarray(cas, np.int64)
    geo = np.array([cascade_geometry(c, bound, H) for c in range(8)], np.float32)
    span, half = geo[cas, 0], geo[cas, 1]
    inv = f(1) / f(H - 1)
    out = np.empty((cas.shape[0], 3), np.float32)
    for a, c in enumerate((x, y, z)):
        t = f(2) * np.asarray(c).astype(np.float32)
        t = t * inv
        t = t - f(1)
        t = t * span
        u = (words[:, word_of_axis[a]] >> np.uint32(8)).astype(np.float32) * f(2.0 ** -24)
        j = u * f(2)
        j = j - f(1)
        j = j * half
        out[:, a] = t + j
    assert out.dtype == np.float32
    return out


def occupied(grid):
    """list over the cascades of ascending uint32 cell indices with grid > 0."""
    with np.errstate(invalid="ignore"):
        return [np.flatnonzero(g > 0).astype(np.uint32) for g in np.asarray(grid)]


def select_keys(grid, C, H, n, seed, occ=None, draw_over=lambda cnt: cnt):
    """uint32 [C * 2n] keys in drawing order.  `occ` overrides the occupied lists and `draw_over` the range of the occupied
    draw: both exist for the seeded defects of tests/test_density_cells_ref.py only."""
    bits = 3 * log2_exact(H)
    H3 = 1 << bits
    occ = occupied(grid) if occ is None else occ
    i = np.arange(C * 2 * n, dtype=np.uint64)
    w = rand4((int(seed) & (2 ** 64 - 1)) ^ SELECT_XOR, i)
    cas = (i // np.uint64(2 * n)).astype(np.uint32)
    j = (i % np.uint64(2 * n)).astype(np.uint32)
    cell = w[:, 0] & np.uint32(H3 - 1)
    for c in range(C):
        cnt = len(occ[c])
        if cnt == 0:
            continue
        m = (cas == c) & (j >= n)
        pick = (w[m, 1].astype(np.uint64) * np.uint64(draw_over(cnt))) >> np.uint64(32)
        cell[m] = occ[c][pick.astype(np.int64)]
    return (cas << np.uint32(bits)) | cell


def cells_from_sorted_keys(keys, H, bound, seed, counters=None, word_of_axis=(0, 1, 2)):
    """sorted keys -> (int32 Morton indices, float32 [P, 3] positions).  `counters` (default: 0 .. P - 1, the position
    after the sort) and `word_of_axis` exist for the seeded defects only."""
    bits = 3 * log2_exact(H)
    keys = np.asarray(keys, np.uint32)
    idx = keys & np.uint32((1 << bits) - 1)
    cas = keys >> np.uint32(bits)
    x, y, z = morton3_invert(idx)
    counters = np.arange(keys.shape[0], dtype=np.uint64) if counters is None else counters
    xyz = positions(cas, x, y, z, rand4(seed, counters), bound, H, word_of_axis)
    return idx.astype(np.int32), xyz


def cells_partial(grid, C, H, bound, n, seed):
    return cells_from_sorted_keys(np.sort(select_keys(grid, C, H, n, seed)), H, bound, seed)


def cells_full(C, H, bound, seed):
    H3 = H ** 3
    p = np.arange(C * H3, dtype=np.uint64)
    cas, cell = p // np.uint64(H3), p % np.uint64(H3)
    x, y, z = cell % np.uint64(H), (cell // np.uint64(H)) % np.uint64(H), cell // np.uint64(H * H)
    xyz = positions(cas, x, y, z, rand4(seed, p), bound, H)
    return morton3(x, y, z).astype(np.int32), xyz


def sort_geometry(C, H):
    """(key_bits, low, nb) of the partial update's sort."""
    bits = 3 * log2_exact(H)
    key_bits = bits + int(C - 1).bit_length()                  # ceil(log2 C) bits of cascade above the Morton index
    low = max(12, key_bits - 12)
    nb = -(-(C << bits) // (1 << low))
    return key_bits, low, nb


def value_counts(keys):
    """(values, how often each occurs) of a key array."""
    return np.unique(np.asarray(keys), return_counts=True)


def compare(got_idx, got_xyz, want_idx, want_xyz):
    """The comparator of the exact tests: Morton indices element for element, positions bit for bit.  -> None when equal,
    else a one-line description of the first difference."""
    got_idx, want_idx = np.asarray(got_idx), np.asarray(want_idx)
    got_xyz, want_xyz = np.asarray(got_xyz, np.float32), np.asarray(want_xyz, np.float32)
    if got_idx.shape != want_idx.shape or got_xyz.shape != want_xyz.shape:
        return f"shapes {got_idx.shape} {got_xyz.shape}, statement {want_idx.shape} {want_xyz.shape}"
    bad = np.flatnonzero(got_idx != want_idx)
    if bad.size:
        p = int(bad[0])
        return f"{bad.size} indices differ, first at point {p}: {int(got_idx[p])}, statement {int(want_idx[p])}"
    a = np.ascontiguousarray(got_xyz).view(np.uint32).reshape(-1, 3)
    b = np.ascontiguousarray(want_xyz).view(np.uint32).reshape(-1, 3)
    bad = np.flatnonzero((a != b).any(axis=1))
    if bad.size:
        p = int(bad[0])
        return (f"{bad.size} positions differ in their bits, first at point {p}: {got_xyz.reshape(-1, 3)[p].tolist()}, "
                f"statement {want_xyz.reshape(-1, 3)[p].tolist()}")
    return None


# ---------------------------------------------------------------------------------------------------------------------
# the cases

def _plant(C, H, cells_per_cascade, value=0.5):
    grid = np.zeros((C, H ** 3), np.float32)
    for cas, cells in enumerate(cells_per_cascade):
        grid[cas, np.asarray(cells, np.int64)] = value
    return grid


def _random_cells(rng, H3, k, must=()):
    """k distinct cells, `must` among them."""
    must = np.asarray(must, np.int64)
    rest = rng.choice(H3, size=k + len(must), replace=False)
    rest = rest[~np.isin(rest, must)][:k - len(must)]
    out = np.concatenate([must, rest])
    assert len(np.unique(out)) == k
    return out


class Case:
    """One call of enerf_density_grid_cells with a grid: its arguments, and what must hold for it to reach its branch."""

    def __init__(self, name, C, H, bound, n, seed, grid, check=None):
        self.name, self.C, self.H, self.bound, self.n, self.seed = name, C, H, float(bound), n, seed
        self._grid, self._check = grid, check
        self.P = C * 2 * n

    def grid(self):
        return self._grid()

    def statement(self, grid=None):
        """-> dict(keys sorted, idx, xyz, occ)"""
        grid = self.grid() if grid is None else grid
        occ = occupied(grid)
        keys = np.sort(select_keys(grid, self.C, self.H, self.n, self.seed, occ=occ))
        idx, xyz = cells_from_sorted_keys(keys, self.H, self.bound, self.seed)
        return dict(keys=keys, idx=idx, xyz=xyz, occ=occ, grid=grid)

    def assert_precondition(self, st):
        key_bits, low, nb = sort_geometry(self.C, self.H)
        assert low <= SORT_MAX_LOW and nb <= SORT_MAX_BUCKETS
        assert st["keys"].shape == (self.P,) and int(st["keys"].max()) < self.C << (3 * log2_exact(self.H))
        if self._check:
            self._check(self, st, key_bits, low, nb)

    def __repr__(self):
        return self.name


def existing_shape_grid():
    """The shape tests/test_gpu_density_update.py draws statistically: cascade 0 with 40 occupied cells, cascade 1 with
    5000 (the last cell of a 4096-cell block among them), cascade 2 with none; 1000 cells of cascade 0 at -1."""
    H3 = 64 ** 3
    rng = np.random.default_rng(3)
    grid = np.zeros((3, H3), np.float32)
    occ0, occ1 = _random_cells(rng, H3, 40), _random_cells(rng, H3, 5000, must=[5 * OCC_BLOCK - 1])
    grid[1, occ1] = rng.random(5000).astype(np.float32) + np.float32(0.1)
    grid[0, rng.choice(H3, 1000)] = -1.0
    grid[0, occ0] = 0.5
    return grid


def _check_existing(case, st, key_bits, low, nb):
    assert [len(o) for o in st["occ"]] == [40, 5000, 0]
    assert int((st["grid"][0] == -1).sum()) >= 900
    # cascade 2 draws all 2n uniformly: its keys are the uniform words of its points, occupied half included
    n, H3 = case.n, case.H ** 3
    i = np.arange(2 * 2 * n, 3 * 2 * n, dtype=np.uint64)
    want = np.sort((rand4(case.seed ^ SELECT_XOR, i)[:, 0] & np.uint32(H3 - 1)) | np.uint32(2 << 18))
    assert np.array_equal(st["keys"][2 * 2 * n:], want)


def _check_nb1(chunk_relation):
    def check(case, st, key_bits, low, nb):
        assert nb == 1 and low == 12 and key_bits == 12
        assert chunk_relation(case.P, SORT_CHUNK)
        assert all(len(o) > 0 for o in st["occ"])
    return check


def _check_small_p(case, st, key_bits, low, nb):
    assert case.P < 2 * SORT_MAX_BUCKETS and nb == 24


def _check_all_buckets(case, st, key_bits, low, nb):
    H3 = case.H ** 3
    assert nb == 4096 and low == 12 and key_bits == 24
    assert (st["grid"][0, :4096] > 0).any() and (st["grid"][case.C - 1, H3 - 4096:] > 0).any()
    b = st["keys"] >> np.uint32(low)
    assert b[0] == 0 and b[-1] == 4095                       # ... and both buckets receive keys


def _check_low13(case, st, key_bits, low, nb):
    assert key_bits == 25 and low == 13 and nb == 4096 and case.H ** 3 // OCC_BLOCK == 4096
    for cas in range(case.C):
        blocks = np.unique(st["occ"][cas] // OCC_BLOCK)
        assert {1023, 1024, 4095} <= set(blocks.tolist())


def _check_low14(case, st, key_bits, low, nb):
    assert key_bits == 26 and low == 14 and nb == 4096


def _heavy_values(st, low):
    """per bucket, the number of values that occur more than HEAVY_ABOVE times."""
    v, c = value_counts(st["keys"])
    return np.bincount((v[c > HEAVY_ABOVE] >> np.uint32(low)).astype(np.int64)), c


def _check_heavy(lo, hi):
    def check(case, st, key_bits, low, nb):
        assert nb == 1
        heavy, _ = _heavy_values(st, low)
        assert lo <= int(heavy[0]) <= hi, heavy
    return check


def _check_boundary(case, st, key_bits, low, nb):
    _, c = value_counts(st["keys"])
    assert (c == HEAVY_ABOVE).any() and (c == HEAVY_ABOVE + 1).any()


OCC_EDGE_CELLS = (0, 15, 16, 4095, 4096, 32 ** 3 - 1)
OCC_EDGE_VALUES = (-1.0, 0.0, -0.0, float("nan"), 1e-45, float("inf"))       # the last two are occupied


def _occupied_edges_grid(rot):
    def make():
        grid = np.zeros((2, 32 ** 3), np.float32)
        for k, cell in enumerate(OCC_EDGE_CELLS):
            grid[0, cell] = np.float32(OCC_EDGE_VALUES[(k + rot) % 6])
        grid[1] = np.float32(0.25)
        return grid
    return make


def _check_occupied_edges(rot):
    def check(case, st, key_bits, low, nb):
        assert len(st["occ"][1]) == case.H ** 3
        want = sorted(cell for k, cell in enumerate(OCC_EDGE_CELLS) if (k + rot) % 6 >= 4)
        assert st["occ"][0].tolist() == want and len(want) == 2
        g = st["grid"][0, list(want)]
        assert (g > 0).all() and (g.min() < 1e-38) and np.isinf(g.max())      # the denormal stayed one in float32
        # every draw of the occupied half of cascade 0 lands on those two cells
        v, c = value_counts(st["keys"][:2 * case.n])
        assert all(int(c[v == w][0]) > case.n // 4 for w in want)
    return check


def _rng_cells(seed, H, per_cascade, must=()):
    def make():
        rng = np.random.default_rng(seed)
        return _plant(len(per_cascade), H, [_random_cells(rng, H ** 3, k, must=must) for k in per_cascade])
    return make


def _build_cases():
    cs = []
    ge, eq, lt = (lambda P, c: P > c), (lambda P, c: P == c), (lambda P, c: P < c)
    for n, rel in ((1, lt), (4096, eq), (4097, ge)):
        cs.append(Case(f"one_bucket_n{n}", 1, 16, 1, n, 41 + n, _rng_cells(1, 16, [7]), _check_nb1(rel)))
    cs.append(Case("p_below_counters", 3, 32, 3, 100, 7, _rng_cells(2, 32, [9, 300, 0]), _check_small_p))
    for seed in (99, 0, 2 ** 63 + 5, 2 ** 64 - 1):
        cs.append(Case(f"existing_shape_seed{seed}", 3, 64, 3, 64 ** 3 // 4, seed, existing_shape_grid, _check_existing))
    for C in (2, 3):
        cs.append(Case(f"workload_c{C}", C, 128, 2 ** (C - 1), 128 ** 3 // 4, 0x1234567890ABCDEF + C,
                       _rng_cells(4, 128, [60000, 7000, 300][:C])))
    cs.append(Case("all_buckets", 8, 128, 100, 50000, 11,
                   _rng_cells(5, 128, [3000] * 8, must=[3, 4095, 128 ** 3 - 4096, 128 ** 3 - 1]), _check_all_buckets))
    edge_blocks = [1023 * 4096 + 4095, 1024 * 4096, 4095 * 4096 + 17, 256 ** 3 - 1]
    cs.append(Case("low13_four_scan_trips", 2, 256, 2, 50000, 12, _rng_cells(6, 256, [4000, 900], must=edge_blocks),
                   _check_low13))
    cs.append(Case("low14", 4, 256, 8, 50000, 13, _rng_cells(7, 256, [4000, 900, 50, 20000], must=edge_blocks),
                   _check_low14))
    cs.append(Case("one_heavy_value", 1, 16, 1, 5000, 14, _rng_cells(8, 16, [1]), _check_heavy(1, 1)))
    for k, lo, hi in ((64, 64, 64), (65, 65, 65), (100, 100, 4096)):
        cs.append(Case(f"heavy_table_{k}", 1, 16, 1, 20000, 15, _rng_cells(9, 16, [k]), _check_heavy(lo, hi)))
    cs.append(Case("count_64_and_65", 1, 16, 1, 20000, 16, _rng_cells(10, 16, [312]), _check_boundary))
    for rot in range(6):
        cs.append(Case(f"occupied_edges_rot{rot}", 2, 32, 2, 3000, 17 + rot, _occupied_edges_grid(rot),
                       _check_occupied_edges(rot)))
    return cs


CASES = _build_cases()
CASE = {c.name: c for c in CASES}
FULL_SWEEPS = ((3, 32), (1, 64), (2, 128))               # (bound, H); C = 1 + ceil(log2 bound)
