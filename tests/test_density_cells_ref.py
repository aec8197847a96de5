"""Host tests of tests/density_cells_ref.py, the exact statement of the density update's cell selection: published
known answers of its generator, seeded defects that its comparator must reject (and that the statistical assertions of
tests/test_gpu_density_update.py mostly accept), and the preconditions of every case that
tests/test_gpu_density_cells_exact.py runs on the device.  No GPU."""
import numpy as np
import pytest

import density_cells_ref as R
from oracle import density_update as OD
from oracle import oracle as O

M64 = 2 ** 64 - 1


# ---- the generator
def test_mix64_reproduces_the_first_two_outputs_of_splitmix64_seed_0():
    g = 0x9E3779B97F4A7C15
    assert int(R.mix64(g)[0]) == 0xE220A8397B1DCDAF
    assert int(R.mix64((2 * g) & M64)[0]) == 0x6E789E6AA1B965F4
    assert [int(v) for v in R.mix64(np.array([g, (2 * g) & M64], np.uint64))] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]


def _mix64_int(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


@pytest.mark.parametrize("seed", [0, 1, 99, 2 ** 63 + 5, M64])
def test_rand4_in_uint64_equals_python_integers(seed):
    counters = [0, 1, 2, 8191, 2 ** 31 - 1, 2 ** 32 - 1]
    got = R.rand4(seed, np.array(counters, np.uint64))
    g = 0x9E3779B97F4A7C15
    for row, c in zip(got, counters):
        a = _mix64_int((seed + g * (2 * c + 1)) & M64)
        b = _mix64_int((a + g * (2 * c + 2) + seed) & M64)
        assert [int(w) for w in row] == [a & 0xFFFFFFFF, a >> 32, b & 0xFFFFFFFF, b >> 32]


def test_morton_is_the_oracles():
    rng = np.random.default_rng(0)
    xyz = rng.integers(0, 512, size=(4000, 3)).astype(np.int32)
    m = R.morton3(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    assert np.array_equal(m.astype(np.int32), O.morton3D(xyz))
    assert np.array_equal(np.stack(R.morton3_invert(m), -1).astype(np.int32), xyz)


def test_positions_are_the_formula_in_float32_and_stay_in_their_cell():
    C, H, bound = 3, 32, 3
    idx, xyz = R.cells_full(C, H, bound, 5)
    assert xyz.dtype == np.float32 and idx.dtype == np.int32
    for cas in range(C):
        sl = slice(cas * H ** 3, (cas + 1) * H ** 3)
        assert np.array_equal(np.sort(idx[sl]), np.arange(H ** 3))
        span, half = OD.cascade_geometry(cas, bound, H)
        off = xyz[sl].astype(np.float64) - OD.cell_centres(idx[sl], cas, bound, H).astype(np.float64)
        assert np.abs(off).max() <= half + 4 * 2.0 ** -24 * bound       # fp32 roundings of values below `bound`
        assert np.abs(off).max() > 0.98 * half
    # the first point by hand: cell (0, 0, 0) of cascade 0, words of counter 0
    w = R.rand4(5, [0])[0]
    f = np.float32
    span, half = f(1.0 - 1.0 / 32), f(1.0 / 32)
    for a in range(3):
        u = f(int(w[a]) >> 8) * f(2.0 ** -24)
        assert xyz[0, a] == f(f(f(f(f(2) * f(0)) * (f(1) / f(31))) - f(1)) * span) + f(f(f(u * f(2)) - f(1)) * half)


# ---- the comparator against seeded defects
@pytest.fixture(scope="module")
def existing():
    case = R.CASE["existing_shape_seed99"]
    st = case.statement()
    st["unsorted"] = R.select_keys(st["grid"], case.C, case.H, case.n, case.seed)
    return case, st


def _from_keys(case, keys, **kw):
    return R.cells_from_sorted_keys(keys, case.H, case.bound, case.seed, **kw)


def _segment(case, cas):
    return slice(cas * 2 * case.n, (cas + 1) * 2 * case.n)


def _defect(case, st, which):
    """-> (indices, positions) of the statement with seeded defect `which` (1-7)."""
    keys = st["keys"].copy()
    if which == 1:                       # one sorted key dropped, its successor written twice
        p = case.n + int(np.flatnonzero(np.diff(keys[case.n:]) > 0)[0])
        assert keys[p] >> 18 == keys[p + 1] >> 18
        keys[p] = keys[p + 1]
        return _from_keys(case, keys)
    if which == 2:                       # the occupied list misses the last cell of a 4096-cell block
        occ = list(st["occ"])
        last = np.flatnonzero(occ[1] % R.OCC_BLOCK == R.OCC_BLOCK - 1)
        assert last.size
        occ[1] = np.delete(occ[1], last[0])
        return _from_keys(case, np.sort(R.select_keys(st["grid"], case.C, case.H, case.n, case.seed, occ=occ)))
    if which == 3:                       # the occupied draw over cnt - 1
        return _from_keys(case, np.sort(R.select_keys(st["grid"], case.C, case.H, case.n, case.seed, occ=st["occ"],
                                                      draw_over=lambda cnt: cnt - 1)))
    if which == 4:                       # one heavy value written c - 1 times, the rest of its cascade shifted
        seg = keys[_segment(case, 0)]
        v, c = R.value_counts(seg)
        heavy = v[c > R.HEAVY_ABOVE]
        assert heavy.size == 40
        p = int(np.searchsorted(seg, heavy[7]))
        keys[_segment(case, 0)] = np.concatenate([seg[:p], seg[p + 1:], seg[-1:]])
        return _from_keys(case, keys)
    if which == 5:                       # jitter words 0 and 1 swapped
        return _from_keys(case, keys, word_of_axis=(1, 0, 2))
    if which == 6:                       # the position's counter taken before the sort
        return _from_keys(case, keys, counters=np.argsort(st["unsorted"], kind="stable").astype(np.uint64))
    if which == 7:                       # one cascade's keys left unsorted across a bucket boundary
        _, low, _ = R.sort_geometry(case.C, case.H)
        seg = keys[_segment(case, 1)]
        q = int(np.flatnonzero(np.diff(seg >> np.uint32(low)) > 0)[3]) + 1
        seg[q - 1], seg[q] = seg[q], seg[q - 1]
        keys[_segment(case, 1)] = seg
        return _from_keys(case, keys)
    raise ValueError(which)


def test_comparator_accepts_the_statement_recomputed(existing):
    case, st = existing
    idx, xyz = R.cells_partial(st["grid"], case.C, case.H, case.bound, case.n, case.seed)
    assert R.compare(idx, xyz, st["idx"], st["xyz"]) is None
    assert R.compare(idx[:-1], xyz[:-1], st["idx"], st["xyz"]) is not None
    flipped = xyz.copy()
    flipped.view(np.uint32)[12345, 2] ^= 1                                   # one last bit of one coordinate
    assert "positions differ" in R.compare(idx, flipped, st["idx"], st["xyz"])
    negz = np.zeros((1, 3), np.float32)
    assert R.compare(idx[:1], -negz, idx[:1], negz) is not None              # bits, not values: -0.0 is not 0.0


@pytest.mark.parametrize("which", [1, 2, 3, 4, 5, 6, 7])
def test_comparator_rejects_every_seeded_defect(existing, which):
    case, st = existing
    idx, xyz = _defect(case, st, which)
    verdict = R.compare(idx, xyz, st["idx"], st["xyz"])
    assert verdict is not None, which
    if which in (5, 6):
        assert np.array_equal(idx, st["idx"]) and "positions differ" in verdict      # the cells are right, the jitter is not


def _statistical_assertions(idx, xyz, grid, C, H, bound, N):
    """The assertions of test_partial_update_draws_uniform_and_occupied_cells_sorted (tests/test_gpu_density_update.py) and
    of its _check_positions, statement for statement, on arrays instead of a device call."""
    H3 = H ** 3
    idx, xyz = idx.reshape(C, -1), xyz.reshape(C, -1, 3)
    occ = [np.flatnonzero(g > 0) for g in grid]
    assert idx.shape == (C, 2 * N)
    for cas in range(C):
        assert np.all(np.diff(idx[cas]) >= 0) and idx[cas].min() >= 0 and idx[cas].max() < H3
        in_occ = np.isin(idx[cas], occ[cas]).sum()
        expect = N + N * len(occ[cas]) / H3 if len(occ[cas]) else 0
        assert abs(in_occ - expect) <= 5 * np.sqrt(N * max(len(occ[cas]), 1) / H3) + 1, (cas, in_occ, expect)
        if len(occ[cas]):
            hits = np.bincount(np.searchsorted(np.sort(occ[cas]), idx[cas][np.isin(idx[cas], occ[cas])]),
                               minlength=len(occ[cas]))
            lam = N / len(occ[cas]) + 2 * N / H3
            assert abs(hits.mean() - lam) < 0.02 * lam
            assert 0.8 < hits.var() / lam < 1.25 if len(occ[cas]) > 1000 else hits.min() > 0.8 * lam
        frac = len(np.unique(idx[cas])) / H3
        want = 1 - np.exp(-0.25 if len(occ[cas]) else -0.5)
        assert abs(frac - want) < 0.03
    for cas in range(C):
        span, half = OD.cascade_geometry(cas, bound, H)
        off = xyz[cas] - OD.cell_centres(idx[cas], cas, bound, H)
        assert np.abs(off).max() <= half * (1 + 1e-5) + 1e-6
        assert np.abs(off).max() > 0.98 * half
        assert abs(off.mean()) < 0.02 * half
        assert np.abs(np.corrcoef(off[:, 0], off[:, 1])[0, 1]) < 0.02


STATISTICS_ACCEPT = {1, 2, 4, 5}


def test_which_seeded_defects_the_statistical_assertions_accept(existing):
    """The argument for the exact comparison, as a checked fact.  On the shape the statistical test runs (C 3, H 64;
    40 / 5000 / 0 occupied cells), its assertions ACCEPT
        1  a sorted key dropped and its successor written twice,
        2  an occupied list without the last cell of a 4096-cell block,
        4  a heavy value written c - 1 times with the rest shifted,
        5  jitter words 0 and 1 swapped,
    and reject only
        3  the occupied draw over cnt - 1: with 40 occupied cells the last of them is never drawn, and `hits.min()` sees it
           (with the 5000 cells of cascade 1 alone it would pass).
    The exact comparator rejects all seven (test_comparator_rejects_every_seeded_defect)."""
    case, st = existing
    args = (st["grid"], case.C, case.H, case.bound, case.n)
    _statistical_assertions(st["idx"], st["xyz"], *args)                      # the statement itself passes them
    accepted = set()
    for which in (1, 2, 3, 4, 5):
        idx, xyz = _defect(case, st, which)
        try:
            _statistical_assertions(idx, xyz, *args)
            accepted.add(which)
        except AssertionError:
            pass
    assert accepted == STATISTICS_ACCEPT


# ---- the cases of the device test reach their branches
@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_case_precondition(case):
    case.assert_precondition(case.statement())


def test_cases_cover_the_table():
    geo = {c.name: R.sort_geometry(c.C, c.H) for c in R.CASES}
    assert {g[1] for g in geo.values()} == {12, 13, 14}                       # every `low`
    assert {1, 24, 4096} <= {g[2] for g in geo.values()}                      # one bucket ... all of them
    assert sorted(c.P for c in R.CASES if c.name.startswith("one_bucket")) == [2, R.SORT_CHUNK, R.SORT_CHUNK + 2]
    assert max(c.P for c in R.CASES) == 3 * 2 * (128 ** 3 // 4)                # the workload's 3.1 M keys
    # what the library refuses: 27 key bits
    assert R.sort_geometry(5, 256)[1] == 15 and R.sort_geometry(3, 256)[:2] == (26, 14)
