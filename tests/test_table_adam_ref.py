"""Host tests of tests/table_adam_ref.py, the fp64 reference tests/test_gpu_table_adam_fp64.py holds the table optimizer
pass to: the reference against the CPU oracle and torch.optim.Adam, the comparator against seeded defects, and the
conditions the committed inputs must meet for the GPU comparison to mean what it says."""
import numpy as np
import pytest
import torch

import table_adam_ref as R
from oracle import oracle as O

U = 2.0 ** -24


@pytest.mark.parametrize("gridtype", [0, 1])
@pytest.mark.parametrize("geom", ["A", "B", "C1", "C4", "C8", "D2"])
def test_grid_grad_ref_matches_the_cpu_oracle(geom, gridtype):
    """grid_grad_ref against oracle.grid_encode_backward at every element:
        |G - oracle| <= (2 D + N) * 2^-24 * A + 2^-24 * |G|,   and the oracle is zero exactly where N == 0.
    The oracle forms every term in fp32 -- D subtractions 1 - frac, D - 1 products of the factors and the product with
    g: 2 D roundings -- and adds the N terms of an element sequentially in fp32 (N roundings at most).  A bound of
    N * 2^-24 * A + 2^-24 * |G| counts the sums alone: elements with one or two contributions then miss it by the
    terms' own roundings (geometry A, hashed: 582 elements, up to 1.30 times that bound)."""
    offsets, L, C, D = R.geometry(geom)
    rng = np.random.default_rng([7, gridtype, sorted(R.GEOMS).index(geom)])
    x = R.make_samples(rng, R.FULL, D)
    worst = 0.0
    for family in R.FAMILIES:
        g = R.make_grads(rng, family, R.FULL, L, C, 0)
        G, A, N = R.grid_grad_ref(x, g, offsets, D, C, R.S_LOG2, R.H_BASE, gridtype)
        ge, _ = O.grid_encode_backward(g, x, np.zeros((int(offsets[-1]), C), np.float32), offsets, R.S_LOG2, R.H_BASE,
                                       gridtype=gridtype)
        bound = (2 * D + N[:, None]) * U * A + U * np.abs(G)
        err = np.abs(ge.astype(np.float64) - G)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (geom, gridtype, family, int((err > bound).sum()), worst)
        assert not ge[N == 0].any()
        assert int(N.sum()) == (R.FULL - 1) * L * (1 << D)          # one sample lies outside [0, 1]^D
    print(f"{geom} gridtype {gridtype}: worst error / bound {worst:.3f}")


def test_adam_ref_matches_torch_adam_in_float64():
    """Four steps with a moving learning rate against torch.optim.Adam on float64 CPU tensors, to 1e-13 relative."""
    rng = np.random.default_rng(3)
    p0 = R.make_params(rng, (257, 2)).astype(np.float64)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=1e-2, betas=(R.B1, R.B2), eps=R.EPS)
    p, m, v = p0, np.zeros_like(p0), np.zeros_like(p0)
    for step in range(4):
        g = rng.normal(size=p0.shape) * (0.1 + step)
        g[::7] = 0.0
        lr = R.lr_of(step)
        for group in opt.param_groups:
            group["lr"] = lr
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = R.adam_ref(p, m, v, g, lr, R.B1, R.B2, R.EPS, step + 1)
        st = opt.state[tp]
        for mine, theirs in ((p, tp.data), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            theirs = theirs.numpy()
            assert np.abs(mine - theirs).max() <= 1e-13 * np.abs(theirs).max(), step


# ---- the comparator must be able to fail ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    """One optimizer step of geometry A from the reference alone: state before (moments live: step 2), the reference
    gradient, and a perfect kernel's answer (adam_ref rounded to fp32)."""
    rng = np.random.default_rng(11)
    r = R.step_reference("A_min1", "one", 0)
    shape = r["G"].shape
    p = R.make_params(rng, shape)
    m = (0.1 * rng.normal(size=shape)).astype(np.float32)
    v = (0.01 * rng.uniform(0.5, 1.5, shape)).astype(np.float32)
    return dict(r=r, p=p, m=m, v=v, lr=R.lr_of(1), t=2)


def _kernel(s, G, t=None, lr=None):
    """What a correctly rounding kernel would store for gradient G."""
    out = R.adam_ref(s["p"], s["m"], s["v"], G, s["lr"] if lr is None else lr, R.B1, R.B2, R.EPS, s["t"] if t is None else t)
    return tuple(a.astype(np.float32) for a in out)


def _step(s, got, G=None, dG=None, t=None):
    r = s["r"]
    return R.compare_step(got, s["p"], s["m"], s["v"], r["G"] if G is None else G, r["dG"] if dG is None else dG, s["lr"],
                          R.B1, R.B2, R.EPS, s["t"] if t is None else t, "one")


def test_comparator_accepts_a_correctly_rounded_result(scene):
    r = scene["r"]
    assert _step(scene, _kernel(scene, r["G"])) == []
    # ... and one that uses the whole gradient bound
    assert _step(scene, _kernel(scene, r["G"] + 0.99 * r["dG"])) == []
    lo, hi = R.RANGES["inside"]
    got = [a.copy() for a in (scene["p"], scene["m"], scene["v"])]
    upd = _kernel(scene, R.REC_SCALE * r["G"])
    for a, b in zip(got, upd):
        a.reshape(-1)[lo:hi] = b.reshape(-1)[lo:hi]
    assert R.compare_range_step(got, scene["p"], scene["m"], scene["v"], R.REC_SCALE * r["G"], R.REC_SCALE * r["dG"], lo, hi,
                                scene["lr"], R.B1, R.B2, R.EPS, scene["t"], "one") == []


def test_comparator_rejects_a_dropped_record(scene):
    """(a) one record missing from the list of the most-populated tile (the first sample's heaviest corner there)."""
    r = scene["r"]
    offsets, C, D = r["offsets"], r["C"], r["D"]
    (x, g), = R.step_inputs("A_min1", "one", 0)
    per_tile = [(int(n.sum(axis=1).max()), l, int(n.sum(axis=1).argmax())) for l, n in enumerate(r["records_hi"])]
    _, level, tile = max(per_tile)
    c = R.corners(x, offsets, D, R.S_LOG2, R.H_BASE, 0)[level]
    Rr = R.TILE_ELEMS // C
    hit = np.argwhere(c["valid"][:, None] & (c["rows"] // Rr == tile))
    b = int(hit[0, 0])
    idx = int(np.argmax(np.where(c["rows"][b] // Rr == tile, c["w"][b], -1.0)))
    G = r["G"].copy()
    G[int(offsets[level]) + c["rows"][b, idx]] -= c["w"][b, idx] * g[level, b].astype(np.float64)
    assert _step(scene, _kernel(scene, G)) != []


def test_comparator_rejects_a_missing_rec_scale_and_a_write_outside_the_range(scene):
    """(b) rec_scale omitted; (f) the element just outside the owner range updated."""
    r = scene["r"]
    lo, hi = R.RANGES["across"]
    args = (scene["p"], scene["m"], scene["v"], R.REC_SCALE * r["G"], R.REC_SCALE * r["dG"], lo, hi, scene["lr"], R.B1, R.B2,
            R.EPS, scene["t"], "one")

    def result(G, a, b):
        got = [t.copy() for t in (scene["p"], scene["m"], scene["v"])]
        for dst, src in zip(got, _kernel(scene, G)):
            dst.reshape(-1)[a:b] = src.reshape(-1)[a:b]
        return got
    assert R.compare_range_step(result(R.REC_SCALE * r["G"], lo, hi), *args) == []
    assert R.compare_range_step(result(r["G"], lo, hi), *args) != []                          # (b)
    assert R.compare_range_step(result(R.REC_SCALE * r["G"], lo, hi + 1), *args) != []        # (f) above
    assert R.compare_range_step(result(R.REC_SCALE * r["G"], lo - 1, hi), *args) != []        # (f) below


def test_comparator_rejects_wrong_bias_corrections_and_a_missing_unscale(scene):
    """(c) bias corrections from `step` (3) where two steps were skipped (t = 1); (d) unscale omitted (scale 1024)."""
    r = scene["r"]
    assert _step(scene, _kernel(scene, r["G"], t=1), t=1) == []
    assert _step(scene, _kernel(scene, r["G"], t=3), t=1) != []                               # (c)
    assert _step(scene, _kernel(scene, 1024.0 * r["G"])) != []                                # (d)


def test_comparator_rejects_a_shifted_small_tensor():
    """(e) one small tensor's elements shifted by one."""
    rng = np.random.default_rng(5)
    n = R.SMALL_SIZES[3]
    p = R.make_params(rng, n)
    m = (0.1 * rng.normal(size=n)).astype(np.float32)
    v = (0.01 * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    g = rng.normal(size=n).astype(np.float32)
    lr, t = float(np.float32(3e-3)), 5
    good = tuple(a.astype(np.float32) for a in R.adam_ref(p, m, v, g, lr, R.B1, R.B2, R.EPS, t))
    bad = tuple(a.astype(np.float32) for a in R.adam_ref(p, m, v, np.roll(g, 1), lr, R.B1, R.B2, R.EPS, t))
    assert R.compare_small(good, p, m, v, g, lr, R.B1, R.B2, R.EPS, t) == []
    assert R.compare_small(bad, p, m, v, g, lr, R.B1, R.B2, R.EPS, t) != []


# ---- conditions on the committed inputs -----------------------------------------------------------------------------
def _loose_share(G, dG, N, offsets, C, sel=None):
    """Share of touched elements with dG > 1e-3 |G|: (worst level, whole table); sel: restrict to these flat elements."""
    touched = np.repeat((N > 0)[:, None], C, axis=1)
    if sel is not None:
        keep = np.zeros(touched.size, bool)
        keep[sel[0]:sel[1]] = True
        touched &= keep.reshape(touched.shape)
    loose = (dG > 1e-3 * np.abs(G)) & touched
    per = [loose[offsets[l]:offsets[l + 1]].sum() / max(1, touched[offsets[l]:offsets[l + 1]].sum())
           for l in range(len(offsets) - 1)]
    return max(per), loose.sum() / max(1, touched.sum())


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_input_conditions(case):
    """What the GPU comparison relies on, from the reference alone, at every step of the case and for both families:
      * signed family: at most 2 % of a level's touched elements and 0.5 % of the table's are compared loosely
        (dG > 1e-3 |G|);
      * the spill case: for some level the records that MUST land in one tile (2^D per sample whose cell differs from the
        previous sample's) exceed the list's capacity ((2 * 2^D * reserve_B) / bins) & ~1, and the slab leaves tiles of
        levels 1-3 without records (the tile loop's empty branch);
      * every other case: at least 30 % of each binned level's tiles receive records.
    (Uniform samples over the unit cube reach every tile of a level, so "some tile receives none" can hold only where
    the samples are confined: the slab of the spill case.)"""
    c = R.CASES[case]
    for family in R.FAMILIES:
        for step, calls in enumerate(c["steps"]):
            if not calls:
                continue
            r = R.step_reference(case, family, step)
            if family == "signed":
                per, whole = _loose_share(r["G"], r["dG"], r["N"], r["offsets"], r["C"])
                print(f"{case} step {step}: loosely compared {100 * per:.2f} % (worst level) {100 * whole:.3f} % (table)")
                assert per <= 0.02 and whole <= 0.005, (case, step, per, whole)
            got = [(n.sum(axis=1) > 0) for l, n in enumerate(r["records_hi"]) if r["plans"][l][2]]
            if "slab" in c:
                over = [l for l in range(r["L"]) if r["caps"][l] and r["records_lo"][l].max() > r["caps"][l]]
                assert over, (case, family, step, "no list is certain to overflow")
                assert 2 in over and 3 in over and 0 not in over
                assert all((~got[l]).any() for l in (1, 2, 3))
            else:
                assert all(t.mean() >= 0.3 for t in got), (case, family, step, [float(t.mean()) for t in got])


@pytest.mark.parametrize("name", sorted(R.RANGES))
def test_input_conditions_owner_range(name):
    """The same cap on the loosely compared share for the owner-range cases, over the elements of the range."""
    for step in range(3):
        r = R.range_reference(name, "signed", step)
        per, whole = _loose_share(r["G_adam"], r["dG_adam"], r["N"], r["offsets"], r["C"], sel=(r["lo"], r["hi"]))
        print(f"range {name} step {step}: loosely compared {100 * per:.2f} % (worst level) {100 * whole:.3f} % (range)")
        assert per <= 0.02 and whole <= 0.005, (name, step, per, whole)
        if name != "dense":
            assert r["whole"].any() == (name != "inside")          # "inside" cuts its one tile; the others hold whole tiles
