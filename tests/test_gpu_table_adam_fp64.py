"""The hash table's optimizer pass (csrc/gridencoder.hip: k_grid_tile_adam and the deferred grid backward that feeds it)
against the fp64 reference of tests/table_adam_ref.py, called through enerf_amd._lib and enerf_amd.backends._gridencoder.

Every case runs three optimizer steps from fresh samples; after each step m, v and p are compared AT EVERY ELEMENT with
the a-priori bound of the reference module (rounding counts of the kernels' statements, carried through Adam), elements
nobody touched included (their moments decay), and the dense gradient buffer must be all zero.  Each step's reference
starts from the kernel's own p / m / v of the step before, so no error is carried from step to step.  Two gradient
families: one-signed (no cancellation: p, m, v held everywhere) and signed (m, v held everywhere; p wherever the
gradient's bound is below 1e-3 of the gradient, elsewhere to 2.5 lr -- tests/test_table_adam_ref.py caps that share).
Forms: plain at C = 1, 2, 4, 8 and D = 2, 3 (replica lists, short last tiles, levels too large to bin, several
backward calls joining one flush, a step with nothing pending), forced list overflow, small tensors riding along, loss
scaling (unscale, step - skipped, skipped steps bit-identical), the owner range, and the calls that must be refused."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import table_adam_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _lib():
    from enerf_amd import _lib as L
    return L


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@contextlib.contextmanager
def binning(min_batch, min_tiles):
    """Force the binned backward; whatever happens inside, leave the library as the rest of the suite expects it."""
    L = _lib()
    lib = L.lib()
    L.check(lib.enerf_debug_grid_bwd_binned(min_batch, min_tiles), "debug_grid_bwd_binned")
    try:
        yield lib
    finally:
        lib.enerf_debug_grid_bwd_binned(16384, 8)
        lib.enerf_grid_owner_range(0, 0, 1.0)
        lib.enerf_amp_cancel()
        lib.enerf_grid_records_discard(L.stream_handle())
        torch.cuda.synchronize()


class Table:
    def __init__(self, geom, rng, gridtype=0):
        self.offsets, self.L, self.C, self.D = R.geometry(geom)
        self.gridtype = gridtype
        rows = int(self.offsets[-1])
        self.p = _dev(R.make_params(rng, (rows, self.C)))
        self.m = torch.zeros_like(self.p)
        self.v = torch.zeros_like(self.p)
        self.g = torch.zeros_like(self.p)
        self.offsets_t = _dev(self.offsets.astype(np.int32))
        self.dummy = torch.empty(1, device=DEV)

    def state(self):
        return tuple(t.cpu().numpy() for t in (self.p, self.m, self.v))

    def backward(self, x, g, layout, reserve, scale=1.0):
        """x [B, D], g [L, B, C] (the reference's layout); layout 1 hands the kernel [B, L * C]."""
        from enerf_amd.backends import _gridencoder as ge
        B = x.shape[0]
        g = g * np.float32(scale)
        gt = _dev(g if layout == 0 else g.transpose(1, 0, 2).reshape(B, self.L * self.C))
        ge.grid_encode_backward(gt, _dev(x), self.p, self.offsets_t, self.g, B, self.D, self.C, self.L, R.S_LOG2, R.H_BASE,
                                False, self.dummy, self.dummy, self.gridtype, layout=layout, defer=True, reserve=reserve)

    def adam(self, lr, step, small=None, n_small=None):
        """-> the entry point's return code (0: launched)."""
        L = _lib()
        if small:
            n = len(small.p) if n_small is None else n_small
            k = len(small.p)
            vp, u32, fl = ctypes.c_void_p * k, ctypes.c_uint32 * k, ctypes.c_float * k
            args = (n, vp(*[t.data_ptr() for t in small.p]), vp(*[t.data_ptr() for t in small.g]),
                    vp(*[t.data_ptr() for t in small.m]), vp(*[t.data_ptr() for t in small.v]),
                    u32(*[t.numel() for t in small.p]), fl(*small.lr), u32(*small.step))
        else:
            args = (0, None, None, None, None, None, None, None)
        return L.lib().enerf_grid_adam_from_records_ex(
            self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.offsets_t.data_ptr(), self.L,
            self.C, lr, R.B1, R.B2, R.EPS, step, *args, L.stream_handle())


class Small:
    """The small tensors that ride in the launch: own learning rate and own step count each."""

    def __init__(self, rng, sizes):
        self.p = [_dev(R.make_params(rng, n)) for n in sizes]
        self.m = [_dev((0.1 * rng.normal(size=n)).astype(np.float32)) for n in sizes]
        self.v = [_dev((0.01 * rng.uniform(0.5, 1.5, n)).astype(np.float32)) for n in sizes]
        self.g = [torch.zeros_like(t) for t in self.p]
        self.lr = [float(np.float32(1e-3 * (k + 1))) for k in range(len(sizes))]
        self.step = [3 + k for k in range(len(sizes))]

    def state(self):
        return [tuple(t[k].cpu().numpy() for t in (self.p, self.m, self.v)) for k in range(len(self.p))]

    def new_grads(self, rng, scale=1.0):
        gs = [rng.normal(size=t.numel()).astype(np.float32) for t in self.p]
        for t, g in zip(self.g, gs):
            t.copy_(_dev(g * np.float32(scale)))
        return gs

    def check(self, before, gs, t_of, what, scale=1.0):
        fails = []
        for k, (b, g) in enumerate(zip(before, gs)):
            got = tuple(t[k].cpu().numpy() for t in (self.p, self.m, self.v))
            fails += R.compare_small(got, *b, g, self.lr[k], R.B1, R.B2, R.EPS, t_of(self.step[k]), f"{what} small[{k}] ")
            back = self.g[k].cpu().numpy()
            if not np.array_equal(back.view(np.uint32), (g * np.float32(scale)).view(np.uint32)):
                fails.append(f"{what} small[{k}]: its gradient came back modified")
        return fails


def run_steps(case, family, lib, tab, small=None, scale=1.0, t_of=lambda step: step, host_step0=1, steps=(0, 1, 2)):
    """The optimizer steps `steps` of a case on `tab`; every step compared with the reference.  scale: the gradients are
    fed multiplied by it (loss scaling armed by the caller); t_of: host step -> the step count Adam must use."""
    c = R.CASES[case]
    rng = np.random.default_rng([c["seed"], R.FAMILIES.index(family), 5])
    fails = []
    for step in steps:
        what = f"{case} {family} step {step}: "
        before = tab.state()
        calls = R.step_inputs(case, family, step)
        if calls:
            r = R.step_reference(case, family, step)
            G, dG = r["G"], r["dG"]
            for x, g in calls:
                tab.backward(x, g, c["layout"], sum(xx.shape[0] for xx, _ in calls), scale)
        else:                                           # nothing pending: the pass runs over a dense gradient
            dense = R.dense_step_gradient(case, family, step)
            tab.g.copy_(_dev(dense * np.float32(scale)))
            G, dG = dense.astype(np.float64), np.zeros(dense.shape)
        if small:
            sbefore, gs = small.state(), small.new_grads(rng, scale)
            small.step = [s + 1 for s in small.step]
        lr = R.lr_of(step)
        rc = tab.adam(lr, host_step0 + step, small)
        assert rc == 0, _lib().lib().enerf_last_error()
        fails += R.compare_step(tab.state(), *before, G, dG, lr, R.B1, R.B2, R.EPS, t_of(host_step0 + step), family, what)
        if small:
            fails += small.check(sbefore, gs, t_of, what, scale)
        if bool(tab.g.any()):
            fails.append(what + "the dense gradient buffer is not all zero")
    return fails


PLAIN = ["A_min1", "A_min8", "B", "C1", "C4", "C8", "D2", "D2_tiled"]


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case", PLAIN)
def test_plain(case, family):
    """Geometry A with and without replica lists (two backward calls joining one flush, a second call of 1000 samples, a
    step with nothing pending), geometry B (a level too large to bin; gradient layout 0), C = 1, 4, 8 (C = 8 with a
    level beyond 512 lists), D = 2 hashed and tiled."""
    c = R.CASES[case]
    with binning(0, c["min_tiles"]) as lib:
        tab = Table(c["geom"], np.random.default_rng(c["seed"]), c.get("gridtype", 0))
        fails = run_steps(case, family, lib, tab)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_spill(family):
    """Every sample in a slab one level-2 cell thick: lists of levels 2 and 3 are CERTAIN to overflow (asserted from the
    reference's own corner rows before anything is launched), so records go into the dense gradient by atomics and the
    `spilled` branch reads lists and dense gradient.  Tiles that may have overflowed get the spill-path bound."""
    c = R.CASES["spill"]
    for step in range(3):
        r = R.step_reference("spill", family, step)
        over = [l for l in range(r["L"]) if r["caps"][l] and r["records_lo"][l].max() > r["caps"][l]]
        assert over, "the spill is not certain"
    with binning(0, c["min_tiles"]) as lib:
        tab = Table(c["geom"], np.random.default_rng(c["seed"]))
        fails = run_steps("spill", family, lib, tab)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case", ["small8", "small5", "small1"])
def test_small_tensors(case, family):
    """n_small = 8, 5, 1 tensors of sizes {1, 7, 64, 2049, 4096, 33, 1024, 3}, each with its own lr and step count,
    against adam_ref; their gradients come back unmodified."""
    c = R.CASES[case]
    with binning(0, c["min_tiles"]) as lib:
        rng = np.random.default_rng(c["seed"])
        tab = Table(c["geom"], rng)
        small = Small(rng, R.SMALL_SIZES[:c["n_small"]])
        fails = run_steps(case, family, lib, tab, small)
    assert not fails, "\n".join(fails)


class Amp:
    """The four device words of the loss-scaling protocol, owned by the test."""

    def __init__(self, scale, found_inf, skipped):
        self.scale = torch.tensor([scale], dtype=torch.float32, device=DEV)
        self.tracker = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.found_inf = torch.tensor([found_inf], dtype=torch.int32, device=DEV)
        self.skipped = torch.tensor([skipped], dtype=torch.int32, device=DEV)

    def arm(self):
        L = _lib()
        L.check(L.lib().enerf_amp_begin(self.scale.data_ptr(), self.tracker.data_ptr(), self.found_inf.data_ptr(),
                                        self.skipped.data_ptr()), "amp_begin")


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("scenario", ["scale", "skipped2", "skipped_ge_step"])
def test_loss_scaling(scenario, family):
    """Armed with scale 1024 (gradients fed multiplied by 1024: the result equals the unscaled reference), with
    skipped = 2 from host step 3 on (Adam's t = 1, 2, 3) and with skipped >= step (t = 1 every time)."""
    c = R.CASES["amp"]
    skipped, host0 = {"scale": (0, 1), "skipped2": (2, 3), "skipped_ge_step": (7, 1)}[scenario]
    with binning(0, c["min_tiles"]) as lib:
        rng = np.random.default_rng(c["seed"])
        tab = Table(c["geom"], rng)
        small = Small(rng, R.SMALL_SIZES[:c["n_small"]])
        amp = Amp(1024.0, 0, skipped)
        amp.arm()
        assert lib.enerf_amp_armed() == 1
        fails = run_steps("amp", family, lib, tab, small, scale=1024.0, t_of=lambda s: s - skipped if s > skipped else 1,
                          host_step0=host0)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_loss_scaling_skipped_step(family):
    """found_inf = 1: table and small tensors keep p / m / v bit for bit and the dense gradient comes back zero; the next,
    unarmed step from fresh gradients equals the reference -- the lists were consumed and the cursors reset."""
    c = R.CASES["amp"]
    with binning(0, c["min_tiles"]) as lib:
        rng = np.random.default_rng(c["seed"])
        tab = Table(c["geom"], rng)
        small = Small(rng, R.SMALL_SIZES[:c["n_small"]])
        fails = run_steps("amp", family, lib, tab, small, steps=(0,))            # moments live
        amp = Amp(1024.0, 1, 0)
        amp.arm()
        before, sbefore = tab.state(), small.state()
        for x, g in R.step_inputs("amp", family, 1):
            tab.backward(x, g, c["layout"], x.shape[0], 1024.0)
        small.new_grads(rng, 1024.0)
        assert tab.adam(R.lr_of(1), 2, small) == 0
        fails += R.compare_identical(tab.state(), before, True, "skipped step: table ")
        for k, (a, b) in enumerate(zip(small.state(), sbefore)):
            fails += R.compare_identical(a, b, True, f"skipped step: small[{k}] ")
        if bool(tab.g.any()):
            fails.append("skipped step: the dense gradient buffer is not all zero")
        lib.enerf_amp_cancel()
        fails += run_steps("amp", family, lib, tab, small, steps=(2,), host_step0=0)      # host step 2: one step was skipped
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("name", sorted(R.RANGES))
def test_owner_range(name, family):
    """rec_scale = 0.5, the dense buffer pre-filled with P0 (what a reduce-scatter delivered).  After the deferred
    backward the dense buffer holds P0 + G outside every tile wholly inside the range and P0 (bit for bit) inside those
    tiles; after Adam the elements of [lo, hi) follow the reference at g = 0.5 (P0 + G), everything outside is
    bit-identical and the dense buffer is zero.  "dense": batch below the (default) binning threshold."""
    c = R.CASES["range"]
    lo, hi = R.RANGES[name]
    with binning(16384 if name == "dense" else 0, 8 if name == "dense" else c["min_tiles"]) as lib:
        tab = Table(c["geom"], np.random.default_rng(c["seed"]))
        L = _lib()
        L.check(lib.enerf_grid_owner_range(lo, hi, R.REC_SCALE), "grid_owner_range")
        fails = []
        for step in range(3):
            what = f"range {name} {family} step {step}: "
            r = R.range_reference(name, family, step)
            before = tab.state()
            tab.g.copy_(_dev(r["P0"]))
            for x, g in R.step_inputs("range", family, step):
                tab.backward(x, g, c["layout"], x.shape[0])
            dense = tab.g.cpu().numpy()
            bad = np.abs(dense.astype(np.float64) - r["dense"]) > r["d_dense"]
            if bad.any():
                fails.append(what + f"dense buffer after the backward: {int(bad.sum())} elements off, first at "
                             f"{int(np.argmax(bad.reshape(-1)))}")
            if not np.array_equal(dense[r["whole"]].view(np.uint32), r["P0"][r["whole"]].view(np.uint32)):
                fails.append(what + "a tile wholly inside the range was flushed into the dense buffer")
            lr = R.lr_of(step)
            assert tab.adam(lr, step + 1) == 0, L.lib().enerf_last_error()
            fails += R.compare_range_step(tab.state(), *before, r["G_adam"], r["dG_adam"], lo, hi, lr, R.B1, R.B2, R.EPS,
                                          step + 1, family, what)
            if bool(tab.g.any()):
                fails.append(what + "the dense gradient buffer is not all zero")
    assert not fails, "\n".join(fails)


def test_refusals():
    """Calls that must return an error and launch nothing (p bit-identical), each with records pending, which are then
    discarded: owner range with C = 4, owner range while loss scaling is armed, a range off multiples of 4, n_small = 9,
    a small tensor with step 0, loss scaling with C = 4."""
    L = _lib()
    rng = np.random.default_rng(21)
    amp = Amp(1024.0, 0, 0)

    def refused(geom, prepare, small=None, n_small=None):
        with binning(0, 8) as lib:
            tab = Table(geom, rng)
            x = R.make_samples(rng, R.FULL, tab.D)
            g = R.make_grads(rng, "signed", R.FULL, tab.L, tab.C, 0)
            prepare(lib)
            tab.backward(x, g, 1, R.FULL)
            before = tab.state()
            rc = tab.adam(R.lr_of(0), 1, small, n_small)
            torch.cuda.synchronize()
            assert rc != 0, "the call was accepted"
            assert R.compare_identical(tab.state(), before, True) == []
            L.check(lib.enerf_grid_records_discard(L.stream_handle()), "records_discard")

    refused("C4", lambda lib: L.check(lib.enerf_grid_owner_range(0, 64, 0.5), "owner_range"))

    def range_and_amp(lib):
        L.check(lib.enerf_grid_owner_range(0, 64, 0.5), "owner_range")
        amp.arm()
    refused("D2", range_and_amp)
    refused("D2", lambda lib: L.check(lib.enerf_grid_owner_range(2, 10, 0.5), "owner_range"))
    nine = Small(rng, [4] * 9)
    refused("D2", lambda lib: None, nine, 9)
    zero = Small(rng, [4, 4])
    zero.step = [3, 0]
    refused("D2", lambda lib: None, zero)
    refused("C4", lambda lib: amp.arm())
