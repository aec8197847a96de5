"""enerf_background_forward / enerf_background_backward (csrc/background.hip) on the GPU: the stages of the forward bit for
bit against the library's own kernels, bg and the three gradients inside the fp64 intervals of tests/background_ref.py,
the weight gradients' bits across runs, and the refusals.

Every output starts as NaN between canary rows that must come back untouched.  Shapes: N = 1, 65 (one wave and a lane),
1000 (eight backward tiles, the last one ragged) and N_SLAB = 128 * 256 + 77: the backward takes tiles of 128 rays in at
most 256 workgroups, so this is the smallest ragged N at which a workgroup walks a second tile and the reducer adds all
256 rows of the slab.  Tables of 2^10 rows a level (level 0 dense, the rest hashed) and 2^19 (the model's own: three
dense levels, one hashed)."""
import functools

import numpy as np
import pytest
import torch

import background_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
CANARY = 12345.0
N_SLAB = 128 * 256 + 77

#        N, C, log2_hashmap_size, radius, view directions
CASES = [(1, 3, 10, 2.0, True),
         (65, 1, 19, 2.0, True),
         (1000, 2, 10, 5.0, False),
         (1000, 3, 19, 2.0, True),
         (N_SLAB, 3, 10, 5.0, True),
         (N_SLAB, 1, 19, 2.0, False)]
IDS = [f"N{n}-C{c}-T{t}-R{r:g}-{'dirs' if d else 'nodirs'}" for n, c, t, r, d in CASES]


def _guarded(rows, cols, fill=float("nan")):
    """-> (buffer with GUARD canary rows on either side, its interior view [rows, cols] filled with `fill`)."""
    buf = torch.full((rows + 2 * GUARD, cols), CANARY, dtype=torch.float32, device=DEV)
    buf[GUARD:GUARD + rows] = fill
    return buf, buf[GUARD:GUARD + rows]


def _intact(buf, rows):
    return bool((buf[:GUARD] == CANARY).all()) and bool((buf[GUARD + rows:] == CANARY).all())


class _Case:
    def __init__(self, N, C, log2_T, radius, dirs):
        self.N, self.C, self.radius, self.dirs = N, C, radius, dirs
        self.geo = geo = R.geometry(log2_hashmap_size=log2_T)
        self.K = 16 + 2 * geo["L"]
        self.table, self.W0, self.W1 = R.make_params(geo, C, seed=100 + C + log2_T)
        self.ro, self.rd = R.make_rays(N, radius, seed=200 + N % 1000)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
        self.d = dict(ro=t(self.ro), rd=t(self.rd), table=t(self.table), W0=t(self.W0), W1=t(self.W1),
                      offsets=t(geo["offsets"].astype(np.int32)))
        self.before = {k: v.clone() for k, v in self.d.items()}

    def inputs_unchanged(self):
        return all(torch.equal(v, self.before[k]) for k, v in self.d.items())

    def forward(self, bg, trace, **kw):
        from enerf_amd import _lib as L
        d, geo = self.d, self.geo
        a = dict(ro=d["ro"].data_ptr(), N=self.N, L=geo["L"], level_dim=2, hidden=64, C=self.C, out=bg.data_ptr())
        a.update(kw)
        return L.lib().enerf_background_forward(
            a["ro"], d["rd"].data_ptr(), self.radius, a["N"], d["table"].data_ptr(), d["offsets"].data_ptr(), a["L"],
            a["level_dim"], geo["S"], geo["H"], geo["gridtype_id"], int(self.dirs), d["W0"].data_ptr(), d["W1"].data_ptr(),
            a["hidden"], a["C"], a["out"], trace.data_ptr() if trace is not None else None, L.stream_handle())

    def backward(self, g, ws, gW0, gW1, gE, **kw):
        from enerf_amd import _lib as L
        d, geo = self.d, self.geo
        a = dict(N=self.N, L=geo["L"], level_dim=2, hidden=64, C=self.C, grad=g.data_ptr(), out=gW0.data_ptr())
        a.update(kw)
        return L.lib().enerf_background_backward(
            d["ro"].data_ptr(), d["rd"].data_ptr(), self.radius, a["N"], d["table"].data_ptr(), d["offsets"].data_ptr(),
            a["L"], a["level_dim"], geo["S"], geo["H"], geo["gridtype_id"], int(self.dirs), d["W0"].data_ptr(),
            d["W1"].data_ptr(), a["hidden"], a["C"], a["grad"], ws.data_ptr() if ws is not None else None, a["out"],
            gW1.data_ptr(), gE.data_ptr(), L.stream_handle())


@functools.lru_cache(maxsize=None)
def _forward_of(i):
    """Case i's forward, once: the case, bg, the trace, and whether every guard survived."""
    c = _Case(*CASES[i])
    bg_buf, bg = _guarded(c.N, c.C)
    tr_buf, trace = _guarded(c.N, 2 + c.K)
    assert c.forward(bg, trace) == 0
    torch.cuda.synchronize()
    assert _intact(bg_buf, c.N) and _intact(tr_buf, c.N) and c.inputs_unchanged()
    # production form: no trace, the same bits
    bg2_buf, bg2 = _guarded(c.N, c.C)
    assert c.forward(bg2, None) == 0
    assert torch.equal(bg, bg2) and _intact(bg2_buf, c.N)
    return c, bg.cpu().numpy(), trace.clone()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_stages_equal_the_librarys_own_kernels(i):
    from enerf_amd.backends import _gridencoder as gb, _raymarching as rb, _shencoder as sb
    c, _, trace = _forward_of(i)
    assert bool(torch.isfinite(trace).all())
    d, geo = c.d, c.geo
    coords = torch.full((c.N, 2), float("nan"), device=DEV)
    rb.polar_from_ray(d["ro"], d["rd"], c.radius, c.N, coords)
    assert torch.equal(trace[:, :2], coords)
    own = trace[:, :2].contiguous()
    grid = torch.full((c.N, 2 * geo["L"]), float("nan"), device=DEV)
    gb.grid_encode_forward(own, d["table"], d["offsets"], grid, c.N, 2, 2, geo["L"], geo["S"], geo["H"], False,
                           torch.empty(1, device=DEV), geo["gridtype_id"], layout=1, affine=(1.0, 0.5))
    assert torch.equal(trace[:, 18:], grid)
    sh = torch.zeros(c.N, 16, device=DEV)
    if c.dirs:
        sb.sh_encode_forward(d["rd"], sh, c.N, 3, 4, False, torch.empty(1, device=DEV))
    assert torch.equal(trace[:, 2:18], sh)
    # ... and the reference's emulation of the cells interpolates the same corners with the same weights
    want, bar = R.features(R.cells(own.cpu().numpy(), geo), c.table, geo["L"])
    assert np.all(np.abs(grid.cpu().numpy() - want) <= bar)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_bg_is_inside_the_fp64_interval(i):
    c, bg, trace = _forward_of(i)
    ref = R.reference(trace[:, 2:].cpu().numpy(), c.W0, c.W1)
    R.check(ref, dict(bg=bg), IDS[i])


@pytest.mark.parametrize("with_weights_sum", [True, False], ids=["weights_sum", "null"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_backward_is_inside_the_fp64_intervals(i, with_weights_sum):
    c, _, trace = _forward_of(i)
    x = trace[:, 2:].cpu().numpy()
    fwd = R.reference(x, c.W0, c.W1)
    share = R.assert_decided(fwd["undecided"])
    rng = np.random.default_rng(300 + i)
    g = R.mask_undecided(rng.standard_normal((c.N, c.C)).astype(np.float32), fwd["undecided"])
    ws = rng.random(c.N).astype(np.float32) if with_weights_sum else None
    cell = R.cells(trace[:, :2].cpu().numpy(), c.geo)
    rows = c.table.shape[0]
    ref = R.reference(x, c.W0, c.W1, g, ws, cell, rows)
    tg = torch.from_numpy(g).to(DEV)
    tws = torch.from_numpy(ws).to(DEV) if ws is not None else None
    runs = []
    for _ in range(2):
        b0, gW0 = _guarded(64, c.K)
        b1, gW1 = _guarded(c.C, 64)
        bE, gE = _guarded(rows, 2, fill=0.0)
        assert c.backward(tg, tws, gW0, gW1, gE) == 0
        torch.cuda.synchronize()
        assert _intact(b0, 64) and _intact(b1, c.C) and _intact(bE, rows) and c.inputs_unchanged()
        runs.append((gW0.clone(), gW1.clone(), gE.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    print(f"undecided rays: {share:.4f}")
    for gW0, gW1, gE in runs:
        got = dict(dW0=gW0.cpu().numpy(), dW1=gW1.cpu().numpy(), dE=gE.cpu().numpy())
        R.check(ref, got, f"{IDS[i]} ws={with_weights_sum}")
        assert ref["touched"].any() and not np.any(got["dE"][~ref["touched"]])


def test_refusals_write_nothing():
    c, _, _ = _forward_of(2)
    rows = c.table.shape[0]
    bufs = [_guarded(c.N, 3), _guarded(c.N, 2 + 16 + 2 * 9), _guarded(64, 16 + 2 * 9), _guarded(3, 64), _guarded(rows, 2)]
    (_, bg), (_, trace), (_, gW0), (_, gW1), (_, gE) = bufs
    g = torch.ones(c.N, 3, device=DEV)
    for kw in (dict(C=0), dict(C=4), dict(hidden=32), dict(hidden=128), dict(level_dim=1), dict(level_dim=4), dict(L=0),
               dict(L=9)):
        assert c.forward(bg, trace, **kw) != 0, kw
        assert c.backward(g, None, gW0, gW1, gE, **kw) != 0, kw
    assert c.forward(bg, trace, ro=None) != 0 and c.forward(bg, trace, out=None) != 0
    assert c.backward(g, None, gW0, gW1, gE, grad=None) != 0 and c.backward(g, None, gW0, gW1, gE, out=None) != 0
    # no rays: success, and nothing is touched either
    assert c.forward(bg, trace, N=0) == 0 and c.backward(g, None, gW0, gW1, gE, N=0) == 0
    torch.cuda.synchronize()
    for buf, inner in bufs:
        assert bool(torch.isnan(inner).all()) and _intact(buf, inner.shape[0])
    assert c.inputs_unchanged()
