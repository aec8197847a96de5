"""The density update's cell selection (csrc/density_update.hip: enerf_density_grid_cells -- occupied list, key draw, bucket
sort, positions; csrc/sweep_points.h) against its exact host statement, tests/density_cells_ref.py.  Nothing in the pass
is random once the seed is given, so every comparison is an equality: Morton indices element for element, positions bit
for bit.  Each case asserts, on the statement alone, the precondition that makes it reach its branch of the kernels (the
same assertions run without a GPU in tests/test_density_cells_ref.py).  The one margin in this file is the 1e-6 on
mean_density that test_grid_update_matches_oracle already uses."""
import ctypes

import numpy as np
import pytest
import torch

import density_cells_ref as R
from oracle import density_update as OD
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
E_BADARG = -1               # include/enerf_hip.h: ENERF_E_BADARG
M64 = 2 ** 64 - 1


def _L():
    from enerf_amd import _lib as L
    return L


def _buffers(P):
    """Outputs for P points: sentinel / NaN filled, over-allocated by R.PAD elements (points, for the positions)."""
    idx = torch.full((P + R.PAD,), R.IDX_SENTINEL, dtype=torch.int32, device=DEV)
    xyz = torch.full((P + R.PAD, 3), float("nan"), dtype=torch.float32, device=DEV)
    return idx, xyz


def _call(grid, C, H, bound, n, seed, out):
    """One enerf_density_grid_cells call on torch's current stream; returns its code without synchronising."""
    L = _L()
    return L.lib().enerf_density_grid_cells(None if grid is None else grid.data_ptr(), C, H, float(bound), n,
                                            ctypes.c_uint64(seed & M64), out[0].data_ptr(), out[1].data_ptr(),
                                            L.stream_handle())


def _untouched(out):
    return bool((out[0] == R.IDX_SENTINEL).all()) and bool(torch.isnan(out[1]).all())


def _used(out, P):
    """The used part on the host, after asserting that all of it was written and nothing behind it."""
    idx, xyz = out
    assert _untouched((idx[P:], xyz[P:])), "the call wrote behind its outputs"
    assert not bool((idx[:P] == R.IDX_SENTINEL).any()), "an index was never written"
    assert not bool(torch.isnan(xyz[:P]).any()), "a position was never written"
    return idx[:P].cpu().numpy(), xyz[:P].cpu().numpy()


_statements = {}


def _statement(case):
    """The case's statement, computed once (the two 256^3 grids are not kept)."""
    if case.name in _statements:
        return _statements[case.name]
    st = case.statement()
    if st["grid"].nbytes <= 64 << 20:
        _statements[case.name] = st
    return st


def _run_case(case, st, grid=None, seed=None, sync=True):
    grid = torch.from_numpy(st["grid"]).to(DEV) if grid is None else grid
    out = _buffers(case.P)
    rc = _call(grid, case.C, case.H, case.bound, case.n, case.seed if seed is None else seed, out)
    assert rc == 0, _L().lib().enerf_last_error().decode("utf-8", "replace")
    if sync:
        torch.cuda.synchronize()
    return grid, out


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_partial_update_cells_equal_the_statement(case):
    st = _statement(case)
    case.assert_precondition(st)
    grid, out = _run_case(case, st)
    idx, xyz = _used(out, case.P)
    verdict = R.compare(idx, xyz, st["idx"], st["xyz"])
    assert verdict is None, verdict
    _, again = _run_case(case, st, grid=grid)                                 # the same seed: the same bits
    assert torch.equal(again[0], out[0]) and torch.equal(again[1].view(torch.int32), out[1].view(torch.int32))
    _, other = _run_case(case, st, grid=grid, seed=(case.seed + 1) & M64)     # another seed: another answer
    assert not (torch.equal(other[0], out[0]) and torch.equal(other[1].view(torch.int32), out[1].view(torch.int32)))
    _used(other, case.P)


@pytest.mark.parametrize("order", [("all_buckets", "one_bucket_n4097"), ("one_bucket_n4097", "all_buckets")])
def test_back_to_back_calls_of_another_bucket_geometry(order):
    """Two calls on one stream with nothing between them: the second finds the first's bucket counters, cursors and
    bases (4096 buckets against 1) in the workspace they share, and both equal their own statements."""
    cases = [R.CASE[name] for name in order]
    sts = [_statement(c) for c in cases]
    assert {R.sort_geometry(c.C, c.H)[2] for c in cases} == {1, 4096}
    grids = [torch.from_numpy(st["grid"]).to(DEV) for st in sts]
    torch.cuda.synchronize()
    outs = [_run_case(c, st, grid=g, sync=False)[1] for c, st, g in zip(cases, sts, grids)]
    torch.cuda.synchronize()
    for c, st, out in zip(cases, sts, outs):
        verdict = R.compare(*_used(out, c.P), st["idx"], st["xyz"])
        assert verdict is None, (c.name, verdict)


@pytest.mark.parametrize("bound,H", R.FULL_SWEEPS)
def test_full_sweep_cells_equal_the_statement(bound, H):
    C = 1 + int(np.ceil(np.log2(bound)))
    P, seed = C * H ** 3, 0xC0FFEE0123456789
    want_idx, want_xyz = R.cells_full(C, H, bound, seed)
    out = _buffers(P)
    assert _call(None, C, H, bound, 0, seed, out) == 0
    torch.cuda.synchronize()
    verdict = R.compare(*_used(out, P), want_idx, want_xyz)
    assert verdict is None, verdict
    again = _buffers(P)
    assert _call(None, C, H, bound, 12345, seed, again) == 0                  # (n_uniform plays no part in a full sweep)
    assert torch.equal(again[0], out[0]) and torch.equal(again[1].view(torch.int32), out[1].view(torch.int32))
    other = _buffers(P)
    assert _call(None, C, H, bound, 0, seed + 1, other) == 0
    assert torch.equal(other[0], out[0]) and not torch.equal(other[1][:P], out[1][:P])    # same cells, other jitter


@pytest.mark.parametrize("C,H,n", [(5, 256, 8), (9, 16, 8), (1, 8, 8), (1, 48, 8), (1, 16, 2 ** 30), (8, 16, 2 ** 28)],
                         ids=["27_key_bits", "nine_cascades", "H8", "H48", "2n_is_2^31", "8_x_2n_is_2^32"])
def test_refused_calls_leave_the_outputs_alone(C, H, n):
    # (the grid has the size the call would read, were it not refused)
    grid = torch.zeros(C * H ** 3, dtype=torch.float32, device=DEV)
    grid[::7] = 0.5
    out = _buffers(64)
    assert _call(grid, C, H, 2.0, n, 3, out) == E_BADARG
    torch.cuda.synchronize()
    assert _untouched(out)
    if (C, H) == (5, 256):
        # the bits of the cascade number are ceil(log2 C): three cascades of 256^3 cells are 26 bits and are served
        assert R.sort_geometry(3, 256)[:2] == (26, 14) and R.sort_geometry(5, 256)[0] == 27


def test_no_samples_with_a_grid_is_no_work():
    grid = torch.full((2 * 32 ** 3,), 0.5, dtype=torch.float32, device=DEV)
    out = _buffers(64)
    assert _call(grid, 2, 32, 2.0, 0, 3, out) == 0
    torch.cuda.synchronize()
    assert _untouched(out)


def test_update_extra_state_evaluates_the_statements_cells():
    """The partial update end to end: the cells and positions of the statement, through the model's own sigma kernel,
    through oracle.density_update.apply_update, are the grid update_extra_state leaves behind -- bit for bit wherever a
    cell was drawn once or not at all; a cell drawn k times holds the result of one of its k sigmas."""
    from enerf_amd import density_update, scene
    from enerf_amd.network import NeRFNetwork
    torch.manual_seed(20)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3).to(DEV)
    model.encoder.embeddings.data.uniform_(-1.0, 1.0)
    scene.install_occupancy(model)
    model.iter_density = 16
    assert density_update.supported(model)
    C, H = int(model.cascade), int(model.grid_size)
    H3, n = H ** 3, H ** 3 // 4
    seed = ((torch.initial_seed() + 1) * density_update._GOLDEN + 16 * 0xD1B54A32D192ED03) & M64
    old = model.density_grid.cpu().numpy().copy()
    idx, xyz = R.cells_partial(old, C, H, float(model.bound), n, seed)
    sig = density_update._sigmas(model, torch.from_numpy(xyz).to(DEV)).cpu().numpy()
    sig = np.nan_to_num(sig, nan=-1.0).reshape(C, 2 * n)
    idx = idx.reshape(C, 2 * n)
    scale, decay, thresh = model.density_scale * 0.003383, 0.95, model.density_thresh

    model.update_extra_state()
    torch.cuda.synchronize()
    new = model.density_grid.cpu().numpy()
    assert model.iter_density == 17

    first, drawn = [], np.zeros((C, H3), np.int64)
    for cas in range(C):
        cells, where, count = np.unique(idx[cas], return_index=True, return_counts=True)
        first.append((cells, sig[cas][where]))
        drawn[cas, cells] = count
    want, _, _ = OD.apply_update(old, [f[0] for f in first], [f[1] for f in first], scale, decay, thresh)
    once = drawn <= 1
    assert (drawn == 1).any() and (drawn > 1).any() and (drawn == 0).any()
    assert np.array_equal(new[once].view(np.uint32), want[once].view(np.uint32))
    assert np.array_equal(new[drawn == 0].view(np.uint32), old[drawn == 0].view(np.uint32))   # not drawn: as the oracle has it
    # drawn k > 1 times: some writer wins.  Every point's own outcome (the oracle's expression, :541-542, per point;
    # equal to the oracle's grid wherever it is the only one) ...
    f = np.float32
    for cas in range(C):
        g = old[cas][idx[cas]]
        t = sig[cas].astype(np.float32) * f(scale)
        outcome = np.where((g >= 0) & (t >= 0), np.maximum(g * f(decay), t), g).astype(np.float32)
        single = once[cas][idx[cas]]
        assert np.array_equal(outcome[single], want[cas][idx[cas]][single])
        # ... and the new value of every cell is the outcome of at least one of its points
        hit = np.zeros(H3, bool)
        match = outcome.view(np.uint32) == new[cas][idx[cas]].view(np.uint32)
        hit[idx[cas][match]] = True
        assert hit[drawn[cas] > 0].all()

    want_mean = float(np.mean(np.clip(new, 0, None), dtype=np.float64))
    assert abs(model.mean_density - want_mean) <= 1e-6 * want_mean
    level = min(want_mean, thresh)
    want_bits = np.unpackbits(O.packbits(new.reshape(-1), np.float32(level)), bitorder="little")
    got_bits = np.unpackbits(model.density_bitfield.cpu().numpy(), bitorder="little")
    near = np.abs(np.clip(new.reshape(-1), 0, None) - level) < 1e-7
    assert np.array_equal(got_bits[~near], want_bits[~near])
