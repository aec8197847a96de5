"""enerf_density_grid_update after a full sweep (csrc/density_update.hip).  With indices == NULL the sigmas are those of
the sweep's own point order (x fastest per cascade), every cell gets exactly one new value, and one kernel reads them in
place of the fill + scatter + EMA over a temporary grid that the path with explicit indices takes.  The loop, the launch
geometry and the order of every sum are the same, so the same sweep handed over with its explicit Morton indices must
leave the same density grid, the same bitfield and the same two statistics, bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _sweep_indices(C, H):
    """Morton index of point p of the sweep: cell = p mod H^3, x = cell mod H fastest, then y, then z."""
    from enerf_amd.backends import _raymarching as rm
    cell = torch.arange(H ** 3, dtype=torch.int32, device=DEV)
    coords = torch.stack([cell % H, (cell // H) % H, cell // (H * H)], dim=-1).to(torch.int32).contiguous()
    idx = torch.empty(H ** 3, dtype=torch.int32, device=DEV)
    rm.morton3D(coords, H ** 3, idx)
    torch.cuda.synchronize()
    assert torch.equal(torch.sort(idx.long()).values, torch.arange(H ** 3, device=DEV))
    return idx.repeat(C).contiguous()


def _update(indices, sigmas, C, H, grid, counter, total_step):
    from enerf_amd import _lib as L
    g = grid.clone()
    bits = torch.zeros(C * H ** 3 // 8, dtype=torch.uint8, device=DEV)
    stats = torch.full((2,), -7.0, dtype=torch.float64, device=DEV)
    L.check(L.lib().enerf_density_grid_update(None if indices is None else indices.data_ptr(), sigmas.data_ptr(), H ** 3, C, H,
                                              0.003383 * 1.5, 0.95, 0.01, g.data_ptr(), bits.data_ptr(),
                                              counter.data_ptr(), total_step, stats.data_ptr(), L.stream_handle()),
            "density_grid_update")
    torch.cuda.synchronize()
    return g, bits, stats


@pytest.mark.parametrize("total_step", [0, 3])
@pytest.mark.parametrize("H", [16, 32])
def test_the_full_sweep_tail_equals_the_update_with_explicit_indices(H, total_step):
    C, H3 = 3, H ** 3
    rng = np.random.default_rng(100 * H + total_step)
    grid = (rng.random((C, H3)) ** 4 * 0.05).astype(np.float32)
    grid[rng.random((C, H3)) < 0.3] = 0.0
    grid[rng.random((C, H3)) < 0.05] = -1.0                                   # mark_untrained_grid cells
    sigmas = (rng.random((C, H3)) ** 3 * 40).astype(np.float32)
    sigmas[rng.random((C, H3)) < 0.2] = 0.0
    counter = rng.integers(1000, 500000, size=(16, 2)).astype(np.int32)
    d_grid, d_sig, d_cnt = (torch.from_numpy(a).to(DEV) for a in (grid, sigmas, counter))
    assert int((d_grid > 0).sum()) and int((d_grid == 0).sum()) and int((d_grid == -1).sum()) and int((d_sig == 0).sum())
    g0, b0, s0 = _update(None, d_sig, C, H, d_grid, d_cnt, total_step)
    g1, b1, s1 = _update(_sweep_indices(C, H), d_sig, C, H, d_grid, d_cnt, total_step)
    assert torch.equal(g0.view(torch.int32), g1.view(torch.int32)), int((g0 != g1).sum())
    assert torch.equal(b0, b1), int((b0 != b1).sum())
    assert torch.equal(s0.view(torch.int64), s1.view(torch.int64)), (s0.tolist(), s1.tolist())
    # the update did something: cells changed, untrained cells did not, some bits are set and some are not
    assert int((g0 != d_grid).sum()) > H3 // 4 and torch.equal(g0 == -1, d_grid == -1)
    assert 0 < int((b0 != 0).sum()) and int((b0 != 255).sum()) > 0
    assert s0[0].item() > 0 and s0[1].item() == float(counter[:total_step, 0].sum())
