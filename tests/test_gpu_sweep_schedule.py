"""The full sweep's placement (enerf_grid_encode_forward_sweep, csrc/gridencoder.hip): the static schedule over the XCD
pairs and the coarse-level walker change where and how often the query point is generated, never a bit of what is
computed.  Compared against the training forward on the points enerf_density_grid_cells writes, and against the
whole-level snake deal (enerf_debug_sweep_route(1, 0)) through update_extra_state."""
import ctypes

import numpy as np
import pytest
import torch

WALK_UNIT = 0x80000000
ROUTES = [(0, 0), (0, 4), (0, 5), (1, 0)]          # (route, walked levels) of enerf_debug_sweep_route
DEFAULT_ROUTE = (0, 5)


def _L():
    from enerf_amd import _lib as L
    return L


def _schedule(L_levels, walk, nchunks):
    out = np.zeros(4 * 64, np.uint32)
    n = _L().lib().enerf_debug_sweep_schedule(L_levels, walk, nchunks, out.ctypes.data, 64)
    assert n > 0, (L_levels, walk, nchunks)
    return out[:4 * n].reshape(n, 4).astype(np.int64)


@pytest.mark.parametrize("walk", [0, 4, 5])
@pytest.mark.parametrize("nchunks", [1, 3, 97, 24576])
def test_schedule_covers_every_level_and_point_once(walk, nchunks):
    """CPU: for every level count the schedule's segments cover each (level, chunk) exactly once; the walker's unit
    stands for levels 0 .. min(walk, L) - 1; the four pairs carry about the same cost."""
    from enerf_amd import build
    build.build(verbose=False)
    for L_levels in range(1, 17):
        segs = _schedule(L_levels, walk, nchunks)
        walked = min(walk, L_levels)
        seen = np.zeros((L_levels, nchunks), np.int32)
        assert list(segs[:, 0]) == sorted(segs[:, 0]) and segs[:, 0].max() < 4       # grouped by pair
        for g, unit, c0, n in segs:
            assert n >= 1 and c0 + n <= nchunks
            levels = range(walked) if unit == WALK_UNIT else [unit]
            if unit != WALK_UNIT:
                assert walked <= unit < L_levels
            else:
                assert walked > 0
            for lv in levels:
                seen[lv, c0:c0 + n] += 1
        assert (seen == 1).all(), (L_levels, walk, nchunks)
    if nchunks == 24576:
        # the 16-level schedule: no pair carries more than 1 % over the mean of the table's costs
        segs = _schedule(16, walk, nchunks)
        lv_us = [264.2, 256.0, 258.0, 264.2, 259.3, 273.3, 277.9, 328.9, 394.1, 501.5, 591.6, 655.3, 683.6, 697.8,
                 700.1, 704.0]
        walk_us = {4: 463.2, 5: 531.5}
        load = np.zeros(4)
        for g, unit, c0, n in segs:
            load[g] += (walk_us[walk] if unit == WALK_UNIT else lv_us[unit]) * n / nchunks
        assert load.max() <= 1.01 * load.mean(), load


@pytest.fixture
def sweep_route():
    L = _L()

    def set_route(route, walk):
        L.check(L.lib().enerf_debug_sweep_route(route, walk), "debug_sweep_route")

    yield set_route
    set_route(*DEFAULT_ROUTE)
    L.lib().enerf_debug_grid_level_mask(0xffffffff)


def _model(bound):
    from enerf_amd.network import NeRFNetwork
    torch.manual_seed(11)
    m = NeRFNetwork(encoding="hashgrid", bound=bound, cuda_ray=True, out_dim_color=3).cuda()
    m.encoder.embeddings.data.uniform_(-1.0, 1.0)
    return m


def _sweep(model, C, H, seed, out):
    L = _L()
    enc = model.encoder
    S = float(np.log2(enc.per_level_scale))
    aff = (float(model.bound), float(np.float32(1.0) / np.float32(2 * model.bound)))
    L.check(L.lib().enerf_grid_encode_forward_sweep(enc.embeddings.detach().data_ptr(), enc.offsets.data_ptr(),
                                                    out.data_ptr(), C, H, float(model.bound), ctypes.c_uint64(seed), 2,
                                                    16, S, int(enc.base_resolution), int(enc.gridtype_id), 2, aff[0],
                                                    aff[1], L.stream_handle()), "sweep")
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("bound", [2, 3])
@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("H", [64, 128])
def test_sweep_features_equal_the_training_forward_on_every_route(sweep_route, bound, C, H):
    """Every route's features equal enerf_grid_encode_forward's on the points enerf_density_grid_cells writes, level by
    level, bit for bit; with a level mask, exactly the masked-in levels are written."""
    from enerf_amd.backends import _gridencoder as gb
    L = _L()
    model = _model(bound)
    enc = model.encoder
    P, seed = C * H ** 3, 0x0DDBA11CAFEF00D + 977 * H + C
    idx = torch.empty(P, dtype=torch.int32, device="cuda")
    xyz = torch.empty(P, 3, dtype=torch.float32, device="cuda")
    L.check(L.lib().enerf_density_grid_cells(None, C, H, float(bound), H ** 3 // 4, ctypes.c_uint64(seed),
                                             idx.data_ptr(), xyz.data_ptr(), L.stream_handle()), "cells")
    S = float(np.log2(enc.per_level_scale))
    aff = (float(bound), float(np.float32(1.0) / np.float32(2 * bound)))
    Pp = (P + 31) // 32 * 32
    want = torch.full((16, Pp, 2), 7.0, device="cuda")
    gb.grid_encode_forward(xyz, enc.embeddings.detach(), enc.offsets, want, P, 3, 2, 16, S, enc.base_resolution, False,
                           want, enc.gridtype_id, layout=2, affine=aff)
    del idx, xyz
    got = torch.empty_like(want)
    for route, walk in ROUTES:
        sweep_route(route, walk)
        got.fill_(-7.0)
        _sweep(model, C, H, seed, got)
        for lv in range(16):
            assert torch.equal(got[lv], want[lv]), (route, walk, lv)
    if C == 3:
        for walk in (4, 5):
            low = (1 << walk) - 1
            for mask in (low, 0xffff & ~low):
                sweep_route(0, walk)
                L.lib().enerf_debug_grid_level_mask(mask)
                got.fill_(-7.0)
                _sweep(model, C, H, seed, got)
                L.lib().enerf_debug_grid_level_mask(0xffffffff)
                for lv in range(16):
                    if (mask >> lv) & 1:
                        assert torch.equal(got[lv], want[lv]), (walk, hex(mask), lv)
                    else:
                        assert bool((got[lv] == -7.0).all()), (walk, hex(mask), lv)


@pytest.mark.gpu
@pytest.mark.parametrize("bound", [2, 3])
def test_three_full_updates_equal_the_snake_deal(sweep_route, bound):
    """Three consecutive full update_extra_state calls (iter_density < 16): the same density_grid, bitfield and
    mean_density on the snake deal and on every schedule."""
    states = []
    for route, walk in ROUTES[::-1]:
        sweep_route(route, walk)
        m = _model(bound)
        m.local_step = 5
        m.step_counter[:5, 0] = torch.tensor([100, 200, 300, 400, 500], dtype=torch.int32)
        means = []
        for _ in range(3):
            assert m.iter_density < 16
            m.update_extra_state()
            means.append(m.mean_density)
        torch.cuda.synchronize()
        states.append((m.density_grid.clone(), m.density_bitfield.clone(), means))
    for g, bits, means in states[1:]:
        assert torch.equal(g, states[0][0]) and torch.equal(bits, states[0][1]) and means == states[0][2]
