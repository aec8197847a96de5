"""Full density sweep's grid encode by route (development aid): the whole sweep on the snake deal and on each schedule,
and the walker alone.   python tools/sweep_units.py  ->  us per sweep; per-pair cost of the walker on one XCD pair."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from enerf_amd import _lib, fused_network  # noqa: E402
from enerf_amd.network import NeRFNetwork  # noqa: E402

WALK_UNIT = 0x80000000
dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = NeRFNetwork(encoding="hashgrid", bound=3, cuda_ray=True, out_dim_color=3).to(dev)
L = _lib.lib()
n_pts = model.cascade * model.grid_size ** 3
nchunks = ((n_pts + 31) // 32 * 32 + 255) // 256


def timed(mask, reps=10):
    L.enerf_debug_grid_level_mask(mask)
    sweep = lambda: fused_network.density_sigma_sweep(model, model.cascade, model.grid_size, 7)
    for _ in range(2):
        sweep()
    torch.cuda.synchronize()
    _lib.prof.reset()
    _lib.prof.enable(True, only=("grid_fwd",))
    for _ in range(reps):
        sweep()
    torch.cuda.synchronize()
    _lib.prof.enable(False)
    ms, n = _lib.prof.read("grid_fwd")
    L.enerf_debug_grid_level_mask(0xffffffff)
    return 1e3 * ms / n


def schedule(walk):
    out = np.zeros(4 * 64, np.uint32)
    n = L.enerf_debug_sweep_schedule(16, walk, nchunks, out.ctypes.data, 64)
    return out[:4 * n].reshape(n, 4)


with torch.no_grad():
    print(f"points {n_pts}, chunks per level {nchunks}")
    for route, walk in [(1, 0), (0, 0), (0, 4), (0, 5)]:
        L.enerf_debug_sweep_route(route, walk)
        line = f"route {route} walk {walk}: all levels {timed(0xffffffff):7.1f} us"
        if walk:
            segs = schedule(walk)
            share = max([n / nchunks for g, u, c0, n in segs if u == WALK_UNIT])      # the walker's busiest pair
            t = timed((1 << walk) - 1)
            line += f"   walker alone {t:7.1f} us ({share:.3f} of it on one pair: {t / share:7.1f} us per pair)"
        print(line)
        if route == 0:
            for g in range(4):
                print("   pair", g, [("W" if u == WALK_UNIT else int(u), int(c0), int(n)) for gg, u, c0, n in
                                    schedule(walk) if gg == g])
L.enerf_debug_sweep_route(0, 5)
