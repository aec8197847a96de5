"""Mint tests/golden/ref_event_accumulation.npz from the reference's own `render_ev_accumulation` (this container only).

    cd <repo> && python -B tests/refcheck/mint_event_accumulation_golden.py

TEST INFRASTRUCTURE ONLY.  Loads the reference's utils/plot_utils.py at run time -- every package that module imports and
this machine does not have replaced by an empty stand-in, and `np.int`, which the function uses and numpy no longer has,
aliased to `int` -- and runs its function on seeded tiny inputs.  Stored per case: `<name>_x`, `<name>_y`, `<name>_pol`
(the inputs as handed over) and `<name>_img` (uint8 [H, W, 3], what it returned); `H`, `W`.  Nothing of the reference's
text is kept: only these arrays.

The cases, all on a 6 x 8 sensor: integer sensor coordinates with every pixel repeated under both polarities (the last
event must win) in -1/+1 and in 0/1 polarities; float coordinates (a rectify map's output) with negatives, values in
[W - 1, W) and [H - 1, H), values at and beyond W / H; a single event; all events on one pixel with alternating polarity.
"""
import importlib
import os
import sys
from unittest.mock import MagicMock

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from oracle.ref_import import REFERENCE  # noqa: E402

H, W = 6, 8


def load_reference():
    sys.dont_write_bytecode = True
    if not hasattr(np, "int"):
        np.int = int
    sys.path.insert(0, REFERENCE)
    for _ in range(64):
        try:
            return importlib.import_module("utils.plot_utils")
        except ModuleNotFoundError as e:                                   # a package this machine does not have
            if e.name is None or e.name.startswith("utils"):
                raise
            sys.modules[e.name] = MagicMock()
    raise RuntimeError("utils.plot_utils does not import")


def cases():
    g = np.random.default_rng(20240911)
    z = {}
    n = 400
    x, y = g.integers(0, W, n), g.integers(0, H, n)
    z["sensor_pm1"] = (x.astype(np.uint16), y.astype(np.uint16), g.choice(np.array([-1, 1], np.int8), n))
    z["sensor_01"] = (x.astype(np.int64), y.astype(np.int64), g.integers(0, 2, n).astype(np.int8))
    xf = g.uniform(-2.0, W + 2.0, n).astype(np.float32)
    yf = g.uniform(-2.0, H + 2.0, n).astype(np.float32)
    xf[:12] = [-0.25, -1.0, W - 1, W - 0.5, np.nextafter(np.float32(W), np.float32(0)), W, W + 0.5, 0.0, 0.999, 3.5, W - 1, 2.0]
    yf[:12] = [1.0, 2.0, 0.0, H - 0.5, H - 1, 1.0, 1.0, -0.001, np.nextafter(np.float32(H), np.float32(0)), H, H + 3.0, -5.0]
    z["float_coords"] = (xf, yf, g.choice(np.array([-1, 1], np.int8), n))
    z["single"] = (np.array([W - 1], np.uint16), np.array([H - 1], np.uint16), np.array([1], np.int8))
    k = 33
    z["one_pixel"] = (np.full(k, 3, np.uint16), np.full(k, 2, np.uint16), np.where(np.arange(k) % 2 == 0, 1, -1).astype(np.int8))
    return z


def main():
    ref = load_reference()
    out = {"H": np.int64(H), "W": np.int64(W)}
    for name, (x, y, pol) in cases().items():
        img = ref.render_ev_accumulation(x.copy(), y.copy(), pol.copy(), H, W)
        out[name + "_x"], out[name + "_y"], out[name + "_pol"], out[name + "_img"] = x, y, pol, img
        print(name, x.dtype, x.shape, img.dtype, img.shape, int((img != 255).any(-1).sum()), "cells painted")
    path = os.path.join(ROOT, "tests", "golden", "ref_event_accumulation.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
