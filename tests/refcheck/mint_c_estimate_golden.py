"""Mint tests/golden/ref_c_estimate.npz from the reference's own `estimate_C_thres_from_pol_dL` (this container only).

    cd <repo> && python -B tests/refcheck/mint_c_estimate_golden.py

TEST INFRASTRUCTURE ONLY.  Loads the reference's utils/event_utils.py at run time -- with `h5py` and `numba`, which that
module imports and this machine does not have, replaced by empty stand-ins -- and runs its function on the CPU with the
shapes its docstring states, (N,1) polarities and (N,C) intensity differences.  Stored per case: `<name>_pols`,
`<name>_delta` (fp32) and `<name>_out` (the four medians in the order median_on, median_off, median_on_sign,
median_off_sign).  Nothing of the reference's text is kept: only these arrays.

The cases (all N <= 4097): C = 1 and 3; odd and even class counts; all-positive and all-negative polarities (empty
classes); polarity magnitudes above 1 and zeros (accumulate_evs); delta == 0 rows, which belong to both sign classes;
repeated values; one NaN; N = 1, 2, 3 (the reference's luma branch, which tests the number of events) and 4.
"""
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.ref_import import REFERENCE  # noqa: E402

NAMES = ("median_on", "median_off", "median_on_sign", "median_off_sign")


def load_reference():
    sys.dont_write_bytecode = True
    for name in ("h5py", "numba"):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules["h5py"], "File"):
        sys.modules["h5py"].File = object                # (named in an annotation only)
    if not hasattr(sys.modules["numba"], "jit"):
        sys.modules["numba"].jit = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))
    sys.path.insert(0, REFERENCE)
    import importlib
    return importlib.import_module("utils.event_utils")


def cases():
    g = np.random.default_rng(20240607)
    z = {}

    def add(name, pols, delta):
        z[name] = (np.asarray(pols, np.float32).reshape(-1, 1), np.asarray(delta, np.float32))

    def signs(n, p_pos=0.5):
        return np.where(g.random(n) < p_pos, 1.0, -1.0)

    for C in (1, 3):
        # a typical step: single polarities, deltas around +-0.2 with the wrong sign now and then
        n = 4097
        p = signs(n)
        add(f"typical_c{C}", p, p[:, None] * 0.2 + 0.15 * g.standard_normal((n, C)))
        # even and odd class counts (the lower middle element for an even count)
        for n_pos, n_neg in ((6, 5), (5, 6), (128, 129)):
            p = np.concatenate([np.ones(n_pos), -np.ones(n_neg)])
            g.shuffle(p)
            add(f"counts_{n_pos}_{n_neg}_c{C}", p, g.standard_normal((n_pos + n_neg, C)))
        add(f"all_positive_c{C}", np.ones(257), g.standard_normal((257, C)))
        add(f"all_negative_c{C}", -np.ones(256), g.standard_normal((256, C)))
        # accumulate_evs: polarity sums, zeros among them
        n = 1000
        add(f"accumulated_c{C}", g.integers(-4, 5, n).astype(np.float32), 0.3 * g.standard_normal((n, C)))
        # early in training: both renders are the background, delta is exactly zero for most events
        n = 2048
        d = 0.1 * g.standard_normal((n, C))
        d[g.random(n) < 0.8] = 0.0
        add(f"zero_rows_c{C}", signs(n), d)
        # repeated values: a few levels only
        n = 999
        add(f"repeated_c{C}", signs(n) * g.integers(1, 3, n), g.integers(-3, 4, (n, C)) * 0.125)
        # one NaN
        n = 301
        d = g.standard_normal((n, C))
        p = signs(n)
        d[17, C - 1] = np.nan
        add(f"one_nan_c{C}", p, d)
        for n in (1, 2, 3, 4):
            add(f"n{n}_c{C}", signs(n), g.standard_normal((n, C)))
            add(f"n{n}_neg_c{C}", -np.ones(n), g.standard_normal((n, C)))
    return z


def main():
    ref = load_reference()
    out = {}
    for name, (pols, delta) in cases().items():
        est = ref.estimate_C_thres_from_pol_dL(torch.from_numpy(pols), torch.from_numpy(delta))
        out[name + "_pols"], out[name + "_delta"] = pols, delta
        out[name + "_out"] = np.array([float(est[k]) for k in NAMES], np.float32)
        print(name, pols.shape, delta.shape, out[name + "_out"])
    path = os.path.join(ROOT, "tests", "golden", "ref_c_estimate.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
