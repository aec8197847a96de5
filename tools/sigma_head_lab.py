"""The density-only head (sigma net of update_extra_state) over depth x residency x non-temporal loads (development aid).

Needs a library built with the variants:  ENERF_DEFINES=-DENERF_SIG_HEAD_LAB python -m enerf_amd.build --force
(form = 1000 + 100 * NT + 10 * wavefronts per SIMD + depth; 0 = the form shipped before the load pipeline, 1 = the default).
Per form: the head's kernel time at the full sweep's and the partial update's batch (the library's own kernel-attached
events), torch.equal of sigma against form 0, and the wall time of a full update_extra_state.

usage: python tools/sigma_head_lab.py [out.json]
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from enerf_amd import _lib as L, fused_network, scene  # noqa: E402
from enerf_amd.network import NeRFNetwork  # noqa: E402

FORMS = [0, 1] + [1000 + 100 * nt + 10 * w + d for nt in (0, 1) for w in (1, 2) for d in (1, 2, 3, 4)]


def head_us(m, feats, sigma, B, reps=20):
    for _ in range(3):
        fused_network._sigma_only(m, feats, sigma, B)
    torch.cuda.synchronize()
    L.prof.reset()
    L.prof.enable(True, only=("ffmlp_fwd",))
    for _ in range(reps):
        fused_network._sigma_only(m, feats, sigma, B)
    torch.cuda.synchronize()
    L.prof.enable(False)
    ms, n = L.prof.read("ffmlp_fwd")
    return 1e3 * ms / n


def update_us(m, reps=10):
    for _ in range(2):
        m.iter_density = 0
        m.update_extra_state()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        m.iter_density = 0
        m.update_extra_state()
    t1.record()
    torch.cuda.synchronize()
    return 1e3 * t0.elapsed_time(t1) / reps


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    torch.manual_seed(0)
    lib = L.lib()
    m = NeRFNetwork(encoding="hashgrid", bound=3, cuda_ray=True, out_dim_color=3).cuda()
    scene.install_occupancy(m)
    m.train()
    rows = []
    ref = {}
    sizes = {"full": 3 * 128 ** 3, "partial": 3 * 128 ** 3 // 2}
    bufs = {}
    for name, B in sizes.items():
        Bp = fused_network.pad32(B)
        bufs[name] = (torch.randn(16, Bp, 2, device="cuda") * 0.1, torch.empty(B, device="cuda"))
    prev = lib.enerf_debug_sigma_head(-1)
    try:
        for form in FORMS:
            lib.enerf_debug_sigma_head(form)
            if lib.enerf_debug_sigma_head(-1) != form:
                print(f"form {form}: not in this build (needs -DENERF_SIG_HEAD_LAB)")
                continue
            row = {"form": form}
            for name, B in sizes.items():
                feats, sigma = bufs[name]
                row[f"head_{name}_us"] = round(head_us(m, feats, sigma, B), 2)
                if form == 0:
                    ref[name] = sigma.clone()
                row[f"equal_{name}"] = bool(torch.equal(sigma, ref[name]))
            row["update_full_us"] = round(update_us(m), 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
    finally:
        lib.enerf_debug_sigma_head(prev)
    if out:
        with open(out, "w") as f:
            json.dump({"points": sizes, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
