"""The parameters' exponential moving average on one GPU: ParamEMA.update() (csrc/optim.hip k_ema_multi, one launch over
all tensors) beside `ema_statement` (torch_ema's three elementwise statements per tensor) over the same tensors.

Shape: the parameters of BASELINE configs[1], i.e. of bench.py's model -- the hash table L16 F2 T2^19 at bound 3 plus the
nn.Linear nets.  Five rounds, the two variants alternating within a round; per round and variant 100 repetitions after a
warm-up, device time between two events around the repetitions (and the host's enqueue time around the same loop).  Every
round is one JSON line, appended to `--out` (profiles/ema_bench.jsonl) and printed; the kernel's line also carries its
bytes/s at 12 B/parameter (read s, read p, write s) and that as a share of the measured HBM peak.

The two tensors of the table (2 x 52 MB) fit in the 256 MiB Infinity Cache, and back-to-back repetitions find them there;
an update that runs once per epoch does not.  So after the rounds each variant is timed `--cold` more times one update
at a time, every one behind a pass over a 512 MiB buffer that evicts the cache (events around the single update: a
24 us window, so these lines are coarser); they are the figure to hold against the HBM peak.

    python tools/bench_ema.py [--rounds 5] [--reps 100] [--cold 20] [--out profiles/ema_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from enerf_amd.ema import ParamEMA, ema_statement  # noqa: E402

DEV = "cuda"
HBM_PEAK_GBS = 6290.0           # measured float4 copy on an MI355X (8.0 TB/s on paper)
BYTES_PER_PARAM = 12


def timed(fn, reps, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps, host * 1e6 / reps            # microseconds per repetition


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--cold", type=int, default=20, help="single updates behind a cache-evicting pass, per variant")
    ap.add_argument("--bound", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema: no GPU (this tool measures, it has no other mode)")
    from enerf_amd.network import NeRFNetwork
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=a.bound, cuda_ray=True, out_dim_color=3).to(DEV)
    params = list(model.parameters())
    n = sum(p.numel() for p in params)
    ema = ParamEMA(params, 0.95)
    ema.num_updates = 500                                    # (past the warm-up: every repetition uses 0.95)
    shadows = [p.detach().clone() for p in params]
    omd = 1.0 - 0.95

    def statement():
        for s, p in zip(shadows, params):
            ema_statement(s, p.detach(), omd)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        def emit(**kw):
            line = json.dumps(kw)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        emit(what="device", name=torch.cuda.get_device_name(0), torch=torch.__version__, tensors=len(params),
             parameters=n, sizes=[p.numel() for p in params], reps=a.reps)
        for r in range(a.rounds):
            for variant, fn in (("kernel", ema.update), ("statement", statement)):
                dev_us, host_us = timed(fn, a.reps)
                extra = {}
                if variant == "kernel":
                    gbs = n * BYTES_PER_PARAM / (dev_us * 1e-6) / 1e9
                    extra = dict(gbytes_per_s=gbs, share_of_hbm_peak=gbs / HBM_PEAK_GBS)
                emit(what="round", round=r, variant=variant, device_us=dev_us, host_us=host_us, **extra)
        if a.cold > 0:
            evict = torch.zeros(512 << 20, dtype=torch.uint8, device=DEV)
            for variant, fn in (("kernel", ema.update), ("statement", statement)):
                us = []
                for _ in range(a.cold):
                    evict.add_(1)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    us.append(e0.elapsed_time(e1) * 1e3)
                us.sort()
                med = us[len(us) // 2]
                extra = {}
                if variant == "kernel":
                    gbs = n * BYTES_PER_PARAM / (med * 1e-6) / 1e9
                    extra = dict(gbytes_per_s=gbs, share_of_hbm_peak=gbs / HBM_PEAK_GBS)
                emit(what="cold", variant=variant, updates=a.cold, device_us_median=med, device_us_min=us[0],
                     device_us_max=us[-1], **extra)


if __name__ == "__main__":
    main()
