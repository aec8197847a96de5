"""The set-up of the fused NeRF MLP kernels (csrc/nerf_mlp.hip) is one memory latency: the valid-row count, the first
tile's inputs and the operand fragments are all requested before anything waits for a loaded value.  Read off the compiled
code (hipcc cross-compiles without a GPU): between the wait for the kernel arguments and the last 16-byte fragment load in
front of the set-up barrier there is no s_waitcnt on vmcnt, and all of a thread's fragment loads sit there."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _body(text, kernel):
    m = re.search(r"^(_ZN\S*%s\S*):.*?$(.*?)^\s*\.amdhsa_kernel \1" % re.escape(kernel), text, re.S | re.M)
    assert m, f"{kernel} not found in the unit's assembly"
    return [ln.strip() for ln in m.group(2).splitlines() if ln.strip() and not ln.strip().startswith((";", "."))]


# unit, kernel (mangled-name fragment), 16-byte fragment loads per thread: fragments * 128 lanes-of-16-bytes / 256 threads
# (the matrix-pipe form k_nerf_bwd_mfma, the comparator of the bit-identity tests, shares the source but is not held to this:
#  the compiler starts its LDS stores a few loads early)
@pytest.mark.parametrize("src,kernel,nloads", [("nerf_mlp.hip", "10k_nerf_fwdE", 12), ("nerf_mlp_bwd.hip", "10k_nerf_bwdE", 20)])
def test_every_set_up_load_is_issued_before_the_first_wait(src, kernel, nloads, tmp_path):
    from enerf_amd import build
    flags = [f for f in build.FLAGS if f not in ("-fPIC",)] + build.EXTRA.get(src, [])
    out = tmp_path / (src + ".s")
    subprocess.check_call([build._hipcc()] + flags + ["-S", "--cuda-device-only", os.path.join(build.CSRC, src), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    ins = _body(out.read_text(), kernel)
    barrier = next(i for i, s in enumerate(ins) if s.startswith("s_barrier"))
    args_wait = next(i for i, s in enumerate(ins) if s.startswith("s_waitcnt") and "lgkmcnt(0)" in s)
    frag_loads = [i for i, s in enumerate(ins[:barrier]) if s.startswith("global_load_dwordx4")]
    assert args_wait < barrier and len(frag_loads) == nloads, (args_wait, barrier, len(frag_loads))
    early = [s for s in ins[args_wait + 1:frag_loads[-1]] if s.startswith("s_waitcnt") and "vmcnt" in s]
    assert not early, f"{kernel}: waits on loads in front of the last fragment load: {early}"
    # the first tile's X (eight 8-byte loads per thread) is among the requests in front of the barrier
    assert sum(1 for s in ins[:barrier] if s.startswith("global_load_dwordx2")) >= 8
