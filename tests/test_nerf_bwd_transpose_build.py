"""What the compiler made of the two forms of the fused MLP backward (csrc/nerf_mlp.hip, compiled as nerf_mlp_bwd.hip): the
default, k_nerf_bwd, transposes the operands of its weight-gradient products with ds_read_b64_tr_b16 instead of the 60
selection-matrix MFMAs per tile that k_nerf_bwd_mfma spends on them, still claims more than half of a CU's LDS (one
workgroup per CU: the kernel is built without the operand barrier) and keeps everything in registers.  The device code is
compiled to assembly here (hipcc cross-compiles without a GPU)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    from enerf_amd import build
    src = "nerf_mlp_bwd.hip"
    flags = [f for f in build.FLAGS if f not in ("-fPIC",)] + build.EXTRA.get(src, [])
    out = tmp_path_factory.mktemp("nerf_bwd") / (src + ".s")
    subprocess.check_call([build._hipcc()] + flags + ["-S", "--cuda-device-only", os.path.join(build.CSRC, src), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    return out.read_text()


def _kernel(text, name):
    """-> (instructions of the kernel whose mangled name holds `name`, its descriptor + metadata fields)."""
    m = re.search(r"^(_Z\w*" + name + r"E\w*):.*\n([\s\S]*?)^\.Lfunc_end", text, re.M)
    assert m, f"{name} not found in the unit's assembly"
    sym = m.group(1)
    ins = [ln.split(";")[0].strip() for ln in m.group(2).splitlines()]
    ins = [i for i in ins if i and not i.startswith(".")]
    meta = {}
    d = re.search(r"\.amdhsa_kernel " + sym + r"\n([\s\S]*?)\.end_amdhsa_kernel", text)
    assert d, "no kernel descriptor"
    for key in ("group_segment_fixed_size", "private_segment_fixed_size", "uses_dynamic_stack"):
        meta[key] = int(re.search(r"\.amdhsa_" + key + r" (\d+)", d.group(1)).group(1))
    y = re.search(r"\.name:\s+" + sym + r"\n([\s\S]*?)\.wavefront_size", text)
    assert y, "no metadata entry"
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        meta["md_" + key] = int(re.search(r"\." + key + r":\s+(\d+)", y.group(1)).group(1))
    return ins, meta


def _count(ins, prefix):
    return sum(1 for i in ins if i.startswith(prefix))


def test_default_backward_transposes_through_lds(asm):
    lds_form, meta = _kernel(asm, "k_nerf_bwd")
    pipe_form, _ = _kernel(asm, "k_nerf_bwd_mfma")
    assert _count(lds_form, "ds_read_b64_tr_b16") > 0
    assert _count(pipe_form, "ds_read_b64_tr_b16") == 0
    n_lds, n_pipe = _count(lds_form, "v_mfma_f32_32x32x16_bf16"), _count(pipe_form, "v_mfma_f32_32x32x16_bf16")
    assert n_pipe - n_lds == 60, (n_pipe, n_lds)           # 14 flip_tile x 4 + 2 flip_natural x 2 per tile
    assert 80 * 1024 < meta["group_segment_fixed_size"] <= 160 * 1024, meta
    assert meta["md_vgpr_spill_count"] == 0 and meta["md_sgpr_spill_count"] == 0, meta
    assert meta["private_segment_fixed_size"] == 0 and meta["md_private_segment_fixed_size"] == 0, meta
    assert meta["uses_dynamic_stack"] == 0, meta
    assert not [i for i in lds_form if i.startswith(("scratch_", "buffer_"))], "scratch memory instructions"
