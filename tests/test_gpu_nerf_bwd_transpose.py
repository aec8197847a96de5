"""k_nerf_bwd (csrc/nerf_mlp.hip) transposes the operands of its weight-gradient products either on the matrix pipe
(enerf_debug_nerf_bwd_transpose(0): products with 0/1 selection matrices) or through per-wave LDS images read back with
ds_read_b64_tr_b16 (1, the default).  Both hand every weight-gradient MFMA the same operand bits, so the feature gradient
and the ten weight gradients must be equal under torch.equal (a transpose through LDS keeps a -0 that a multiply by 1.0
turns into +0; torch.equal counts the two as equal, which is intended).  The entry points are called directly: the table
gradient (the grid backward's atomics) is no part of this."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# B, out_c: one lane of one tile; a second tile with one row; the out_c > 4 path; many workgroups; 1 026 tiles on 1 024
# wavefronts (two wavefronts run a second tile: every image is overwritten while the tile loop goes on)
CASES = [(1, 3), (33, 1), (2048, 7), (4097, 3), (32 * 1024 + 33, 3)]
BIG = 32 * 1024 + 33


def _inputs(B, out_c):
    from enerf_amd.fused_mlp import pad32
    from enerf_amd.network import NeRFNetwork
    from enerf_amd import fused_network as fn
    torch.manual_seed(1000 * out_c + B)
    m = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=out_c).to(DEV)
    weights = [p.detach().contiguous() for p in fn.network_params(m)[1:]]
    Bp = pad32(B)
    feats = torch.zeros(16, Bp, 2, device=DEV)
    feats[:, :B] = torch.rand(16, B, 2, device=DEV) * 2 - 1
    dirs = torch.nn.functional.normalize(torch.randn(B, 3, device=DEV), dim=-1).contiguous()
    g_rgb = torch.randn(B, out_c, device=DEV)
    g_sigma = torch.randn(B, device=DEV)
    return weights, feats, dirs, g_rgb, g_sigma


def _run(mode, B, out_c, inputs, valid=None):
    """-> (dfeat [16, Bp, 2], [dws0, dws1, dwc0, dwc1, dwc2]) of one forward + backward under transpose `mode`."""
    from enerf_amd import _lib as L, fused_network as fn
    lib, s = L.lib(), L.stream_handle()
    weights, feats, dirs, g_rgb, g_sigma = inputs
    seg_s, seg_c = fn._weight_segments("linear", weights)
    sigma = torch.empty(B, device=DEV)
    rgb = torch.zeros(B, out_c, device=DEV)
    dfeat = torch.empty_like(feats)
    dws = [torch.empty_like(w) for w in weights]
    dseg_s = (ctypes.c_void_p * 4)(dws[0].data_ptr(), None, None, dws[1].data_ptr())
    dseg_c = (ctypes.c_void_p * 4)(dws[2].data_ptr(), dws[3].data_ptr(), None, dws[4].data_ptr())
    prev_prec = lib.enerf_mlp32_precision(1)
    prev = lib.enerf_debug_nerf_bwd_transpose(mode)
    if valid is not None:
        lib.enerf_mlp32_valid_rows(valid.data_ptr())
    try:
        assert lib.enerf_debug_nerf_bwd_transpose(-1) == mode
        L.check(lib.enerf_nerf_mlp_forward(feats.data_ptr(), dirs.data_ptr(), seg_s, seg_c, 31, B, out_c, sigma.data_ptr(),
                                           rgb.data_ptr(), 0, s), "nerf_mlp_forward")
        L.check(lib.enerf_nerf_mlp_backward(g_rgb.data_ptr(), g_sigma.data_ptr(), 1.0, feats.data_ptr(), dirs.data_ptr(),
                                            rgb.data_ptr(), seg_s, seg_c, dseg_s, dseg_c, 31, 1, B, out_c,
                                            dfeat.data_ptr(), 1, s), "nerf_mlp_backward")
        torch.cuda.synchronize()
    finally:
        if valid is not None:
            lib.enerf_mlp32_valid_rows(None)
        lib.enerf_debug_nerf_bwd_transpose(prev)
        lib.enerf_mlp32_precision(prev_prec)
    return dfeat, dws


_NAMES = ("dwseg_s[0]", "dwseg_s[3]", "dwseg_c[0]", "dwseg_c[1]", "dwseg_c[3]")


def _same(a, b, rows=None):
    fa, fb = (a[0], b[0]) if rows is None else (a[0][:, :rows], b[0][:, :rows])
    assert torch.equal(fa, fb), ("dfeat", int((fa != fb).sum()))
    for x, y, what in zip(a[1], b[1], _NAMES):
        assert torch.equal(x, y), (what, int((x != y).sum()), float((x - y).abs().max()))
    assert all(bool(torch.isfinite(x).all()) for x in a[1]) and float(a[1][3].abs().max()) > 0


def test_the_setting_defaults_to_lds_and_returns_the_previous_value():
    from enerf_amd import _lib as L
    lib = L.lib()
    assert lib.enerf_debug_nerf_bwd_transpose(-1) == 1
    assert lib.enerf_debug_nerf_bwd_transpose(0) == 1
    assert lib.enerf_debug_nerf_bwd_transpose(-1) == 0
    assert lib.enerf_debug_nerf_bwd_transpose(1) == 0
    assert lib.enerf_debug_nerf_bwd_transpose(-1) == 1


@pytest.mark.parametrize("B,out_c", CASES)
def test_lds_transposes_give_the_matrix_pipe_gradients(B, out_c):
    inputs = _inputs(B, out_c)
    _same(_run(1, B, out_c, inputs), _run(0, B, out_c, inputs))


@pytest.mark.parametrize("B", [4097, BIG])
def test_lds_transposes_give_the_matrix_pipe_gradients_with_pad_tiles(B):
    """enerf_mlp32_valid_rows = B - 700: pad tiles and the wave-uniform skip between two uses of an image."""
    inputs = _inputs(B, 3)
    real = B - 700
    inputs[3][real:] = 0
    inputs[4][real:] = 0
    cnt = torch.tensor([real, 0], dtype=torch.int32, device=DEV)
    _same(_run(1, B, 3, inputs, valid=cnt), _run(0, B, 3, inputs, valid=cnt), rows=real)


def test_lds_transposes_are_bit_stable_from_run_to_run():
    inputs = _inputs(BIG, 3)
    first = _run(1, BIG, 3, inputs)
    for it in range(20):
        again = _run(1, BIG, 3, inputs)
        assert torch.equal(again[0], first[0]), (it, "dfeat")
        for x, y, what in zip(again[1], first[1], _NAMES):
            assert torch.equal(x, y), (it, what)
