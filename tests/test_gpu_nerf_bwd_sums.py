"""k_nerf_bwd (csrc/nerf_mlp.hip), its set-up and its per-workgroup sums.  The default form (LDS transposes,
enerf_debug_nerf_bwd_transpose(1)) issues every global load of the set-up -- the valid-row count, the first tile's inputs,
the 40 operand fragments -- before its first wait and consumes the count only after the set-up barrier; its four waves
then store their weight-gradient accumulators into a region each and one pass writes (w0 + w2) + (w1 + w3).  The
matrix-pipe form (0) has no room for four regions and keeps the two-phase sums (waves 2 / 3 add into the regions of
waves 0 / 1): the same association, so the feature gradient and the five weight gradients must be equal under
torch.equal.  The entry points are called directly, at precision 1, as in test_gpu_nerf_bwd_transpose.py."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# B, out_c: 255 of the 256 workgroups flush nothing but zeros; a second tile with one row and one colour row; out_c = 16
# (the entry point accepts 1..16): every row of the colour output layer's sums is live and the four regions fill the
# 160 KiB of LDS to the last word; many workgroups; 1 026 tiles on 1 024 wavefronts (two run a second tile)
BIG = 32 * 1024 + 33
CASES = [(1, 3), (33, 1), (2048, 16), (4097, 3), (BIG, 3)]
_NAMES = ("dwseg_s[0]", "dwseg_s[3]", "dwseg_c[0]", "dwseg_c[1]", "dwseg_c[3]")


def _inputs(B, out_c):
    from enerf_amd.fused_mlp import pad32
    from enerf_amd.network import NeRFNetwork
    from enerf_amd import fused_network as fn
    torch.manual_seed(7000 * out_c + B)
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


def _same(a, b, rows=None):
    fa, fb = (a[0], b[0]) if rows is None else (a[0][:, :rows], b[0][:, :rows])
    assert torch.equal(fa, fb), ("dfeat", int((fa != fb).sum()))
    for x, y, what in zip(a[1], b[1], _NAMES):
        assert x.shape == y.shape and torch.equal(x, y), (what, int((x != y).sum()), float((x - y).abs().max()))
    assert all(bool(torch.isfinite(x).all()) for x in a[1]) and float(a[1][3].abs().max()) > 0


@pytest.mark.parametrize("B,out_c", CASES)
def test_four_region_sums_give_the_two_phase_sums(B, out_c):
    inputs = _inputs(B, out_c)
    _same(_run(1, B, out_c, inputs), _run(0, B, out_c, inputs))


def test_the_row_count_read_after_the_set_up_skips_the_same_tiles():
    """enerf_mlp32_valid_rows = B - 700: the count bounds the tile loop and the wave-uniform skips, and the new set-up
    consumes it only after its barrier.  Rows past the count get zero feature gradients and add nothing to the sums."""
    B = 4097
    inputs = _inputs(B, 3)
    real = B - 700
    inputs[3][real:] = 0
    inputs[4][real:] = 0
    cnt = torch.tensor([real, 0], dtype=torch.int32, device=DEV)
    new, old = _run(1, B, 3, inputs, valid=cnt), _run(0, B, 3, inputs, valid=cnt)
    _same(new, old, rows=real)
    first_pad = (real + 31) // 32 * 32                   # the first row of the first skipped tile
    assert float(new[0][:, first_pad:].abs().max()) == 0.0 and float(old[0][:, first_pad:].abs().max()) == 0.0


def test_the_sums_are_bit_stable_from_run_to_run():
    inputs = _inputs(BIG, 3)
    first = _run(1, BIG, 3, inputs)
    for it in range(2):
        again = _run(1, BIG, 3, inputs)
        assert torch.equal(again[0], first[0]), (it, "dfeat")
        for x, y, what in zip(again[1], first[1], _NAMES):
            assert torch.equal(x, y), (it, what)
