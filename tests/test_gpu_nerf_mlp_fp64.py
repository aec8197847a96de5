"""k_nerf_fwd / k_nerf_bwd (csrc/nerf_mlp.hip: the sigma net and the colour net as one launch per direction) against the fp64
reference and the per-entry error model of tests/nerf_mlp_ref.py.  The entry points are called directly
(enerf_nerf_mlp_forward with flags 0, enerf_nerf_mlp_backward with flags 1); the reference runs on the device.  No row of
a batch is a knife-edge sample (nerf_mlp_ref.make_batch), so the strict bars hold for every entry of every output.

Cases (default-initialised weights, out_c 3, w0_cols_c 31, overwrite 1, sigma_scale 1, LDS transposes unless stated):
  A  shapes: B in {1, 31, 32, 33, 4097}; B = 289 and 32 * 37 + 5 on ONE workgroup (enerf_debug_mlp32_grid_caps(1, 1): its four
     wavefronts take three / ten rounds of the tile loop, the last one ragged); B = 289 on the matrix-pipe transposes
  B  out_c in {1, 4, 5, 16} at B = 321
  C  w0_cols_c = 32: NaN in wc0's pad column, a sentinel in the gradient's
  D  |h0| up to 29 (row 0 of ws1 scaled: trunc_exp's clamp decides > 2 % of the rows on either side), sigma_scale 0.25
  E  overwrite = 0 onto random gradient buffers
  F  enerf_mlp32_valid_rows(_ex): padding rows, NaN in every wholly skipped tile
  G  the operand fragments are rebuilt for weights changed in place

Worst err / bar per output, measured on an MI355X (pytest -s):
  case                                sigma    rgb     dX   dws0   dws1   dwc0   dwc1   dwc2
  A B1                                0.006  0.002  0.003  0.027  0.032  0.041  0.008  0.001
  A B31                               0.008  0.007  0.019  0.026  0.010  0.020  0.019  0.001
  A B32                               0.008  0.008  0.021  0.032  0.018  0.027  0.031  0.001
  A B33                               0.009  0.006  0.022  0.020  0.009  0.021  0.012  0.001
  A B4097                             0.013  0.010  0.036  0.002  0.001  0.001  0.003  0.000
  A B289-one-workgroup                0.008  0.009  0.023  0.009  0.005  0.007  0.003  0.000
  A B1189-one-workgroup               0.011  0.010  0.039  0.005  0.002  0.004  0.002  0.000
  A B289-one-workgroup-matrix-pipe    0.012  0.010  0.040  0.007  0.004  0.006  0.005  0.000
  B out_c1                            0.009  0.007  0.048  0.015  0.004  0.012  0.007  0.000
  B out_c4                            0.014  0.011  0.029  0.008  0.005  0.005  0.004  0.000
  B out_c5                            0.009  0.010  0.020  0.007  0.004  0.003  0.002  0.001
  B out_c16                           0.009  0.009  0.009  0.002  0.003  0.003  0.002  0.000
  C padded                            0.013  0.007  0.025  0.007  0.005  0.005  0.002  0.000
  D large-h0                          0.020  0.008  0.815  0.162  0.020  0.004  0.003  0.000
  E accumulate                        0.011  0.008  0.029  0.007  0.003  0.005  0.004  0.000
  F count0                            no real row: every gradient exactly zero
  F count1                            0.005  0.001  0.007  0.038  0.028  0.024  0.014  0.001
  F count32                           0.012  0.007  0.024  0.022  0.012  0.017  0.018  0.001
  F count3397                         0.016  0.010  0.038  0.003  0.001  0.002  0.001  0.000
  F count4102                         0.016  0.009  0.038  0.002  0.001  0.002  0.001  0.000
  F ex1500                            0.013  0.012  0.033  0.002  0.002  0.002  0.004  0.000
  F ex5000                            0.011  0.010  0.036  0.003  0.001  0.002  0.001  0.000
  G first weights                     0.009  0.008  0.028  0.009  0.004  0.005  0.003  0.000
  G second weights, same tensors      0.012  0.011  0.029  0.006  0.004  0.004  0.006  0.000
(D runs closest to its bars: the forward's own error in h0 reaches d h0 = g exp(h0) to first order, and |h0| is up to 29.)
"""
import ctypes

import pytest
import torch

import nerf_mlp_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -777.0


def _spec(B, seed, out_c=3, w0c=31, overwrite=1, scale=1.0, caps=None, transpose=1, large_h0=False):
    return dict(B=B, seed=seed, out_c=out_c, w0c=w0c, overwrite=overwrite, scale=scale, caps=caps, transpose=transpose,
                large_h0=large_h0)


SHAPES = {f"B{B}": _spec(B, seed) for B, seed in ((1, 15), (31, 11), (32, 12), (33, 13), (4097, 14))}
SHAPES["B289-one-workgroup"] = _spec(289, 20, caps=(1, 1))
SHAPES["B1189-one-workgroup"] = _spec(32 * 37 + 5, 21, caps=(1, 1))
SHAPES["B289-one-workgroup-matrix-pipe"] = _spec(289, 22, caps=(1, 1), transpose=0)
COLOURS = {f"out_c{c}": _spec(321, 30 + c, out_c=c) for c in (1, 4, 5, 16)}
PADDED = _spec(321, 50, w0c=32)
LARGE_H0 = _spec(321, 68, scale=0.25, large_h0=True)
ACCUMULATE = _spec(321, 70, overwrite=0)
# F: (count, base, cap) at B = 4097 -> real rows = min(base + min(count, cap), B)  (cap 0: min(count, B))
PAD_B = 4097
PAD_ROWS = {"count0": (0, 0, 0), "count1": (1, 0, 0), "count32": (32, 0, 0), "count3397": (3397, 0, 0),
            "count4102": (4102, 0, 0), "ex1500": (1500, 1024, 2048), "ex5000": (5000, 1024, 2048)}
PAD_SEEDS = {name: 90 + k for k, name in enumerate(PAD_ROWS)}
REBUILD = (_spec(321, 80), _spec(321, 81))


def _real_rows(count, base, cap):
    return min(base + min(count, cap), PAD_B) if cap else min(count, PAD_B)


def all_specs():
    """Every batch this module draws, as (name, spec): tests/test_nerf_mlp_ref.py draws them all on the host."""
    yield from SHAPES.items()
    yield from COLOURS.items()
    yield from (("padded", PADDED), ("large-h0", LARGE_H0), ("accumulate", ACCUMULATE))
    for name, v in PAD_ROWS.items():
        if _real_rows(*v):
            yield name, _spec(_real_rows(*v), PAD_SEEDS[name])
    yield from (("rebuild-0", REBUILD[0]), ("rebuild-1", REBUILD[1]))


def draw(spec):
    """-> (the five fp32 weights, the batch) on the host; wc0 with w0c columns (a pad column holds NaN)."""
    ws = R.default_weights(spec["out_c"], spec["seed"])
    inp = R.make_batch(spec["B"], ws, 1000 + spec["seed"])
    if spec["large_h0"]:
        R.scale_h0_row(ws, inp["X"])
    if spec["w0c"] == 32:
        ws[2] = torch.cat([ws[2], torch.full((64, 1), float("nan"))], dim=1).contiguous()
    return ws, inp


def _tensors(ws, X, d, g_rgb, g_sigma, out_c, dw_fill=None):
    """Device tensors of one call: inputs, outputs prefilled with sentinels (dfeat: NaN; dW: NaN, or `dw_fill`)."""
    B = X.shape[0]
    t = dict(ws=[w.to(DEV).contiguous() for w in ws], feats=R.to_level_major(X).to(DEV), dirs=d.to(DEV).contiguous(),
             g_rgb=g_rgb.to(DEV).contiguous(), g_sigma=g_sigma.to(DEV).contiguous(),
             sigma=torch.full((B,), SENTINEL, device=DEV), rgb=torch.full((B, out_c), SENTINEL, device=DEV))
    t["dfeat"] = torch.full_like(t["feats"], float("nan"))
    t["dws"] = [torch.full_like(w, float("nan")) if dw_fill is None else dw_fill[k].to(DEV).contiguous()
                for k, w in enumerate(t["ws"])]
    return t


def _launch(t, B, out_c, w0c=31, overwrite=1, scale=1.0, caps=None, transpose=1, valid=None):
    """One forward (flags 0) and one backward (flags 1) on the tensors `t`; every setting touched is restored.
    `valid`: (device int32 count, base, cap) for enerf_mlp32_valid_rows(_ex)."""
    from enerf_amd import _lib as L, fused_network as fn
    lib, s = L.lib(), L.stream_handle()
    seg_s, seg_c = fn._weight_segments("linear", t["ws"])
    dws = t["dws"]
    dseg_s = (ctypes.c_void_p * 4)(dws[0].data_ptr(), None, None, dws[1].data_ptr())
    dseg_c = (ctypes.c_void_p * 4)(dws[2].data_ptr(), dws[3].data_ptr(), None, dws[4].data_ptr())
    prev_prec = lib.enerf_mlp32_precision(1)
    prev_tr = lib.enerf_debug_nerf_bwd_transpose(transpose)
    try:
        if caps is not None:
            lib.enerf_debug_mlp32_grid_caps(*caps)
        if valid is not None:
            cnt, base, cap = valid
            if cap:
                lib.enerf_mlp32_valid_rows_ex(cnt.data_ptr(), base, cap)
            else:
                lib.enerf_mlp32_valid_rows(cnt.data_ptr())
        L.check(lib.enerf_nerf_mlp_forward(t["feats"].data_ptr(), t["dirs"].data_ptr(), seg_s, seg_c, w0c, B, out_c,
                                           t["sigma"].data_ptr(), t["rgb"].data_ptr(), 0, s), "nerf_mlp_forward")
        L.check(lib.enerf_nerf_mlp_backward(t["g_rgb"].data_ptr(), t["g_sigma"].data_ptr(), float(scale),
                                            t["feats"].data_ptr(), t["dirs"].data_ptr(), t["rgb"].data_ptr(), seg_s, seg_c,
                                            dseg_s, dseg_c, w0c, overwrite, B, out_c, t["dfeat"].data_ptr(), 1, s),
                "nerf_mlp_backward")
        torch.cuda.synchronize()
    finally:
        lib.enerf_mlp32_valid_rows(None)
        lib.enerf_debug_mlp32_grid_caps(0, 0)
        lib.enerf_debug_nerf_bwd_transpose(prev_tr)
        lib.enerf_mlp32_precision(prev_prec)


def _reference(t, B, scale=1.0):
    """fp64 on the device, from the very tensors the kernels read (their first B rows)."""
    return R.reference(R.from_level_major(t["feats"], B), t["dirs"][:B], t["ws"], t["g_rgb"][:B], t["g_sigma"][:B], scale)


def _got(t, B):
    got = dict(sigma=t["sigma"][:B], rgb=t["rgb"][:B], dX=R.from_level_major(t["dfeat"], B))
    got.update({k: (v[:, :31] if k == "dwc0" else v) for k, v in zip(R.DW_NAMES, t["dws"])})
    return got


def _run_spec(name, spec):
    ws, inp = draw(spec)
    B, out_c = spec["B"], spec["out_c"]
    t = _tensors(ws, inp["X"], inp["d"], inp["g_rgb"], inp["g_sigma"], out_c)
    _launch(t, B, out_c, spec["w0c"], spec["overwrite"], spec["scale"], spec["caps"], spec["transpose"])
    ref = _reference(t, B, spec["scale"])
    R.check(ref, _got(t, B), name)
    assert bool((t["dfeat"][:, B:] == 0).all())          # the rows that pad the batch to a tile: written as zeros
    return t, ref


@pytest.mark.parametrize("name", list(SHAPES))
def test_a_shapes(name):
    _run_spec("A " + name, SHAPES[name])


@pytest.mark.parametrize("name", list(COLOURS))
def test_b_colour_outputs(name):
    _run_spec("B " + name, COLOURS[name])


def test_c_padded_first_layer_of_the_colour_net():
    ws, inp = draw(PADDED)
    B = PADDED["B"]
    assert ws[2].shape == (64, 32) and bool(torch.isnan(ws[2][:, 31]).all())
    fill = [torch.full_like(w, SENTINEL) for w in ws]
    t = _tensors(ws, inp["X"], inp["d"], inp["g_rgb"], inp["g_sigma"], 3, dw_fill=fill)
    _launch(t, B, 3, w0c=32)
    R.check(_reference(t, B), _got(t, B), "C padded")
    assert bool((t["dws"][2][:, 31] == SENTINEL).all())   # the pad column: neither read (NaN) nor written


def test_d_large_h0_with_sigma_scale():
    t, ref = _run_spec("D large-h0", LARGE_H0)
    R.assert_large_h0(ref)


def test_e_accumulation():
    ws, inp = draw(ACCUMULATE)
    B = ACCUMULATE["B"]
    g = torch.Generator().manual_seed(7)
    base = [torch.randn(w.shape, generator=g) for w in ws]
    t = _tensors(ws, inp["X"], inp["d"], inp["g_rgb"], inp["g_sigma"], 3, dw_fill=base)
    _launch(t, B, 3, overwrite=0)
    R.check(_reference(t, B), _got(t, B), "E accumulate", base={k: b.to(DEV) for k, b in zip(R.DW_NAMES, base)})


@pytest.mark.parametrize("name", list(PAD_ROWS))
def test_f_padding_rows(name):
    count, base, cap = PAD_ROWS[name]
    B, real = PAD_B, _real_rows(count, base, cap)
    kept = (real + 31) // 32 * 32                        # rows from here on sit in tiles that are skipped whole
    ws = R.default_weights(3, PAD_SEEDS[name])
    g = torch.Generator().manual_seed(count + 5)
    # rows from the real count to the end of its tile: finite inputs, zero output gradients (they are computed);
    # rows of wholly skipped tiles: NaN in every input
    X = torch.rand(B, 32, generator=g) * 2 - 1
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1)
    g_rgb, g_sigma = torch.zeros(B, 3), torch.zeros(B)
    if real:
        inp = R.make_batch(real, ws, 1000 + PAD_SEEDS[name])
        for dst, k in ((X, "X"), (d, "d"), (g_rgb, "g_rgb"), (g_sigma, "g_sigma")):
            dst[:real] = inp[k]
    for dst in (X, d, g_rgb, g_sigma):
        dst[kept:] = float("nan")
    t = _tensors(ws, X, d, g_rgb, g_sigma, 3)
    cnt = torch.tensor([count, 0], dtype=torch.int32, device=DEV)
    _launch(t, B, 3, valid=(cnt, base, cap))
    for k, v in zip(R.DW_NAMES, t["dws"]):
        assert bool(torch.isfinite(v).all()), k
    assert bool((t["dfeat"][:, real:] == 0).all())
    assert bool((t["sigma"][kept:] == SENTINEL).all()) and bool((t["rgb"][kept:] == SENTINEL).all())
    if real == 0:
        assert all(bool((v == 0).all()) for v in t["dws"])
        print(f"err / bar [F {name}]: no real row, every gradient exactly zero")
        return
    ref = _reference(t, real)
    got = _got(t, B)
    got.update(sigma=got["sigma"][:real], rgb=got["rgb"][:real], dX=got["dX"][:real])
    R.check(ref, got, f"F {name}, {real} real rows")


def test_g_fragments_are_rebuilt_for_weights_changed_in_place():
    first, second = REBUILD
    B = first["B"]
    ws, inp = draw(first)
    t = _tensors(ws, inp["X"], inp["d"], inp["g_rgb"], inp["g_sigma"], 3)
    _launch(t, B, 3)
    R.check(_reference(t, B), _got(t, B), "G first weights")
    ws2, inp2 = draw(second)
    for w, w2 in zip(t["ws"], ws2):
        assert not torch.equal(w.cpu(), w2)
        w.copy_(w2)
    t["feats"].copy_(R.to_level_major(inp2["X"]))
    for k, src in (("dirs", "d"), ("g_rgb", "g_rgb"), ("g_sigma", "g_sigma")):
        t[k].copy_(inp2[src])
    _launch(t, B, 3)
    R.check(_reference(t, B), _got(t, B), "G second weights, same tensors")
