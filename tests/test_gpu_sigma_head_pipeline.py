"""The density-only head's load pipeline (csrc/mlp32s.hip: k_mlp32s_fwd with D > 0) against the form shipped before it
(enerf_debug_sigma_head(0): one tile ahead, 512 workgroups).  The per-tile arithmetic is the same
instruction sequence, so sigma must be the same bits; what can go wrong is the bookkeeping around it -- which register set
serves which tile, the requests sent before the weights are staged, the rest of a wavefront's tiles after its full-speed
trips, the rows past the batch.

Shapes.  With the forward grid capped at 1 / 2 workgroups (enerf_debug_mlp32_grid_caps) a launch is 4 / 8 wavefronts, and a
batch of T tiles gives wavefront w its tiles w, w + 4 (8), ...: the row counts below make wavefronts of 0 to 7 tiles, which
covers 0, 1, 2, D, D + 1 and 2 D + 1 for every depth D <= 3 (the default is 2), with last tiles of 1, 5, 17, 31 and 32 live
rows.  The features carry NaN in their pad rows and sigma a sentinel behind its last row.  Arithmetic modes: split-bf16 (1,
the default), bf16 and fp16 operands (2, 3: the same kernel on one product), and exact fp32 (0), whose head is bound by
its fp32 MFMAs and keeps the old kernel under either selector value -- the comparison holds there all the same.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -777.0
U = 2.0 ** -16                        # one split-bf16 product (tests/nerf_mlp_ref.py)

# (forward-grid cap, rows): tiles per wavefront in the comment
CAPPED = [(1, 1), (1, 31), (1, 32), (1, 33),          # 1 0 0 0 / 1 1 0 0
          (1, 32 * 5 + 5),                            # T = 6:  2 2 1 1
          (1, 32 * 12 + 5),                           # T = 13: 4 3 3 3
          (1, 32 * 17 + 32),                          # T = 18: 5 5 4 4
          (1, 32 * 20 + 5),                           # T = 21: 6 5 5 5
          (1, 32 * 26 + 17),                          # T = 27: 7 7 7 6
          (2, 32 * 8 + 5),                            # T = 9:  2 1 1 1 1 1 1 1
          (2, 32 * 18 + 5),                           # T = 19: 3 3 3 2 2 2 2 2
          (2, 32 * 36 + 5),                           # T = 37: 5 5 5 5 5 4 4 4
          (2, 32 * 49 + 31)]                          # T = 50: 7 7 6 6 6 6 6 6


def _lib():
    from enerf_amd import _lib as L
    return L


def _problem(B, seed):
    """-> (level-major features [16, Bp, 2] with NaN pad rows, weight blob [W0 64x32 | Wout 16x64])."""
    g = torch.Generator().manual_seed(seed)
    Bp = (B + 31) // 32 * 32
    feats = torch.rand(16, Bp, 2, generator=g) * 2 - 1
    feats[:, B:, :] = float("nan")
    w0 = (torch.rand(64, 32, generator=g) * 2 - 1) / 32 ** 0.5
    wo = (torch.rand(16, 64, generator=g) * 2 - 1) / 64 ** 0.5
    return feats.to(DEV).contiguous(), torch.cat([w0.reshape(-1), wo.reshape(-1)]).to(DEV).contiguous()


def _head(feats, blob, B):
    """sigma [B] of the current form and arithmetic; the 64 floats behind it must keep their sentinel."""
    L = _lib()
    out = torch.full((B + 64,), SENTINEL, device=DEV)
    L.check(L.lib().enerf_mlp32_forward(feats.data_ptr(), blob.data_ptr(), B, 32, 16, 1, 0, 6, None, None, 1, 0,
                                        out.data_ptr(), L.stream_handle()), "mlp32_forward(sigma only)")
    torch.cuda.synchronize()
    assert bool((out[B:] == SENTINEL).all())
    return out[:B].clone()


def _both_forms(feats, blob, B, precision):
    """-> (sigma of the form shipped before, sigma of the default form) in one arithmetic mode; the selector is restored."""
    lib = _lib().lib()
    prev_p = lib.enerf_mlp32_precision(precision)
    prev_f = lib.enerf_debug_sigma_head(-1)
    try:
        lib.enerf_debug_sigma_head(0)
        assert lib.enerf_debug_sigma_head(-1) == 0
        old = _head(feats, blob, B)
        lib.enerf_debug_sigma_head(1)
        assert lib.enerf_debug_sigma_head(-1) == 1
        new = _head(feats, blob, B)
    finally:
        lib.enerf_debug_sigma_head(prev_f)
        lib.enerf_mlp32_precision(prev_p)
    return old, new


def test_selector_round_trip():
    lib = _lib().lib()
    assert lib.enerf_debug_sigma_head(-1) == 1                  # the pipelined head is the default
    assert lib.enerf_debug_sigma_head(0) == 1
    assert lib.enerf_debug_sigma_head(7) == 0                   # not a form: ignored
    assert lib.enerf_debug_sigma_head(-1) == 0
    assert lib.enerf_debug_sigma_head(1) == 0
    assert lib.enerf_debug_sigma_head(-1) == 1


@pytest.mark.parametrize("cap,B", CAPPED, ids=[f"cap{c}-B{b}" for c, b in CAPPED])
def test_capped_grids_bit_identical_to_the_one_ahead_form(cap, B):
    lib = _lib().lib()
    feats, blob = _problem(B, 100 + B)
    lib.enerf_debug_mlp32_grid_caps(cap, 0)
    try:
        for precision in (1, 0, 2, 3):
            old, new = _both_forms(feats, blob, B, precision)
            assert bool(torch.isfinite(old).all()), precision
            assert torch.equal(new, old), (precision, int((new != old).sum()))
    finally:
        lib.enerf_debug_mlp32_grid_caps(0, 0)


def test_uncapped_grid_bit_identical_and_within_the_fp64_bar():
    """3 x 32 x (resident wavefronts) + 7 rows on the default grid: three rounds of every wavefront and a ragged fourth
    for one.  Both forms against each other (torch.equal) and against an fp64 evaluation of the net at the bar of the fp64
    MLP tests (tests/nerf_mlp_ref.py): |sigma - sigma_fp64| <= (1e-4 + 3 u H0^) sigma_fp64, H0^ the magnitudes carried
    through the two products with the reference's own ReLU mask, u = 2^-16."""
    waves = 8 * torch.cuda.get_device_properties(0).multi_processor_count       # two per SIMD, four SIMDs per CU
    B = 3 * 32 * waves + 7
    feats, blob = _problem(B, 7)
    X = feats[:, :B, :].permute(1, 0, 2).reshape(B, 32).double()
    w0, wo0 = blob[:64 * 32].view(64, 32).double(), blob[64 * 32:64 * 32 + 64].double()
    pre = X @ w0.t()
    ref = torch.exp(torch.relu(pre) @ wo0)
    H0 = ((X.abs() @ w0.abs().t()) * (pre > 0)) @ wo0.abs()
    bar = (1e-4 + 3 * U * H0) * ref
    for precision in (1, 0):
        old, new = _both_forms(feats, blob, B, precision)
        assert torch.equal(new, old), (precision, int((new != old).sum()))
        worst = float(((new.double() - ref).abs() / bar).max())
        print(f"precision {precision}: worst |sigma - fp64| / bar = {worst:.3f}")
        assert worst <= 1.0, precision


def test_full_sweep_update_is_bit_equal_between_the_forms():
    """One update_extra_state full sweep (grid_size 32, one cascade): density grid, bitfield and mean_density."""
    from enerf_amd.network import NeRFNetwork

    class Small(NeRFNetwork):
        grid_size = 32

    lib = _lib().lib()
    prev = lib.enerf_debug_sigma_head(-1)
    res = []
    try:
        for form in (0, 1):
            torch.manual_seed(3)
            m = Small(encoding="hashgrid", bound=1, cuda_ray=True, out_dim_color=3).to(DEV)
            m.encoder.embeddings.data.uniform_(-1.0, 1.0)
            m.train()
            assert m.cascade == 1 and m.iter_density == 0
            lib.enerf_debug_sigma_head(form)
            m.update_extra_state()
            torch.cuda.synchronize()
            res.append((m.density_grid.clone(), m.density_bitfield.clone(), m.mean_density))
    finally:
        lib.enerf_debug_sigma_head(prev)
    (g0, b0, m0), (g1, b1, m1) = res
    assert float(g0.max()) > 0.0
    assert torch.equal(g1, g0) and torch.equal(b1, b0) and m1 == m0
