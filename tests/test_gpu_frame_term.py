"""The compositing launch with the frame tail (enerf_composite_rays_train_fwd_bwd_frames_c, csrc/raymarching.hip) through
enerf_amd.backends._raymarching: held bit for bit to the MSE form where the two state the same thing, to torch's alpha mix bit
for bit, and to fp64 for what only this entry computes (the per-ray error, the weighted loss).

Rays: test_gpu_composite_channels' case (sample counts 0, 1, 2, 63, 64, 65, 128, 200 and a ninth, dropped ray; M = 640, 523
used) and a second one of 37 rays -- two full workgroups of 16 and a partial one -- with permuted ids, empty rays among them
and 100 unowned rows behind the last sample.  Every output buffer starts as NaN, so a row nobody wrote is seen."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_composite_channels import BGS, DEV, _bg, _case, _rb

pytestmark = pytest.mark.gpu
CASES = ["nine", "thirty_seven"]
W03 = float(np.float32(0.3))                     # the weight as the C ABI's float carries it


def _case37(C, seed=5):
    g = torch.Generator(device=DEV).manual_seed(seed)
    N = 37
    counts = [(7 * i) % 70 for i in range(N)]                # 0 (rays 0, 10, 20, 30), 7 .. 69: one or two 64-lane chunks
    used = sum(counts)
    M = used + 100
    offs = [sum(counts[:i]) for i in range(N)]
    index = torch.randperm(N, generator=g, device=DEV).to(torch.int32)
    rays = torch.stack([index, torch.tensor(offs, dtype=torch.int32, device=DEV),
                        torch.tensor(counts, dtype=torch.int32, device=DEV)], 1).contiguous()
    rnd = lambda *s: torch.rand(*s, generator=g, device=DEV)
    return dict(C=C, N=N, M=M, used=used, rays=rays, sigmas=rnd(M) * 20 + 0.01, deltas=rnd(M, 2) * 0.02 + 1e-3,
                rgbs=rnd(M, C), counter=torch.tensor([used, N], dtype=torch.int32, device=DEV), bg_shared=rnd(C),
                bg_ray=rnd(N, C))


def _nan(*s):
    return torch.full(s, float("nan"), dtype=torch.float32, device=DEV)


def _frames(k, bg, pixels, weight, loss0=0.0):
    N, M, C = k["N"], k["M"], k["C"]
    r = dict(ws=_nan(N), image=_nan(N, C), out=_nan(N, C), gs=_nan(M), gr=_nan(M, C), gt=_nan(N, C), err=_nan(N),
             loss=torch.full((), loss0, dtype=torch.float32, device=DEV))
    _rb().composite_rays_train_fwd_bwd_frames(k["sigmas"], k["rgbs"], k["deltas"], k["rays"], M, N, r["ws"], r["image"], bg,
                                              r["out"], pixels, weight, k["counter"], r["gs"], r["gr"], r["gt"], r["err"],
                                              r["loss"])
    return r


def _mse(k, bg, target):
    N, M, C = k["N"], k["M"], k["C"]
    r = dict(ws=_nan(N), image=_nan(N, C), out=_nan(N, C), gs=_nan(M), gr=_nan(M, C))
    _rb().composite_rays_train_fwd_bwd_mse(k["sigmas"], k["rgbs"], k["deltas"], k["rays"], M, N, r["ws"], r["image"], bg,
                                           r["out"], target.contiguous(), 2.0 / (C * N), k["counter"], r["gs"], r["gr"])
    return r


@functools.lru_cache(maxsize=None)
def _runs(C, form, case):
    """Every launch the tests below look at, made once per (C, background form, case) and left unchanged."""
    k = _case(C) if case == "nine" else _case37(C)
    bg = _bg(k, form)
    g = torch.Generator(device=DEV).manual_seed(23)
    pixels = torch.rand(k["N"], C, generator=g, device=DEV)
    with_alpha = torch.cat([pixels, torch.rand(k["N"], 1, generator=g, device=DEV)], 1).contiguous()
    plain = _frames(k, bg, pixels, 1.0)
    alpha = _frames(k, bg, with_alpha, 1.0)
    return dict(k=k, bg=bg, pixels=pixels, with_alpha=with_alpha, plain=plain, alpha=alpha,
                mse_plain=_mse(k, bg, pixels), mse_alpha=_mse(k, bg, alpha["gt"]),
                preset=_frames(k, bg, pixels, 1.0, loss0=0.25), weighted=_frames(k, bg, pixels, W03))


def _same_as_mse(r, m, k):
    for name in ("ws", "image", "out", "gs", "gr"):
        assert torch.isfinite(r[name]).all(), name
        assert torch.equal(r[name], m[name]), name
    assert float(r["gs"][k["used"]:].abs().max()) == 0 and float(r["gr"][k["used"]:].abs().max()) == 0
    assert float(r["gs"][:k["used"]].abs().max()) > 0 and float(r["gr"][:k["used"]].abs().max()) > 0


params = lambda f: pytest.mark.parametrize("case", CASES)(pytest.mark.parametrize("form", BGS)(
    pytest.mark.parametrize("C", [1, 2, 3])(f)))


@params
def test_finished_pixels_at_weight_one_equal_the_mse_entry(C, form, case):
    """pix_stride == C, weight = 1: what the MSE entry also has, bit for bit; the ground truth is the pixels."""
    s = _runs(C, form, case)
    _same_as_mse(s["plain"], s["mse_plain"], s["k"])
    assert torch.equal(s["plain"]["gt"], s["pixels"])


@params
def test_alpha_pixels_are_mixed_as_torch_mixes_them(C, form, case):
    """pix_stride == C + 1: gt_out is torch's p * a + bg * (1 - a) bit for bit; the rest is the MSE entry fed that gt."""
    s = _runs(C, form, case)
    p, a = s["with_alpha"][:, :C], s["with_alpha"][:, C:]
    bg = s["bg"]
    assert torch.equal(s["alpha"]["gt"], p * a + bg * (1 - a))
    assert not torch.equal(s["alpha"]["gt"], p)
    _same_as_mse(s["alpha"], s["mse_alpha"], s["k"])


@params
def test_per_ray_error_against_fp64(C, form, case):
    """rtol 1e-6: at most five fp32 roundings (the difference, its square, two additions, the division) of non-negative
    terms, 5 * 2^-24 = 3e-7.  Missed and dropped rays carry (bg - gt)^2: their out_image is the background."""
    s = _runs(C, form, case)
    k = s["k"]
    for r in (s["plain"], s["alpha"]):
        want = ((r["out"].double() - r["gt"].double()) ** 2).sum(-1) / C
        assert torch.isfinite(r["err"]).all() and float(want.min()) > 0
        rel = float(((r["err"].double() - want).abs() / want).max())
        print(f"C={C} {form} {case}: err max rel = {rel:.2e}")
        assert rel <= 1e-6
    counts, offs, ids = k["rays"][:, 2], k["rays"][:, 1], k["rays"][:, 0].long()
    unmarched = ids[(counts == 0) | (offs + counts >= k["M"])]
    assert unmarched.numel() >= (2 if case == "nine" else 4)
    bgt = s["bg"] if isinstance(s["bg"], torch.Tensor) else torch.tensor(s["bg"], device=DEV)
    bg_rows = bgt.expand(k["N"], C) if bgt.dim() < 2 else bgt
    assert torch.equal(s["alpha"]["out"][unmarched], bg_rows[unmarched])
    assert float(s["alpha"]["ws"][unmarched].abs().max()) == 0


@params
def test_loss_is_the_weighted_mean_error_added_into_its_slot(C, form, case):
    """rtol N * 2^-24 * 4 against the fp64 sum (the worst case of accumulating N terms in fp32, each itself a few
    roundings).  A pre-set 0.25 stays: the difference to the zero-started value is the rounding of the additions into a
    value below 1 -- one per workgroup, 2^-24 each, and as much again for the subtraction here."""
    s = _runs(C, form, case)
    N = s["k"]["N"]
    for r in (s["plain"], s["alpha"]):
        want = float((((r["out"].double() - r["gt"].double()) ** 2).sum(-1) / C).sum() / N)
        got = float(r["loss"])
        print(f"C={C} {form} {case}: loss rel = {abs(got - want) / want:.2e}")
        assert abs(got - want) <= N * 2.0 ** -24 * 4 * want
    groups = (N + 15) // 16
    assert abs((float(s["preset"]["loss"]) - 0.25) - float(s["plain"]["loss"])) <= 2 * groups * 2.0 ** -24


def _ulps(got, ref64):
    """|got - ref| in units of the fp32 spacing at ref."""
    ref32 = ref64.float().abs()
    ulp = (torch.nextafter(ref32, torch.full_like(ref32, float("inf"))) - ref32).double()
    return ((got.double() - ref64).abs() / ulp).max()


@params
def test_weight_scales_the_gradients_and_the_loss_and_not_the_error(C, form, case):
    """weight = 0.3 against weight = 1: gradients 0.3 x to 2 ulp, loss 0.3 x (to the accumulation bound of the loss test: the
    workgroups' atomics land in any order), err_out and every image unchanged."""
    s = _runs(C, form, case)
    one, w = s["plain"], s["weighted"]
    for name in ("ws", "image", "out", "gt", "err"):
        assert torch.equal(w[name], one[name]), name
    used = s["k"]["used"]
    for name in ("gs", "gr"):
        assert torch.isfinite(w[name]).all()
        assert float(w[name][used:].abs().max()) == 0
        u = float(_ulps(w[name][:used], W03 * one[name][:used].double()))
        print(f"C={C} {form} {case}: {name} max ulp = {u:.2f}")
        assert u <= 2.0, name
    N = s["k"]["N"]
    assert abs(float(w["loss"]) - W03 * float(one["loss"])) <= N * 2.0 ** -24 * 4 * W03 * float(one["loss"])


@pytest.mark.parametrize("C", [1, 3])
def test_bad_pixel_stride_and_missing_counter_are_bad_arguments(C):
    from enerf_amd import _lib as L
    k = _case(C)
    N, M = k["N"], k["M"]

    def call(pixels, counter):
        _rb().composite_rays_train_fwd_bwd_frames(k["sigmas"], k["rgbs"], k["deltas"], k["rays"], M, N, _nan(N), _nan(N, C),
                                                  0.3, _nan(N, C), pixels, 1.0, counter, _nan(M), _nan(M, C))
    for width in (C - 1, C + 2):
        if width:
            with pytest.raises(RuntimeError, match=r"code -1\): .*pix_stride"):
                call(torch.rand(N, width, device=DEV), k["counter"])
    with pytest.raises(RuntimeError, match=r"code -1\): .*counter"):
        call(torch.rand(N, C, device=DEV), None)
    assert L.lib().enerf_last_error()
    call(torch.rand(N, C, device=DEV), k["counter"])             # and the well-formed call goes through
