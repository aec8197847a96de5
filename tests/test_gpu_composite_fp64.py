"""The marching route's compositing kernels (csrc/raymarching.hip: k_composite_train_fwd, k_composite_train_bwd<MSE>,
k_composite_train_fwd_bwd_mse<C, MseTail | FrameTail>, k_composite_rays, k_composite_rays_frame) through
enerf_amd.backends._raymarching, against the fp64 reference and the a-priori bars of tests/composite_ref.py (the error
model is derived in that module's docstring; tests/test_composite_ref.py holds the C oracle and a numpy statement of the
scan order to the same bars and shows that they reject ten seeded defects).

Sixteen cases: N = 1, 3, 4, 5, 15, 16, 17, 33 rays twice over (partial workgroups at 4 and at 16 rays), C = 1, 2, 3, the
background a scalar, shared or per ray, every family (RAND, THIN, WALL, SAT_LATE, ZERO, ONE_HOT) at every sample count
1, 2, 15 .. 17, 31 .. 33, 47 .. 49, 63 .. 65, 127 .. 129, 200, 1023, 1024, plus empty and dropped rays; the largest
case has under 6000 samples.  Every output buffer starts as NaN: a row a kernel must not touch stays NaN, a row it must
zero or write shows up if it did not.  Each test prints its worst error / bar per output (and per family).

The loss values are held to 4 N u relative against the fp64 sum over the written out_image (the accumulation of N terms of
a few roundings each), plus one rounding of the preset-plus-loss value per workgroup's atomic addition.  The per-ray error
of the frame tail: the difference, its square, C - 1 additions and the division, (C + 3) u relative."""
import functools

import numpy as np
import pytest
import torch

import composite_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = R.U
ALL = list(range(R.N_CASES))
PRESET = 0.25


def _rb():
    from enerf_amd.backends import _raymarching
    return _raymarching


def _dev(a):
    return torch.tensor(np.asarray(a), device=DEV)


def _nan(*s):
    return torch.full(s, float("nan"), dtype=torch.float32, device=DEV)


@functools.lru_cache(maxsize=None)
def _inputs(i):
    c = R.make_case(i)
    d = {k: _dev(c[k]) for k in ("sigmas", "rgbs", "deltas", "rays", "target", "g_image", "g_ws")}
    d["bg"] = c["bg"] if c["form"] == "scalar" else _dev(c["bg"])
    d["pixels_alpha"] = _dev(c["pixels"])
    d["pixels"] = _dev(np.ascontiguousarray(c["pixels"][:, :c["C"]]))
    d["counter"] = torch.tensor([c["counter"], c["N"]], dtype=torch.int32, device=DEV)
    return c, d


def _host(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _finish(W, title):
    print(W.report(title))
    assert not W.fails, "\n".join(W.fails)


def _loss_check(what, got, want, N):
    groups = (N + 15) // 16
    bar = 4 * N * U * want + groups * U * (PRESET + want)
    print(f"{what}: loss error / bar = {abs(got - (PRESET + want)) / bar:.3g}")
    assert abs(got - (PRESET + want)) <= bar


# ------------------------------------------------------------------------------------------------------------- the forwards
@functools.lru_cache(maxsize=None)
def _forward(i, blend):
    c, d = _inputs(i)
    N, M, C = c["N"], c["M"], c["C"]
    r = dict(ws=_nan(N), depth=_nan(N), image=_nan(N, C))
    if blend:
        r["out"] = _nan(N, C)
        _rb().composite_rays_train_forward_blend(d["sigmas"], d["rgbs"], d["deltas"], d["rays"], M, N, r["ws"], r["depth"],
                                                 r["image"], d["bg"], r["out"])
    else:
        _rb().composite_rays_train_forward(d["sigmas"], d["rgbs"], d["deltas"], d["rays"], M, N, r["ws"], r["depth"],
                                           r["image"])
    return r


@pytest.mark.parametrize("blend", [False, True], ids=["forward", "forward_blend"])
@pytest.mark.parametrize("i", ALL)
def test_forward(i, blend):
    W = R.Worst()
    R.check_run(W, f"case {i}", i, "plain", _host(_forward(i, blend)))
    _finish(W, f"case {i} composite_rays_train_forward{'_blend' if blend else ''}:")


# ------------------------------------------------------------------------------------------------------------ the backwards
@pytest.mark.parametrize("i", ALL)
def test_backward(i):
    """Random fp32 g_image, g_ws; weights_sum and image as the forward wrote them.  Rows no marched ray owns stay NaN."""
    c, d = _inputs(i)
    N, M, C = c["N"], c["M"], c["C"]
    f = _forward(i, True)
    r = dict(gs=_nan(M), gr=_nan(M, C))
    _rb().composite_rays_train_backward(d["g_ws"], d["g_image"], d["sigmas"], d["rgbs"], d["deltas"], d["rays"], f["ws"],
                                        f["image"], M, N, r["gs"], r["gr"])
    W = R.Worst()
    R.check_run(W, f"case {i}", i, "plain", _host(r))
    _finish(W, f"case {i} composite_rays_train_backward:")


@pytest.mark.parametrize("i", ALL)
def test_backward_mse(i):
    """Gradients of the MSE on the forward's own out_image; zero rows; the loss added to a preset 0.25."""
    c, d = _inputs(i)
    N, M, C = c["N"], c["M"], c["C"]
    f = _forward(i, True)
    r = dict(gs=_nan(M), gr=_nan(M, C))
    loss = torch.full((), PRESET, dtype=torch.float32, device=DEV)
    _rb().composite_rays_train_backward_mse(f["out"], d["target"], c["grad_scale"], d["bg"], d["counter"], d["sigmas"], d["rgbs"],
                                            d["deltas"], d["rays"], f["ws"], f["image"], M, N, r["gs"], r["gr"], loss)
    got = _host(r)
    got["out"] = f["out"].cpu().numpy()
    W = R.Worst()
    R.check_run(W, f"case {i}", i, "mse", got)
    _finish(W, f"case {i} composite_rays_train_backward_mse:")
    want = float(((got["out"].astype(np.float64) - c["target"].astype(np.float64)) ** 2).sum() / (C * N))
    _loss_check(f"case {i} backward_mse", float(loss), want, N)


@pytest.mark.parametrize("i", ALL)
def test_fwd_bwd_mse(i):
    """weights_sum, image, out_image, both gradients, the zero rows and the loss from one launch."""
    c, d = _inputs(i)
    N, M, C = c["N"], c["M"], c["C"]
    r = dict(ws=_nan(N), image=_nan(N, C), out=_nan(N, C), gs=_nan(M), gr=_nan(M, C))
    loss = torch.full((), PRESET, dtype=torch.float32, device=DEV)
    _rb().composite_rays_train_fwd_bwd_mse(d["sigmas"], d["rgbs"], d["deltas"], d["rays"], M, N, r["ws"], r["image"], d["bg"],
                                           r["out"], d["target"], c["grad_scale"], d["counter"], r["gs"], r["gr"], loss)
    got = _host(r)
    W = R.Worst()
    R.check_run(W, f"case {i}", i, "mse", got)
    _finish(W, f"case {i} composite_rays_train_fwd_bwd_mse:")
    want = float(((got["out"].astype(np.float64) - c["target"].astype(np.float64)) ** 2).sum() / (C * N))
    _loss_check(f"case {i} fwd_bwd_mse", float(loss), want, N)


def _frames(i, alpha, weight, loss0):
    c, d = _inputs(i)
    N, M, C = c["N"], c["M"], c["C"]
    r = dict(ws=_nan(N), image=_nan(N, C), out=_nan(N, C), gs=_nan(M), gr=_nan(M, C), gt=_nan(N, C), err=_nan(N),
             loss=torch.full((), loss0, dtype=torch.float32, device=DEV))
    _rb().composite_rays_train_fwd_bwd_frames(d["sigmas"], d["rgbs"], d["deltas"], d["rays"], M, N, r["ws"], r["image"],
                                              d["bg"], r["out"], d["pixels_alpha" if alpha else "pixels"], weight,
                                              d["counter"], r["gs"], r["gr"], r["gt"], r["err"], r["loss"])
    return _host(r)


@pytest.mark.parametrize("alpha", [False, True], ids=["pixels", "pixels_alpha"])
@pytest.mark.parametrize("i", ALL)
def test_fwd_bwd_frames(i, alpha):
    """The frame tail at weight 0.3: everything the MSE form writes, against fp64 and against fl(0.3 * the same call at
    weight 1); gt_out against the fp64 mix, err_out and the loss against fp64 from the written out_image and gt_out."""
    c = R.make_case(i)
    N, C = c["N"], c["C"]
    form = "frames_alpha" if alpha else "frames"
    got, one = _frames(i, alpha, R.W03, PRESET), _frames(i, alpha, 1.0, 0.0)
    W = R.Worst()
    R.check_run(W, f"case {i}", i, form, got, one)
    _, by_id = R.row_families(c)
    W.compare(f"case {i}", "gt_out", R.frame_gt(c, alpha), got["gt"], by_id)
    err = ((got["out"].astype(np.float64) - got["gt"].astype(np.float64)) ** 2).sum(1) / C
    W.compare(f"case {i}", "err_out", (err, (C + 3) * U * err + R.ETA), got["err"], by_id)
    _finish(W, f"case {i} composite_rays_train_fwd_bwd_frames ({form}):")
    _loss_check(f"case {i} fwd_bwd_frames {form}", float(got["loss"]), R.W03 * float(err.sum()) / N, N)


# ------------------------------------------------------------------------------------------------------ inference compositing
@pytest.mark.parametrize("C", [1, 2, 3])
def test_composite_rays_two_rounds(C):
    """8 then 16 samples a ray; the second round on the survivors, from the nonzero sums the first one left.  Rays end on a
    delta == 0 terminator, after the sample whose pre-sample T is below 1e-5, or not at all."""
    c = R.infer_case(C)
    N = c["N"]
    ws, depth, image = (torch.zeros(s, dtype=torch.float32, device=DEV) for s in (N, N, (N, C)))
    alive = list(range(N))
    rays_t = c["nears"][c["rays"][:, 0]].copy()
    W = R.Worst()
    ended = []
    for rnd in (0, 1):
        ids = c["rays"][alive, 0]
        ref, keep = R.infer_round_reference(c, rnd, alive, rays_t, ws.cpu().numpy(), depth.cpu().numpy(), image.cpu().numpy())
        assert keep.mean() >= 0.99
        sig, dl, rgb = R.infer_round_inputs(c, rnd, alive)
        A, n_step = len(alive), R.INFER_STEPS[rnd]
        t_dev = _dev(rays_t)
        _rb().composite_rays(A, n_step, _dev(ids.astype(np.int32)), t_dev, _dev(sig.reshape(-1)), _dev(rgb.reshape(-1, C)),
                             _dev(dl.reshape(-1, 2)), ws, depth, image)
        rays_t = t_dev.cpu().numpy()
        fam = np.full(int(keep.sum()), "INFER", dtype=object)
        for name, got in (("rays_t", rays_t), ("ws", ws.cpu().numpy()[ids]), ("depth", depth.cpu().numpy()[ids]),
                          ("image", image.cpu().numpy()[ids])):
            r = ref["t" if name == "rays_t" else name]
            W.compare(f"round {rnd}", f"{name} round {rnd}", (r[0][keep], r[1][keep]), got[keep], fam)
        ended.append(int((rays_t < 0).sum()))
        alive = [n for n, t in zip(alive, rays_t) if t >= 0]
        rays_t = rays_t[rays_t >= 0].copy()
    _finish(W, f"composite_rays C = {C}; rays ended per round {ended}, alive after both {len(alive)}:")
    assert ended[0] > 10 and ended[1] > 10 and len(alive) > 5


@pytest.mark.parametrize("C", [1, 2, 3])
def test_composite_rays_frame(C):
    """weights_sum, the blended image, the normalised depth and the `used` count of the whole-frame kernel."""
    c = R.infer_case(C)
    N, M = c["N"], c["M"]
    ref = R.infer_frame_reference(c)
    keep = ref["keep"]
    assert keep.mean() >= 0.99
    r = dict(ws=_nan(N), depth=_nan(N), image=_nan(N, C))
    used = torch.zeros(1, dtype=torch.int32, device=DEV)
    _rb().composite_rays_frame(_dev(c["sigmas"]), _dev(c["rgbs"]), _dev(c["deltas"]), _dev(c["rays"]), N, M, _dev(c["nears"]),
                               _dev(c["fars"]), _dev(c["bg"]), r["ws"], r["depth"], r["image"], used)
    W = R.Worst()
    fam = np.full(int(keep.sum()), "INFER", dtype=object)
    for name, got in _host(r).items():
        W.compare("frame", name, (ref[name][0][keep], ref[name][1][keep]), got[keep], fam)
    _finish(W, f"composite_rays_frame C = {C}:")
    if keep.all():
        assert int(used) == int(ref["used"].sum())
