"""csrc/view_finish.hip on the GPU against enerf_amd/view.py's torch statement on the same tensors,
and TrainHarness.test / ViewRenderer end to end on the native routes.

Bars.  Float outputs are measured against the statement evaluated in fp64: the kernel may deviate by four times what the
fp32 torch statement itself deviates on the same inputs (a powf that differs from torch's by an ulp in front of the
1.055 p - 0.055 cancellation), at least 1e-6; NaN positions coincide.  out_u8 is exactly to_u8 of the same launch's
out_f32, and differs from the fp64 statement's bytes only where the fp64 value times 255 lies within 1e-3 of an integer, by
1 there.  The nearest-pixel choice and enerf_view_minmax are exact; so is the running mean without the colour curve
(products, sums and quotients rounded once, as numpy's fp32)."""
import argparse as ap

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import det_fill_

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(5, 7, 12, 16), (11, 13, 30, 35), (24, 32, 24, 32), (7, 3, 257, 1)]       # 257 = one block of 256 and one more


def _image(h, w, C, seed, special=True):
    """Uniform in [-0.1, 1.2] (both branches of the curve, the clamp, negative powf arguments), a few NaN / inf entries."""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(h, w, C, generator=g) * 1.3 - 0.1
    depth = torch.rand(h, w, generator=g) * 1.3 - 0.1
    if special:
        flat = img.view(-1)
        k = torch.randperm(flat.numel(), generator=g)[:3]
        flat[k[0]] = float("nan")
        if flat.numel() > 8:
            flat[k[1]], flat[k[2]] = float("inf"), -float("inf")
        depth.view(-1)[int(k[0]) % depth.numel()] = float("nan")
    return img, depth


def _same_nan(a, b):
    assert torch.equal(a.isnan(), b.isnan())


def _check_floats(got, s32, s64, what):
    """got (kernel), s32 (fp32 statement), s64 (fp64 statement), all on the CPU."""
    _same_nan(got, s64)
    inf = s64.isinf()
    assert torch.equal(got[inf].double(), s64[inf]), what
    ok = s64.isfinite()
    own = (s32.double() - s64)[ok].abs().max().item() if ok.any() else 0.0
    err = (got.double() - s64)[ok].abs().max().item() if ok.any() else 0.0
    assert err <= max(4 * own, 1e-6), (what, err, own)
    return err, own


def _bytes_vs_fp64(u8, s64, what):
    """Bytes against the fp64 statement's: apart only where the fp64 value times 255 lies within 1e-3 of an integer, by 1."""
    from enerf_amd import view
    want = view.to_u8_statement(s64)
    s = s64 * 255
    near = (s - s.round()).abs() < 1e-3
    diff = u8.int() - want.int()
    assert (diff[~near] == 0).all() and diff.abs().max() <= 1, what
    return int(near.sum()), int((diff != 0).sum())


def _check_bytes(u8, f32, s64, what):
    from enerf_amd import view
    assert torch.equal(u8, view.to_u8_statement(f32)), what              # exactly to_u8 of the same launch's floats
    return _bytes_vs_fp64(u8, s64, what)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("h,w,H,W", SHAPES)
def test_finish_against_the_statement(h, w, H, W, C):
    from enerf_amd import view
    img, depth = _image(h, w, C, seed=h * 100 + C)
    fin = img[img.isfinite()]
    mm = torch.stack([fin.min(), fin.max()])
    g = torch.Generator().manual_seed(5)
    acc0 = torch.rand(H, W, C, generator=g)
    dimg, ddepth, dmm = img.to(DEV), depth.to(DEV), mm.to(DEV)
    worst = (0.0, 0.0)
    for linear in (False, True):
        for use_mm in (False, True):
            for spp in (None, 0, 1, 5):
                for use_depth in (False, True):
                    what = (linear, use_mm, spp, use_depth)
                    kw = dict(out_size=(H, W), linear=linear, spp=spp or 0)
                    acc = None if spp is None else acc0.clone().to(DEV)
                    acc32 = None if spp is None else acc0.clone().to(DEV)
                    acc64 = None if spp is None else acc0.double()
                    got = view.finish(dimg, ddepth if use_depth else None, minmax=dmm if use_mm else None, accum=acc, **kw)
                    s32 = view.finish_statement(dimg, ddepth if use_depth else None, minmax=dmm if use_mm else None,
                                                accum=acc32, **kw)
                    s64 = view.finish_statement(img.double(), depth.double() if use_depth else None,
                                                minmax=mm.double() if use_mm else None, accum=acc64, **kw)
                    assert set(got) == set(s64) == ({"image", "image_u8", "depth", "depth_u8"} if use_depth
                                                    else {"image", "image_u8"})
                    got = {k: v.cpu() for k, v in got.items()}
                    e = _check_floats(got["image"], s32["image"].cpu(), s64["image"], what)
                    worst = max(worst, e)
                    _check_bytes(got["image_u8"], got["image"], s64["image"], what)
                    if spp is not None:
                        assert torch.equal(acc.cpu().isnan(), got["image"].isnan())
                        assert torch.equal(torch.nan_to_num(acc.cpu()), torch.nan_to_num(got["image"]))   # the buffer IS the result
                    if not linear:                       # only exactly rounded operations: the bits of the statement
                        host = view.finish_statement(img, None, minmax=mm if use_mm else None,       # (on the CPU: IEEE)
                                                     accum=None if spp is None else acc0.clone(), **kw)
                        a, b = got["image"], host["image"]
                        _same_nan(a, b)
                        assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)), what
                    if use_depth:                        # steps 1 and 5 only: a gather
                        _same_nan(got["depth"], s64["depth"])
                        assert torch.equal(torch.nan_to_num(got["depth"]).double(), torch.nan_to_num(s64["depth"])), what
                        _check_bytes(got["depth_u8"], got["depth"], s64["depth"], what)
    print(f"\n({h}, {w}) -> ({H}, {W}), C = {C}: worst deviation from fp64 {worst[0]:.3g} (the fp32 statement's own {worst[1]:.3g})")


@pytest.mark.parametrize("h,w,H,W", SHAPES + [(30, 35, 11, 13), (6, 5, 12, 10)])
def test_nearest_pixel_is_f_interpolates(h, w, H, W):
    """An image whose values are its own pixel indices, finished: F.interpolate's choice for every pixel."""
    from enerf_amd import view
    idx = torch.arange(h * w, dtype=torch.float32, device=DEV).reshape(h, w)
    got = view.finish(idx[..., None].contiguous(), idx, out_size=(H, W), outputs=("image", "depth"))
    want = F.interpolate(idx[None, None], size=(H, W), mode="nearest")[0, 0]
    want_cpu = F.interpolate(idx.cpu()[None, None], size=(H, W), mode="nearest")[0, 0]
    assert torch.equal(want.cpu(), want_cpu)
    assert torch.equal(got["image"][..., 0], want) and torch.equal(got["depth"], want)


def test_each_output_null_in_turn_and_constant_image():
    from enerf_amd import view
    h, w, H, W, C = 11, 13, 30, 35, 3
    img, depth = _image(h, w, C, seed=9)
    dimg, ddepth = img.to(DEV), depth.to(DEV)
    full = view.finish(dimg, ddepth, out_size=(H, W), linear=True)
    for drop in view.OUTPUTS:
        outs = tuple(o for o in view.OUTPUTS if o != drop)
        got = view.finish(dimg, ddepth, out_size=(H, W), linear=True, outputs=outs)
        assert set(got) == set(outs)
        for k in outs:
            _same_nan(got[k].float(), full[k].float())
            assert torch.equal(torch.nan_to_num(got[k].float()), torch.nan_to_num(full[k].float())), (drop, k)
    only = view.finish(dimg, ddepth, out_size=(H, W), outputs=("depth_u8",))
    assert set(only) == {"depth_u8"} and torch.equal(only["depth_u8"], full["depth_u8"])
    acc = torch.zeros(H, W, C, device=DEV)
    got = view.finish(dimg, None, out_size=(H, W), linear=True, accum=acc, spp=0, outputs=("image_u8",))
    assert torch.equal(got["image_u8"], full["image_u8"])
    assert torch.equal(torch.nan_to_num(acc), torch.nan_to_num(full["image"]))
    # the running buffer as the ONLY colour output: it is the result (out_f32 = accum in the library's call)
    for spp in (0, 3):
        acc, acc2 = (torch.full((H, W, C), 0.25, device=DEV) for _ in range(2))
        got = view.finish(dimg, None, out_size=(H, W), linear=True, accum=acc, spp=spp, outputs=("image",))
        both = view.finish(dimg, None, out_size=(H, W), linear=True, accum=acc2, spp=spp, outputs=("image", "image_u8"))
        assert set(got) == {"image"} and got["image"].data_ptr() == acc.data_ptr()
        _same_nan(acc, acc2)
        assert torch.equal(torch.nan_to_num(acc), torch.nan_to_num(acc2))
        host = view.finish_statement(img, None, out_size=(H, W), linear=True, accum=torch.full((H, W, C), 0.25), spp=spp,
                                     outputs=("image",))["image"]
        assert torch.equal(view.to_u8_statement(acc.cpu()), both["image_u8"].cpu())
        ok = host.isfinite()
        assert (acc.cpu() - host)[ok].abs().max() <= 1e-6
    # max == min: the scaled frame is 0, not 0 / 0
    const = torch.full((h, w, C), 0.3, device=DEV)
    mm = view.minmax(const)
    assert mm.tolist() == [pytest.approx(0.3), pytest.approx(0.3)] and mm[0] == mm[1]
    got = view.finish(const, None, out_size=(H, W), minmax=mm, linear=True)
    assert (got["image"] == 0).all() and (got["image_u8"] == 0).all()
    with pytest.raises(RuntimeError, match="view_finish"):
        from enerf_amd import _lib as L
        L.check(L.lib().enerf_view_finish(dimg.data_ptr(), None, h, w, 4, H, W, 0, None, None, 0, None, None, None, None,
                                          L.stream_handle()), "view_finish")


def test_bytes_cap_on_one_frame():
    """48 x 64 x 3, fixed seed: the entries where the fp64 value times 255 lies within 1e-3 of an integer -- the only
    ones whose byte may differ from the fp64 statement's, by 1 -- are at most 1 % of the frame.  (tests/test_view_host.py
    confirms the same cap for the fp32 statement alone: 25 entries of 9216 lie that close, none differs.)"""
    from enerf_amd import view
    g = torch.Generator().manual_seed(11)
    img = torch.rand(48, 64, 3, generator=g) * 1.3 - 0.1
    got = view.finish(img.to(DEV), linear=True)
    s64 = view.finish_statement(img.double(), linear=True)
    s32 = view.finish_statement(img.to(DEV), linear=True)
    err, own = _check_floats(got["image"].cpu(), s32["image"].cpu(), s64["image"], "cap")
    near, differ = _check_bytes(got["image_u8"].cpu(), got["image"].cpu(), s64["image"], "cap")
    print(f"\nentries within 1e-3 of an integer: {near} of {img.numel()}; bytes that differ: {differ}; "
          f"floats {err:.3g} from fp64 (the fp32 statement {own:.3g})")
    assert near <= 0.01 * img.numel()


@pytest.mark.parametrize("linear", [False, True])
def test_running_mean_over_five_launches(linear):
    from enerf_amd import evaluate as E
    from enerf_amd import view
    h, w, H, W, C = 11, 13, 30, 35, 3
    g = torch.Generator().manual_seed(21)
    acc = torch.full((H, W, C), float("nan"), device=DEV)                 # (spp == 0 overwrites, whatever is there)
    buf = buf64 = None
    idx = view.nearest_index(h, w, H, W).reshape(-1)
    for spp in range(5):
        f = torch.rand(h, w, C, generator=g) * 1.3 - 0.1
        out = view.finish(f.to(DEV), None, out_size=(H, W), linear=linear, accum=acc, spp=spp, outputs=("image", "image_u8"))
        assert out["image"].data_ptr() == acc.data_ptr()
        up = f.reshape(h * w, C)[idx].reshape(H, W, C)
        up64 = up.double()
        if linear:
            up, up64 = E.linear_to_srgb(up), E.linear_to_srgb(up64)
        up = up.numpy()
        buf = up if spp == 0 else (buf * spp + up) / (spp + 1)            # nerf/gui.py:143 in numpy fp32
        buf64 = up64 if spp == 0 else (buf64 * spp + up64) / (spp + 1)
        assert buf.dtype == np.float32
        got = acc.cpu()
        if linear:
            ok = buf64.isfinite()
            _same_nan(got, buf64)
            own = (torch.from_numpy(buf).double() - buf64)[ok].abs().max().item()
            err = (got.double() - buf64)[ok].abs().max().item()
            assert err <= max(4 * own, 1e-6), (spp, err, own)
        else:
            assert np.array_equal(got.numpy(), buf), spp
        assert torch.equal(out["image_u8"].cpu(), view.to_u8_statement(got))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 131075])
def test_minmax_is_exact(n):
    from enerf_amd import view
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    want = torch.stack(torch.aminmax(x))
    assert torch.equal(view.minmax(x.to(DEV).reshape(1, n, 1)).cpu(), want)
    if n > 1:                                                            # NaNs are skipped, wherever they stand
        x[torch.randperm(n, generator=g)[:max(1, n // 7)]] = float("nan")
        x[0] = x[-1] = float("nan")
        fin = x[~x.isnan()]
        if fin.numel():
            assert torch.equal(view.minmax(x.to(DEV).reshape(n, 1, 1)).cpu(), torch.stack(torch.aminmax(fin)))
            assert torch.equal(view.minmax_statement(x.to(DEV).reshape(n, 1, 1)).cpu(), torch.stack(torch.aminmax(fin)))
    nan = torch.full((n, 1, 1), float("nan"), device=DEV)
    assert view.minmax(nan).tolist() == [0.0, 1.0]
    assert view.minmax(torch.zeros(0, 1, 1, device=DEV)).tolist() == [0.0, 1.0]


# ---------------------------------------------------------------------------------------------------- end to end
H0, W0 = 24, 32


def _views(n, seed):
    from test_view_host import gui_pose, INTRINSICS
    from enerf_amd.frame_sampler import FrameSampler
    poses = torch.stack([torch.from_numpy(gui_pose(seed + k)) for k in range(n)]).to(DEV)
    s = FrameSampler(poses, INTRINSICS, H0, W0, num_rays=-1)
    return [s.batch(i) for i in range(n)]


def _record(model):
    """Every model.render from here on is kept: -> the list of (image, depth) as returned, cloned."""
    kept, render = [], model.render

    def recording(*a, **k):
        out = render(*a, **k)
        kept.append((out["image"].detach().clone(), out["depth"].detach().clone()))
        return out

    model.render = recording
    return kept


def _tree(root):
    import os
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _png_vs_fp64(path, s64, what):
    """A written PNG against the fp64 statement of the render it was made from (the bar of the bytes above)."""
    from enerf_amd import evaluate as E
    img = torch.from_numpy(E.read_png(path).copy())
    s64 = s64[..., 0] if s64.dim() == 3 and s64.shape[-1] == 1 else s64
    assert img.shape == s64.shape, what
    return _bytes_vs_fp64(img, s64, what)


def _same_renders(a, b):
    assert len(a) == len(b) and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("C,color_space", [(3, "linear"), (1, "srgb")])
def test_test_and_view_renderer_end_to_end(fp16, C, color_space, tmp_path, monkeypatch):
    """The native run against the same harness with view.finish forced onto the statement, bars as above: the renders of
    both runs are recorded (they are the same tensors, asserted), the statement is evaluated on them in fp64, and the
    native floats may be four times as far from it as the statement run's (floor 1e-6); bytes and PNGs differ from the
    fp64 bytes only next to an integer."""
    import os
    from test_view_host import gui_pose, INTRINSICS
    from enerf_amd import stratified, view
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    torch.manual_seed(3)
    model = NeRFNetwork(encoding="hashgrid", bound=1, cuda_ray=False, out_dim_color=C)
    det_fill_(list(model.parameters()), 3, -0.5, 0.5)
    model = model.to(DEV)
    h = TrainHarness(model, fp16=fp16, ema_decay=0.9)
    opt = ap.Namespace(out_dim_color=C, color_space=color_space, render_kwargs={"num_steps": 16})
    linear = color_space == "linear"
    views = _views(3, seed=30)
    kept = _record(model)
    model.train()
    calls = stratified.stats["calls"]
    paths = h.test(views, opt, str(tmp_path / "native"), name="v", write_depth=True)
    assert stratified.stats["calls"] - calls >= 3 and model.training and "mlp_precision" not in model.__dict__
    assert len(paths) == 3
    test_renders = list(kept)
    del kept[:]

    def frames(r):
        out = []
        for ds in (1.0, 0.5):
            for k in range(3):
                torch.manual_seed(50 + k)
                f = r.frame(gui_pose(40), downscale=ds)
                assert f["spp"] == k + 1
                out.append({k2: (v.clone() if torch.is_tensor(v) else v) for k2, v in f.items()})
        return out

    r = view.ViewRenderer(h, H0, W0, INTRINSICS, opt)
    r.frame(gui_pose(39))                                                 # (first use: allocations, code objects)
    del kept[:]
    calls = stratified.stats["calls"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        native = frames(r)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert stratified.stats["calls"] - calls >= 6 and model.training
    frame_renders = list(kept)
    del kept[:]
    # the same harness with view.finish forced onto the statement
    monkeypatch.setattr(view, "finish", view.finish_statement)
    monkeypatch.setattr(view, "minmax", view.minmax_statement)
    h.test(views, opt, str(tmp_path / "statement"), name="v", write_depth=True)
    _same_renders(kept, test_renders)
    del kept[:]
    stated = frames(view.ViewRenderer(h, H0, W0, INTRINSICS, opt))
    _same_renders(kept, frame_renders)
    # test(): both trees against the fp64 statement of the recorded renders
    assert _tree(tmp_path / "native") == _tree(tmp_path / "statement") and len(_tree(tmp_path / "native")) == 6
    for i, (img, dep) in enumerate(test_renders):
        s64 = view.finish_statement(img.reshape(H0, W0, C).double().cpu(), dep.reshape(H0, W0).double().cpu(), linear=linear)
        for d in ("native", "statement"):
            _png_vs_fp64(os.path.join(tmp_path, d, f"v_{i:04d}.png"), s64["image"], (d, i))
            _png_vs_fp64(os.path.join(tmp_path, d, "depth", f"v_{i:04d}_depth.png"), s64["depth"], (d, i, "depth"))
    # frame(): the running buffers against the fp64 statement's running buffer over the recorded renders
    for j, ds in enumerate((1.0, 0.5)):
        rH, rW = int(H0 * ds), int(W0 * ds)
        acc64 = torch.zeros(H0, W0, C, dtype=torch.float64)
        for k in range(3):
            a, b = native[3 * j + k], stated[3 * j + k]
            img, dep = frame_renders[3 * j + k]
            s64 = view.finish_statement(img.reshape(rH, rW, C).double().cpu(), dep.reshape(rH, rW).double().cpu(),
                                        out_size=(H0, W0), linear=linear, accum=acc64, spp=k)
            assert a["image"].shape == (H0, W0, C) and a["depth"].shape == (H0, W0) and a["image_u8"].dtype == torch.uint8
            assert torch.equal(a["depth"].cpu().double(), s64["depth"]) and torch.equal(a["depth"], b["depth"])
            _check_floats(a["image"].cpu(), b["image"].cpu(), s64["image"], (ds, k))
            _check_bytes(a["image_u8"].cpu(), a["image"].cpu(), s64["image"], (ds, k))
            _bytes_vs_fp64(b["image_u8"].cpu(), s64["image"], (ds, k, "statement"))


def test_test_on_a_cuda_ray_model(tmp_path):
    import os
    from enerf_amd import view
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=1, cuda_ray=True, out_dim_color=3).to(DEV)
    h = TrainHarness(model, occupancy="synthetic")
    opt = ap.Namespace(out_dim_color=3, color_space="linear")
    views = _views(2, seed=60)
    h.epoch = 100
    kept = _record(model)
    h.test(views, opt, str(tmp_path))
    assert _tree(tmp_path) == sorted(["ngp_ep0100_0000.png", "ngp_ep0100_0001.png", "depth/ngp_ep0100_0000_depth.png",
                                      "depth/ngp_ep0100_0001_depth.png"])
    assert len(kept) == 2
    for i, (img, dep) in enumerate(kept):
        s64 = view.finish_statement(img.reshape(H0, W0, 3).double().cpu(), dep.reshape(H0, W0).double().cpu(), linear=True)
        _png_vs_fp64(os.path.join(tmp_path, f"ngp_ep0100_{i:04d}.png"), s64["image"], i)
        _png_vs_fp64(os.path.join(tmp_path, "depth", f"ngp_ep0100_{i:04d}_depth.png"), s64["depth"], (i, "depth"))


def test_render_path_normalized_on_the_device(tmp_path, monkeypatch):
    import os
    from test_view_host import gui_pose, INTRINSICS
    from enerf_amd import view
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.render_path import interpolate_poses
    from enerf_amd.trainer import TrainHarness
    torch.manual_seed(3)
    model = NeRFNetwork(encoding="hashgrid", bound=1, cuda_ray=False, out_dim_color=1)
    det_fill_(list(model.parameters()), 3, -0.5, 0.5)
    h = TrainHarness(model.to(DEV))
    opt = ap.Namespace(out_dim_color=1, render_kwargs={"num_steps": 16})
    poses = interpolate_poses(gui_pose(70), gui_pose(71), 2)
    kept = _record(h.model)
    h.render_path(poses, INTRINSICS, H0, W0, opt, str(tmp_path / "native"), normalize=True)
    renders = list(kept)
    del kept[:]
    monkeypatch.setattr(view, "finish", view.finish_statement)
    monkeypatch.setattr(view, "minmax", view.minmax_statement)
    h.render_path(poses, INTRINSICS, H0, W0, opt, str(tmp_path / "statement"), normalize=True)
    _same_renders(kept, renders)
    assert _tree(tmp_path / "native") == _tree(tmp_path / "statement") and len(_tree(tmp_path / "native")) == 9
    for i, (img, dep) in enumerate(renders):
        img64 = img.reshape(H0, W0, 1).double().cpu()
        # (min and max are values of the frame: exact in fp32, so the fp64 statement scales by the same two numbers)
        s64 = view.finish_statement(img64, dep.reshape(H0, W0).double().cpu(), minmax=view.minmax_statement(img64))
        a, b = (torch.from_numpy(np.load(tmp_path / d / "raws" / f"{i}.npy")) for d in ("native", "statement"))
        assert a.shape == (H0, W0, 1) and a.min() == 0 and a.max() == 1
        _check_floats(a, b, s64["image"], i)
        for d in ("native", "statement"):
            _png_vs_fp64(os.path.join(tmp_path, d, "rgb", f"{i}.png"), s64["image"], (d, i))
            _png_vs_fp64(os.path.join(tmp_path, d, "depth", f"{i}_depth.png"), s64["depth"], (d, i, "depth"))
