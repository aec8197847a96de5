"""TrainHarness.test / render_path and ViewRenderer on the CPU (enerf_amd/view.py): the reference's
own Trainer.test and its GUI's accumulation around Trainer.test_gui reproduced (tests/golden/ref_view.npz, minted by
tests/refcheck/mint_view_golden.py), the statement's pieces, the file trees, the writer behind the render and the
renderer's bookkeeping."""
import argparse as ap
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import det_fill_, golden
from test_eval_host import make_views, BOUND, FILL

H, W, V = 24, 32, 3
INTRINSICS = (40.0, 40.0, 16.0, 12.0)
TEST_CASES = {                                # the golden's runs of the reference's Trainer.test
    "t_srgb3": dict(seed=41, C=3, color_space="srgb"),
    "t_lin1": dict(seed=42, C=1, color_space="linear"),
}
GUI_CASES = {                                 # ... and of NeRFGUI.test_step around Trainer.test_gui, `calls` times each
    "g_srgb3": dict(seed=43, C=3, color_space="srgb", downscale=1, calls=3, bg=True),
    "g_lin1": dict(seed=44, C=1, color_space="linear", downscale=0.37, calls=3, bg=False),
    "g_lin3": dict(seed=45, C=3, color_space="linear", downscale=0.37, calls=3, bg=True),
}


def gui_pose(seed):
    """A cam2world pose [4, 4] fp32: the camera near (0, 0, 1.5), looking down -z at the [-1, 1]^3 box, a little turned."""
    from scipy.spatial.transform import Rotation
    g = np.random.default_rng(seed)
    R = Rotation.from_euler("xyz", g.uniform(-0.1, 0.1, 3)).as_matrix() @ np.diag([1.0, -1.0, -1.0])
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = R
    pose[:3, 3] = np.array([0.0, 0.0, 1.5]) + g.uniform(-0.1, 0.1, 3)
    return pose


def gui_bg(c):
    return torch.tensor([0.2, 0.5, 0.8])[:c["C"]].clone() if c["bg"] else None


def path_inputs():
    """12 seeded cam2world poses [12, 4, 4] fp64 and 5 rows [t, px, py, pz, qx, qy, qz, qw]."""
    from scipy.spatial.transform import Rotation
    g = np.random.default_rng(12)
    poses = np.tile(np.eye(4), (12, 1, 1))
    poses[:, :3, :3] = Rotation.from_euler("xyz", g.uniform(-0.4, 0.4, (12, 3))).as_matrix()
    poses[:, :3, 3] = g.uniform(-1.0, 1.0, (12, 3))
    q = g.normal(size=(5, 4))
    quats = np.concatenate([np.arange(5.0)[:, None], g.uniform(-1, 1, (5, 3)), q / np.linalg.norm(q, axis=1, keepdims=True)], 1)
    return poses, quats


def _model(c):
    from enerf_amd.network import NeRFNetwork
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=BOUND, cuda_ray=False, out_dim_color=c["C"])
    det_fill_(list(model.parameters()), c["seed"], *FILL)
    return model


def _opt(c):
    return ap.Namespace(out_dim_color=c["C"], color_space=c["color_space"], render_kwargs={"num_steps": 16})


def _bytes_match(got, frames_f32, ref_bytes):
    """`got` equals the reference's bytes, except where the reference wrapped a value above 255 that to_u8 clips."""
    wrapped = np.asarray(frames_f32, np.float32) * 255 >= 256
    assert np.array_equal(got[~wrapped], ref_bytes[~wrapped])
    assert (got[wrapped] == 255).all()


# ------------------------------------------------------------------------------------------- against the reference
@pytest.mark.parametrize("tag", list(TEST_CASES))
def test_test_reproduces_the_reference_trainer(tag, cpu_oracle_backend, tmp_path):
    from enerf_amd import evaluate as E
    from enerf_amd import view
    from enerf_amd.trainer import TrainHarness
    g, c = golden("ref_view"), TEST_CASES[tag]
    model = _model(c)
    h = TrainHarness(model)
    h.epoch = 100
    views = make_views(c["seed"], V, H, W, c["C"], False)
    renders = []
    render = model.render
    model.render = lambda *a, **k: renders.append(render(*a, **k)) or renders[-1]
    model.train()
    paths = h.test(views, _opt(c), str(tmp_path), name="t")
    assert model.training
    # the float frames first, to the bar tests/test_eval_host.py holds the same renders to
    got = np.stack([r["image"].reshape(H, W, c["C"]).numpy() for r in renders])
    np.testing.assert_allclose(got, g[f"{tag}_render"], rtol=0, atol=1e-6)
    assert [os.path.relpath(p, tmp_path) for p in paths] == list(g[f"{tag}_names"][0::2])
    linear = c["color_space"] == "linear"
    for i, p in enumerate(paths):
        shown = torch.from_numpy(g[f"{tag}_render"][i])
        shown = E.linear_to_srgb(shown) if linear else shown
        ref = g[f"{tag}_bytes"][i]
        ref = ref[..., ::-1] if c["C"] == 3 else ref[..., 0]              # (cv2's BGR order undone)
        # the files, from OUR renders: the same bytes wherever our frame and the reference's agree on the byte ...
        img = E.read_png(p)
        ours = view.finish_statement(torch.from_numpy(got[i]), linear=linear, outputs=("image_u8",))["image_u8"].numpy()
        assert np.array_equal(img, ours[..., 0] if c["C"] == 1 else ours)
        edge = np.abs(shown.numpy() * 255 - np.rint(shown.numpy() * 255)) < 1e-3       # (1e-6 apart, times 255)
        edge = edge[..., 0] if c["C"] == 1 else edge
        wrapped = (shown.numpy() * 255 >= 256)
        wrapped = wrapped[..., 0] if c["C"] == 1 else wrapped
        keep = ~edge & ~wrapped
        assert np.array_equal(img[keep], ref[keep]) and keep.mean() > 0.95
        # ... and the statement on the REFERENCE's frame: its bytes exactly, but for the wrap
        mine = view.finish_statement(torch.from_numpy(g[f"{tag}_render"][i]), linear=linear,
                                     outputs=("image_u8",))["image_u8"].numpy()
        _bytes_match(mine[..., 0] if c["C"] == 1 else mine, shown.numpy()[..., 0] if c["C"] == 1 else shown.numpy(), ref)
        dref = g[f"{tag}_depth_bytes"][i]
        dmine = view.finish_statement(torch.zeros(H, W, 1), torch.from_numpy(g[f"{tag}_depth"][i]),
                                      outputs=("depth_u8",))["depth_u8"].numpy()
        _bytes_match(dmine, g[f"{tag}_depth"][i], dref)
        assert E.read_png(os.path.join(tmp_path, "depth", f"t_{i:04d}_depth.png")).shape == (H, W)


@pytest.mark.parametrize("tag", list(GUI_CASES))
def test_view_renderer_reproduces_the_reference_gui(tag, cpu_oracle_backend, monkeypatch):
    """The running buffer after each of the GUI's calls.  The renderer makes its rays with the project's own statement
    (frame_sampler.rays_statement), whose operation order is not get_rays': each component is within four fp32 roundings
    of a value below 1 (4 x 2^-24) of the reference's ray, which is asserted; the frames are then compared on the
    reference's rays, so that the bar of tests/test_eval_host.py (1e-6 on the same renders) measures the render, the
    colour curve, the upsampling and the mean, not how the finest hash level amplifies that rounding."""
    from enerf_amd import view
    from enerf_amd.trainer import TrainHarness
    g, c = golden("ref_view"), GUI_CASES[tag]
    model = _model(c)
    r = view.ViewRenderer(TrainHarness(model), H, W, INTRINSICS, _opt(c))
    pose = gui_pose(c["seed"])
    rays, made = view._rays, []
    ref_d = torch.from_numpy(g[f"{tag}_rays_d"])

    def reference_rays(*a):
        ro, rd = rays(*a)
        made.append(rd)
        assert (ro == torch.from_numpy(g[f"{tag}_rays_o"])).all() and (rd[0] - ref_d).abs().max() <= 4 * 2.0 ** -24
        return ro, ref_d[None].clone()

    monkeypatch.setattr(view, "_rays", reference_rays)
    for k in range(c["calls"]):
        torch.manual_seed(c["seed"] * 100 + k)
        out = r.frame(pose, bg_color=gui_bg(c), downscale=c["downscale"])
        assert out["spp"] == k + 1 and out["image"].shape == (H, W, c["C"]) and out["depth"].shape == (H, W)
        np.testing.assert_allclose(out["image"].numpy(), g[f"{tag}_buffers"][k], rtol=0, atol=1e-6)
        want = view.to_u8_statement(torch.from_numpy(g[f"{tag}_buffers"][k])).numpy()
        near = np.abs(g[f"{tag}_buffers"][k] * 255 - np.rint(g[f"{tag}_buffers"][k] * 255)) < 1e-3
        assert np.array_equal(out["image_u8"].numpy()[~near], want[~near])
    assert len(made) == c["calls"] and made[0].shape == (1, int(H * c["downscale"]) * int(W * c["downscale"]), 3)
    # the whole path on the renderer's OWN rays: the frames the user gets.  The unit of the bar is the reference's own
    # error under that change: how far ITS buffers move when every component of its rays is moved by one fp32 rounding
    # (the fixture's `*_one_rounding`: 2.2e-5, 1.0e-5, 1.6e-5 for the three cases; the finest hash level amplifies 6e-8 of a
    # ray that much); the rays above are held to four roundings, so to four of those units
    monkeypatch.setattr(view, "_rays", rays)
    r = view.ViewRenderer(TrainHarness(model), H, W, INTRINSICS, _opt(c))
    worst = 0.0
    for k in range(c["calls"]):
        torch.manual_seed(c["seed"] * 100 + k)
        out = r.frame(pose, bg_color=gui_bg(c), downscale=c["downscale"])
        worst = max(worst, float(np.abs(out["image"].numpy() - g[f"{tag}_buffers"][k]).max()))
    print(f"{tag}: own rays, worst deviation from the reference's buffers {worst:.3g} "
          f"(one rounding of the reference's rays moves them {float(g[f'{tag}_one_rounding']):.3g})")
    assert worst <= 4 * float(g[f"{tag}_one_rounding"])


# ------------------------------------------------------------------------------------------- the statement's pieces
def test_statement_pieces():
    from enerf_amd import evaluate as E
    from enerf_amd import view
    g = torch.Generator().manual_seed(7)
    for (h, w, Ho, Wo) in ((5, 7, 12, 16), (11, 13, 30, 35), (8, 11, 24, 32), (24, 32, 24, 32), (9, 9, 4, 5)):
        idx = torch.arange(h * w, dtype=torch.float32).reshape(1, 1, h, w)
        want = F.interpolate(idx, size=(Ho, Wo), mode="nearest")[0, 0].long()
        assert torch.equal(view.nearest_index(h, w, Ho, Wo), want)
        img = torch.rand(h, w, 3, generator=g)
        up = view.finish_statement(img, torch.rand(h, w, generator=g), out_size=(Ho, Wo))
        assert torch.equal(up["image"], F.interpolate(img.permute(2, 0, 1)[None], size=(Ho, Wo), mode="nearest")[0].permute(1, 2, 0))
    x = torch.rand(1000, generator=g) * 1.3 - 0.1
    assert np.array_equal(view.to_u8_statement(x).numpy(), E.to_u8(x.numpy()))
    assert view.to_u8_statement(torch.tensor([float("nan"), float("inf"), -float("inf"), 1.0, 0.999])).tolist() == \
        [0, 255, 0, 255, 254]
    img = torch.rand(6, 5, 2, generator=g)
    img[0, 0, 0] = float("nan")
    mm = view.minmax_statement(img)
    assert mm[0] == img[~img.isnan()].min() and mm[1] == img[~img.isnan()].max()
    assert view.minmax_statement(torch.full((3, 3, 1), float("nan"))).tolist() == [0.0, 1.0]
    assert view.minmax_statement(torch.zeros(0, 4, 1)).tolist() == [0.0, 1.0]
    out = view.finish_statement(img, minmax=mm)["image"]
    assert torch.equal(out[~img.isnan()], ((img - mm[0]) / (mm[1] - mm[0]))[~img.isnan()])
    const = torch.full((4, 4, 1), 0.3)
    assert (view.finish_statement(const, minmax=view.minmax_statement(const))["image"] == 0).all()
    # the running mean: numpy fp32, as the GUI computes it
    acc = torch.empty(6, 5, 2)
    buf = None
    for spp in range(5):
        f = torch.rand(6, 5, 2, generator=g)
        out = view.finish_statement(f, accum=acc, spp=spp, outputs=("image",))["image"]
        buf = f.numpy() if spp == 0 else (buf * spp + f.numpy()) / (spp + 1)
        assert buf.dtype == np.float32 and np.array_equal(out.numpy(), buf) and out.data_ptr() == acc.data_ptr()
    with pytest.raises(ValueError):
        view.finish_statement(torch.zeros(4, 4, 4))
    with pytest.raises(ValueError):
        view.finish_statement(torch.zeros(4, 4, 1), outputs=("depth",))
    with pytest.raises(ValueError):
        view.finish_statement(torch.zeros(4, 4, 1), accum=torch.zeros(4, 4, 1), outputs=())


def test_fp32_statement_bytes_stay_inside_the_cap():
    """The bar of the GPU test's bytes, confirmed for the fp32 statement alone: against the fp64 statement the bytes of
    one seeded 48 x 64 x 3 frame differ only where the fp64 value times 255 lies within 1e-3 of an integer, by 1, and such
    entries are at most 1 % of the frame.  (Measured here: 25 entries of 9216 lie that close, 0.27 %; no byte differs.)"""
    from enerf_amd import view
    g = torch.Generator().manual_seed(11)
    img = torch.rand(48, 64, 3, generator=g) * 1.3 - 0.1
    a = view.finish_statement(img, linear=True, outputs=("image", "image_u8"))
    b = view.finish_statement(img.double(), linear=True, outputs=("image", "image_u8"))
    s = (b["image"] * 255).numpy()
    near = np.abs(s - np.rint(s)) < 1e-3
    diff = a["image_u8"].numpy().astype(int) - b["image_u8"].numpy().astype(int)
    print(f"entries within 1e-3 of an integer: {int(near.sum())} of {near.size}; bytes that differ: {int((diff != 0).sum())}")
    assert near.mean() <= 0.01
    assert (diff[~near] == 0).all() and np.abs(diff).max() <= 1


# ------------------------------------------------------------------------------------------------------- files
class _Model(torch.nn.Module):
    """A stand-in for the network: model.render is a closed form of the rays, counted."""

    def __init__(self, C=3):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))
        self.out_dim_color, self.cuda_ray, self.calls, self.seen = C, False, 0, []

    def get_params(self, lr):
        return [{"params": [self.w], "lr": lr}]

    def render(self, rays_o, rays_d, staged=False, bg_color=None, perturb=False, **kw):
        self.calls += 1
        self.seen.append(dict(training=self.training, w=float(self.w.detach()), perturb=perturb, bg=bg_color, staged=staged, kw=kw,
                              grad=torch.is_grad_enabled(), n=rays_d.shape[1]))
        base = (rays_d[..., :1] * 0.5 + 0.5) * self.w + rays_o[..., 2:3] * 0.1
        shift = torch.arange(self.out_dim_color, dtype=torch.float32) * 0.2
        noise = torch.rand_like(base) * 0.01 if perturb else 0
        return {"image": base + shift + noise, "depth": rays_d[..., 2].abs()}


def _harness(C=3, **kw):
    from enerf_amd.trainer import TrainHarness
    return TrainHarness(_Model(C), optimizer=torch.optim.Adam, **kw)


def _sampler_views(n=3):
    from enerf_amd.frame_sampler import FrameSampler
    poses = torch.stack([torch.from_numpy(gui_pose(s)) for s in range(n)])
    s = FrameSampler(poses, INTRINSICS, H, W, num_rays=-1)
    return [s.batch(i) for i in range(n)]


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.parametrize("C", [1, 3])
def test_test_file_tree_and_png_round_trip(C, tmp_path):
    from enerf_amd import evaluate as E
    from enerf_amd import view
    h = _harness(C)
    views = _sampler_views()
    opt = ap.Namespace(out_dim_color=C, color_space="linear")
    h.epoch = 7
    paths = h.test(views, opt, str(tmp_path / "a"))
    assert _tree(tmp_path / "a") == [f"ngp_ep0007_{i:04d}.png" for i in range(3)]           # epoch % 100 != 0: no depth
    assert paths == [str(tmp_path / "a" / f"ngp_ep0007_{i:04d}.png") for i in range(3)]
    assert (tmp_path / "a" / "depth").is_dir()
    h.test(views, opt, str(tmp_path / "b"), name="x", write_depth=True)
    assert _tree(tmp_path / "b") == sorted([f"x_{i:04d}.png" for i in range(3)]
                                           + [f"depth/x_{i:04d}_depth.png" for i in range(3)])
    m = h.model
    assert all(not s["training"] and not s["grad"] and s["staged"] and s["bg"] is None and s["perturb"] is False
               and s["kw"]["num_steps"] == 512 and s["kw"]["max_ray_batch"] == 4096 for s in m.seen)
    for i, v in enumerate(views):
        out = m.render(v["rays_o"], v["rays_d"])
        want = view.finish_statement(out["image"].detach().reshape(H, W, C), out["depth"].reshape(H, W), linear=True,
                                     outputs=("image_u8", "depth_u8"))
        img = E.read_png(str(tmp_path / "b" / f"x_{i:04d}.png"))
        assert img.shape == ((H, W) if C == 1 else (H, W, 3))
        assert np.array_equal(img, want["image_u8"].numpy()[..., 0] if C == 1 else want["image_u8"].numpy())
        assert np.array_equal(E.read_png(str(tmp_path / "b" / "depth" / f"x_{i:04d}_depth.png")), want["depth_u8"].numpy())
    h.epoch = 200
    h.test(views[:1], opt, str(tmp_path / "c"))
    assert _tree(tmp_path / "c") == ["depth/ngp_ep0200_0000_depth.png", "ngp_ep0200_0000.png"]


@pytest.mark.parametrize("normalize", [False, True])
def test_render_path_file_tree(normalize, tmp_path):
    from enerf_amd import evaluate as E
    from enerf_amd import frame_sampler as FS
    from enerf_amd import view
    from enerf_amd.render_path import interpolate_poses
    h = _harness(1)
    poses = interpolate_poses(gui_pose(1), gui_pose(2), 3)
    opt = ap.Namespace(out_dim_color=1)
    paths = h.render_path(poses, INTRINSICS, H, W, opt, str(tmp_path), normalize=normalize)
    assert _tree(tmp_path) == sorted([f"rgb/{i}.png" for i in range(4)] + [f"depth/{i}_depth.png" for i in range(4)]
                                     + [f"raws/{i}.npy" for i in range(4)])
    assert paths == [str(tmp_path / "rgb" / f"{i}.png") for i in range(4)]
    assert all(s["bg"] == 1 and s["perturb"] is False and not s["training"] for s in h.model.seen)
    p44 = torch.from_numpy(view._poses44(poses))
    for i in range(4):
        ro, rd, _ = FS.rays_statement(p44, i, INTRINSICS, H, W)
        out = h.model.render(ro[None], rd[None])
        raw = out["image"].detach().reshape(H, W, 1)
        if normalize:
            raw = (raw - raw.min()) / (raw.max() - raw.min())
        assert np.array_equal(np.load(tmp_path / "raws" / f"{i}.npy"), raw.numpy())
        assert np.array_equal(E.read_png(str(tmp_path / "rgb" / f"{i}.png")), E.to_u8(raw.numpy())[..., 0])
        assert np.array_equal(E.read_png(str(tmp_path / "depth" / f"{i}_depth.png")),
                              E.to_u8(out["depth"].reshape(H, W).numpy()))
        if normalize:
            assert raw.min() == 0 and raw.max() == 1


def test_write_behind_equals_synchronous(tmp_path):
    h = _harness(3)
    views = _sampler_views(5)
    opt = ap.Namespace(out_dim_color=3, color_space="srgb")
    h.test(views, opt, str(tmp_path / "behind"), name="v", write_depth=True, write_behind=True)
    h.test(views, opt, str(tmp_path / "sync"), name="v", write_depth=True, write_behind=False)
    assert _tree(tmp_path / "behind") == _tree(tmp_path / "sync") and len(_tree(tmp_path / "sync")) == 10
    for f in _tree(tmp_path / "sync"):
        assert open(tmp_path / "behind" / f, "rb").read() == open(tmp_path / "sync" / f, "rb").read(), f
    poses = np.stack([gui_pose(s) for s in range(4)])
    for wb, d in ((True, "pb"), (False, "ps")):
        h.render_path(poses, INTRINSICS, H, W, opt, str(tmp_path / d), normalize=True, write_behind=wb)
    for f in _tree(tmp_path / "ps"):
        assert open(tmp_path / "pb" / f, "rb").read() == open(tmp_path / "ps" / f, "rb").read(), f


@pytest.mark.parametrize("write_behind", [True, False])
def test_a_failing_writer_raises_from_the_call(write_behind, tmp_path):
    import threading
    from enerf_amd import view
    h = _harness(3)
    views = _sampler_views(6)
    opt = ap.Namespace(out_dim_color=3)
    before = threading.active_count()
    # an unwritable file: a DIRECTORY stands where the third picture should be written
    (tmp_path / "out" / "ngp_ep0001_0002.png").mkdir(parents=True)
    h.model.train()
    with pytest.raises(OSError):
        h.test(views, opt, str(tmp_path / "out"), write_behind=write_behind)
    assert h.model.training and threading.active_count() == before           # the mode is back, the worker has ended
    assert (tmp_path / "out" / "ngp_ep0001_0001.png").is_file()
    # the writer itself: the failure reaches submit() or close(), and the ring never blocks the producer
    w = view.FrameWriter(write_behind, ring=2)
    with pytest.raises(OSError):
        for i in range(8):
            w.submit([("png", str(tmp_path / "out" / "ngp_ep0001_0002.png" / f"{i}.png" / "x"),
                       torch.zeros(4, 4, dtype=torch.uint8))])
        w.close()
    w.close()
    assert threading.active_count() == before


# ------------------------------------------------------------------------------------------------- bookkeeping
def test_view_renderer_bookkeeping():
    from enerf_amd.view import ViewRenderer
    h = _harness(3, ema_decay=0.9)
    m = h.model
    with torch.no_grad():
        h.ema.shadow_params[0].fill_(0.5)                    # the average differs from the weights
    events = []
    for name in ("store", "copy_to", "restore"):
        fn = getattr(h.ema, name)
        setattr(h.ema, name, lambda fn=fn, name=name: (events.append(name), fn())[1])
    render = m.render
    m.render = lambda *a, **k: (events.append("render"), render(*a, **k))[1]
    r = ViewRenderer(h, H, W, INTRINSICS, ap.Namespace(out_dim_color=3, color_space="linear"), max_spp=4)
    pose = gui_pose(3)
    m.train()
    spps = [r.frame(pose)["spp"] for _ in range(7)]
    assert spps == [1, 2, 3, 4, 4, 4, 4] and m.calls == 4                      # nothing is rendered at max_spp
    assert events == ["store", "copy_to", "render", "restore"] * 4
    assert m.training and float(m.w) == 1.0
    assert [s["w"] for s in m.seen] == [0.5] * 4 and [s["perturb"] for s in m.seen] == [1, 1, 2, 3]
    assert all(not s["training"] and not s["grad"] and s["n"] == H * W for s in m.seen)
    last = r.frame(pose)
    assert m.calls == 4 and torch.equal(last["image"], r.frame(pose)["image"])
    # a new pose, downscale or background starts again
    assert r.frame(gui_pose(4))["spp"] == 1 and r.frame(gui_pose(4))["spp"] == 2
    assert r.frame(gui_pose(4), downscale=0.5)["spp"] == 1 and m.seen[-1]["n"] == (H // 2) * (W // 2)
    assert r.frame(gui_pose(4), downscale=0.5)["spp"] == 2
    out = r.frame(gui_pose(4), bg_color=torch.tensor([0.1, 0.2, 0.3]), downscale=0.5)
    assert out["spp"] == 1 and torch.equal(m.seen[-1]["bg"], torch.tensor([0.1, 0.2, 0.3]))
    assert r.frame(gui_pose(4), bg_color=torch.tensor([0.1, 0.2, 0.3]), downscale=0.5)["spp"] == 2
    assert r.frame(gui_pose(4), bg_color=torch.tensor([0.1, 0.2, 0.4]), downscale=0.5)["spp"] == 1
    assert out["image"].shape == (H, W, 3) and out["depth"].shape == (H, W) and out["image_u8"].dtype == torch.uint8
    r.reset()
    assert r.frame(gui_pose(4), bg_color=torch.tensor([0.1, 0.2, 0.4]), downscale=0.5)["spp"] == 1
    # the mode and the weights come back after an exception too
    def boom(*a, **k):
        raise RuntimeError("boom")
    m.render = boom
    m.train()
    with pytest.raises(RuntimeError, match="boom"):
        r.frame(gui_pose(5))
    assert m.training and float(m.w) == 1.0
    m.eval()
    with pytest.raises(RuntimeError, match="boom"):
        r.frame(gui_pose(6))
    assert not m.training


def test_test_uses_no_average_and_restores_the_mode(tmp_path):
    h = _harness(3, ema_decay=0.9)
    with torch.no_grad():
        h.ema.shadow_params[0].fill_(0.5)
    h.model.eval()
    h.test(_sampler_views(1), ap.Namespace(out_dim_color=3), str(tmp_path))
    assert [s["w"] for s in h.model.seen] == [1.0] and not h.model.training     # as the reference's test: the weights
    h.model.train()
    h.model.render = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("boom"))
    with pytest.raises(RuntimeError, match="boom"):
        h.test(_sampler_views(1), ap.Namespace(out_dim_color=3), str(tmp_path))
    assert h.model.training


def test_bad_arguments_return_the_bad_argument_error():
    """enerf_view_finish / enerf_view_minmax refuse before anything is launched: no GPU is needed to ask."""
    from enerf_amd import _lib as L
    lib = L.lib()
    one = 0x1000                                           # (never dereferenced: every call below returns first)
    ok = dict(image=one, depth=None, h=4, w=4, C=3, H=8, W=8, flags=0, minmax=None, accum=None, spp=0, out_f32=one,
              out_u8=None, depth_f32=None, depth_u8=None)
    for change, word in ((dict(C=0), "channels"), (dict(C=4), "channels"), (dict(H=0), "output"), (dict(W=0), "output"),
                         (dict(accum=one, out_f32=None), "accum"), (dict(depth_u8=one), "depth"),
                         (dict(h=0), "image"), (dict(image=None), "image"), (dict(H=1 << 16, W=1 << 16), "output")):
        rc = lib.enerf_view_finish(*{**ok, **change}.values(), None)
        assert rc == -1 and word in lib.enerf_last_error().decode(), (change, rc, lib.enerf_last_error())
    assert lib.enerf_view_finish(*{**ok, "H": 0, "out_f32": None}.values(), None) == 0        # nothing asked: nothing done
    assert lib.enerf_view_finish(*{**ok, "out_f32": None}.values(), None) == 0
    assert lib.enerf_view_minmax(one, 16, None, one, None) == -1 and lib.enerf_view_minmax(None, 16, one, one, None) == -1


def test_exports():
    import enerf_amd
    from enerf_amd import render_path, view
    assert enerf_amd.ViewRenderer is view.ViewRenderer
    assert enerf_amd.spiral_poses is render_path.spiral_poses and enerf_amd.interpolate_poses is render_path.interpolate_poses
    assert enerf_amd.poses_from_quat_list is render_path.poses_from_quat_list
    from enerf_amd.trainer import TrainHarness
    assert callable(TrainHarness.test) and callable(TrainHarness.render_path)
