"""Mint tests/golden/*.npz by running the reference's own Python (this container only).

    cd /root/repo && python -B -m oracle.make_golden

TEST INFRASTRUCTURE ONLY.  The reference has no tests or golden vectors; what it does have is
Python that is an independent statement of parts of the hot path.  This script imports that Python (recipe:
oracle/ref_import.py), drives it on CPU -- the native parts through the reference's own autograd wrappers backed by the
C oracle -- and stores inputs + outputs as small fixtures.  tests/ then check
  (a) enerf_amd's re-stated wrappers / networks / renderer.run / event loss against these fixtures (same oracle backend),
  (b) the oracle's compositing against NeRFRenderer.run's cumprod formula and torch autograd (the only second statement
      of a native kernel the reference contains).
Only data (arrays) is stored; no reference source text.
"""
import argparse
import os
import sys

# the CPU settings tests/conftest.py pins for the suite: fixtures hold the same bits on every x86 machine
os.environ["MKL_CBWR"] = "COMPATIBLE,STRICT"
os.environ["OMP_NUM_THREADS"] = "8"

import numpy as np  # noqa: E402
import torch  # noqa: E402

from . import ref_import  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def det_fill_(params, seed, lo=-1.0, hi=1.0):
    """Deterministic parameter fill shared with the tests (tests/util.py:det_fill_)."""
    g = torch.Generator().manual_seed(seed)
    for p in params:
        p.data.copy_(torch.rand(p.shape, generator=g) * (hi - lo) + lo)


def save(name, **arrays):
    out = {}
    for k, v in arrays.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        out[k] = np.asarray(v)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"  wrote {name}.npz ({', '.join(f'{k}{list(v.shape)}' for k, v in out.items())})")


def pts(n, seed, lo=-1.0, hi=1.0, d=3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, d, generator=g) * (hi - lo) + lo


def gold_grid_wrapper():
    from gridencoder import GridEncoder
    enc = GridEncoder(input_dim=3, num_levels=6, level_dim=2, base_resolution=4, log2_hashmap_size=9,
                      desired_resolution=96)
    det_fill_([enc.embeddings], 11)
    x = pts(96, 12, -1.0, 1.0)
    x[5] = torch.tensor([1.5, 0.0, 0.0])      # out of range -> zeros
    x[6] = torch.tensor([1.0, -1.0, 1.0])     # exactly on the boundary
    x.requires_grad_(True)
    y = enc(x, bound=1)
    w = pts(96, 13, -1, 1, d=12)
    (y * w).sum().backward()
    save("ref_grid_wrapper", x=x, w=w, y=y, grad_embeddings=enc.embeddings.grad, grad_x=x.grad,
         offsets=enc.offsets, per_level_scale=np.float64(enc.per_level_scale))
    # offset tables of the two BASELINE configurations (bound 2 and 3) -- table sizing only
    for bound in (1, 2, 3):
        e = GridEncoder(desired_resolution=2048 * bound)
        save(f"ref_grid_offsets_b{bound}", offsets=e.offsets, per_level_scale=np.float64(e.per_level_scale),
             n_rows=np.int64(e.embeddings.shape[0]))


def gold_sh_wrapper():
    from shencoder import SHEncoder
    for deg in (4, 8):
        enc = SHEncoder(degree=deg)
        d = pts(40, 20 + deg)
        d = d / d.norm(dim=-1, keepdim=True)
        d[3] = d[3] * 0.5     # un-normalised input: kernel must not normalise
        d.requires_grad_(True)
        y = enc(d)
        w = pts(40, 21, d=deg * deg)
        (y * w).sum().backward()
        save(f"ref_sh_wrapper_d{deg}", d=d, w=w, y=y, grad_d=d.grad)


def gold_ffmlp_wrapper():
    from ffmlp import FFMLP
    for (i, o, h, k, B) in ((32, 16, 64, 2, 100), (32, 3, 64, 3, 128)):
        net = FFMLP(i, o, h, k)
        w0 = net.weights.detach().clone()
        net.train()
        x = pts(B, 30 + k, d=i).requires_grad_(True)
        y = net(x)
        gw = pts(B, 31, d=o)
        (y * gw).sum().backward()
        net.eval()
        with torch.no_grad():
            y_inf = net(x.detach())
        save(f"ref_ffmlp_wrapper_k{k}", x=x, gw=gw, y=y, y_inf=y_inf, weights=w0, grad_weights=net.weights.grad,
             grad_x=x.grad)


def _rays(n, seed, bound):
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(n, 3, generator=g) - 0.5) * 0.6 * bound
    o[:, 2] -= 1.6 * bound
    tgt = (torch.rand(n, 3, generator=g) - 0.5) * 1.2 * bound
    d = tgt - o
    d = d / d.norm(dim=-1, keepdim=True)
    return o.unsqueeze(0), d.unsqueeze(0)


def gold_network():
    from nerf.network import NeRFNetwork
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=False, out_dim_color=3)
    det_fill_(list(model.parameters()), 41)
    model.eval()
    x = pts(80, 42, -2, 2)
    d = pts(80, 43)
    d = d / d.norm(dim=-1, keepdim=True)
    sigma, color = model(x, d)
    dens = model.density(x)
    mask = torch.rand(80, generator=torch.Generator().manual_seed(44)) > 0.4
    cm = model.color(x, d, mask=mask, geo_feat=dens["geo_feat"])
    save("ref_network", x=x, d=d, sigma=sigma, color=color, geo_feat=dens["geo_feat"], mask=mask, color_masked=cm)

    # NeRFRenderer.run through the reference (eval mode: deterministic upsampling)
    o, dd = _rays(24, 45, 2)
    for up in (0, 8):
        with torch.no_grad():
            out = model.render(o, dd, staged=False, bg_color=None, perturb=False, num_steps=24, upsample_steps=up,
                               out_dim_color=3)
        save(f"ref_run_up{up}", rays_o=o, rays_d=dd, image=out["image"], depth=out["depth"])
    # training-mode run with gradients (no upsampling: rand-free)
    model.train()
    out = model.render(o, dd, staged=False, bg_color=torch.full((3,), 0.25), perturb=False, num_steps=24,
                       upsample_steps=0, out_dim_color=3)
    loss = (out["image"] ** 2).sum() + out["depth"].sum()
    loss.backward()
    save("ref_run_train", rays_o=o, rays_d=dd, image=out["image"], depth=out["depth"],
         g_sigma0=model.sigma_net[0].weight.grad, g_color2=model.color_net[2].weight.grad,
         g_emb_sum=model.encoder.embeddings.grad.abs().sum(),
         g_emb_l0=model.encoder.embeddings.grad[:4920])


def gold_network_ff():
    from nerf.network_ff import NeRFNetwork
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=False)
    det_fill_([model.encoder.embeddings], 51)
    model.eval()
    x = pts(70, 52, -2, 2)
    d = pts(70, 53)
    d = d / d.norm(dim=-1, keepdim=True)
    with torch.no_grad():
        sigma, rgb = model(x, d)
    save("ref_network_ff", x=x, d=d, sigma=sigma, rgb=rgb, w_sigma=model.sigma_net.weights, w_color=model.color_net.weights)


def gold_composite_vs_run():
    """NeRFRenderer.run's compositing (cumprod formula) on prescribed per-sample sigmas / rgbs, with autograd grads."""
    from nerf.renderer import NeRFRenderer

    N, T = 37, 29
    g = torch.Generator().manual_seed(61)
    sig = (torch.rand(N, T, generator=g) * 6.0).requires_grad_(True)
    sig.data[3] = 0.0                                  # fully transparent ray
    sig.data[4] *= 40.0                                # saturating ray
    rgb = torch.rand(N, T, 3, generator=g).requires_grad_(True)

    class Fake(NeRFRenderer):
        def density(self, x):
            return {"sigma": sig.reshape(-1)}

        def color(self, x, d, mask=None, **kw):
            return rgb.reshape(-1, 3)       # ignore the w>1e-4 mask: the native kernel composites every sample

    m = Fake(bound=1, cuda_ray=False)
    m.train()
    o, d = _rays(N, 62, 1)
    out = m.render(o, d, staged=False, bg_color=torch.zeros(3), perturb=False, num_steps=T, upsample_steps=0,
                   out_dim_color=3)
    image = out["image"][0]
    gi = torch.rand(N, 3, generator=g)
    (image * gi).sum().backward()
    # weights_sum through a second pass with rgb == 1 and its own upstream gradient
    g_sig_img, g_rgb_img = sig.grad.clone(), rgb.grad.clone()
    sig.grad = None
    rgb_saved = rgb.data.clone()
    rgb.data.fill_(1.0)
    out1 = m.render(o, d, staged=False, bg_color=torch.zeros(3), perturb=False, num_steps=T, upsample_steps=0,
                    out_dim_color=3)
    ws = out1["image"][0, :, 0]
    gws = torch.rand(N, generator=g)
    (ws * gws).sum().backward()
    g_sig_ws = sig.grad.clone()
    rgb.data.copy_(rgb_saved)
    # the z/delta sequence run() used (renderer.py:166-176, 228-229)
    from oracle import oracle as O
    nears, fars = O.near_far_from_aabb(o[0].numpy(), d[0].numpy(), m.aabb_train.numpy(), 0.2)
    save("ref_composite_vs_run", rays_o=o[0], rays_d=d[0], nears=nears, fars=fars, sigmas=sig, rgbs=rgb, image=image,
         weights_sum=ws, grad_image=gi, grad_ws=gws, g_sig_img=g_sig_img, g_rgb_img=g_rgb_img, g_sig_ws=g_sig_ws)


def gold_events():
    import argparse as ap
    from nerf.utils import Trainer, get_rays, get_event_rays
    from utils.event_utils import rgb_to_luma, lin_log

    g = torch.Generator().manual_seed(71)
    B, N = 1, 50
    img1 = torch.rand(B, N, 3, generator=g)
    img2 = (img1 + 0.2 * (torch.rand(B, N, 3, generator=g) - 0.5)).clamp(0, 1)
    img3 = torch.rand(B, N, 3, generator=g)
    pols = torch.sign(torch.rand(B, N, generator=g) - 0.5)
    frames = torch.rand(B, N, 3, generator=g)

    class FakeModel:
        def __init__(self):
            self.calls = 0

        def render(self, o, d, **kw):
            self.calls += 1
            im = [img1, img2, img3][(self.calls - 1) % 3].clone().requires_grad_(True)
            self.last = getattr(self, "last", []) + [im]
            return {"image": im, "depth": im[..., 0]}

    results = {}
    cfgs = {
        "luma_linlog": dict(use_luma=1, linlog=1, C_thres=0.2, event_only=1),
        "rgb_linlog": dict(use_luma=0, linlog=1, C_thres=0.2, event_only=1),
        "luma_log": dict(use_luma=1, linlog=0, C_thres=0.2, event_only=1),
        "rgb_log": dict(use_luma=0, linlog=0, C_thres=0.2, event_only=1),
        "normed": dict(use_luma=1, linlog=1, C_thres=-1, event_only=1),
        "both": dict(use_luma=1, linlog=1, C_thres=0.2, event_only=0),
    }
    for name, c in cfgs.items():
        t = Trainer.__new__(Trainer)
        t.device = torch.device("cpu")
        t.out_dim_color = 3
        t.use_luma, t.linlog, t.C_thres, t.event_only = c["use_luma"], c["linlog"], c["C_thres"], c["event_only"]
        t.log_implicit_C_thres = False
        t.negative_event_sampling = False
        t.weight_loss_rgb = 1.0
        t.epoch, t.epoch_start_noEvLoss = 1, 0
        t.criterion = torch.nn.MSELoss(reduction="none")
        if not t.linlog:
            t.log_thres = torch.Tensor([0.0000001])
        t.opt = ap.Namespace()
        t.model = FakeModel()
        data = {"images": frames, "rays_evs_o1": torch.zeros(B, N, 3), "rays_evs_d1": torch.zeros(B, N, 3),
                "rays_evs_o2": torch.zeros(B, N, 3), "rays_evs_d2": torch.zeros(B, N, 3), "pols": pols,
                "rays_o": torch.zeros(B, N, 3), "rays_d": torch.zeros(B, N, 3)}
        delta, gt_pol, loss, _, losses = t.train_step_events(data)
        loss.backward()
        results[f"{name}_loss"] = loss
        results[f"{name}_delta"] = delta
        results[f"{name}_g1"] = t.model.last[0].grad if t.model.last[0].grad is not None else torch.zeros_like(img1)
        results[f"{name}_g2"] = t.model.last[1].grad if t.model.last[1].grad is not None else torch.zeros_like(img1)
        if not c["event_only"]:
            results[f"{name}_g3"] = t.model.last[2].grad
    save("ref_event_loss", img1=img1, img2=img2, img3=img3, pols=pols, frames=frames, **results)
    x = torch.rand(20, 3, generator=g)
    save("ref_event_utils", x=x, luma_esim=rgb_to_luma(x, esim=True), luma_v2e=rgb_to_luma(x, esim=False),
         linlog=lin_log(x * 255, 20))

    # rays
    H, W = 6, 8
    intr = (7.5, 7.0, 3.5, 2.5)
    th = 0.3
    pose = torch.tensor([[np.cos(th), 0, np.sin(th), 0.1], [0, 1, 0, -0.2], [-np.sin(th), 0, np.cos(th), 0.3],
                         [0, 0, 0, 1]], dtype=torch.float32).unsqueeze(0)
    full = get_rays(pose, intr, H, W, -1)
    xs = torch.tensor([0.0, 3.0, 7.0, 2.0])
    ys = torch.tensor([0.0, 5.0, 1.0, 2.0])
    c2w_b = pose[:, :3, :].unsqueeze(1).expand(1, 4, 3, 4).clone()
    c2w_a = c2w_b.clone()
    c2w_a[..., :3, 3] += 0.05
    ev = get_event_rays(xs, ys, c2w_b, c2w_a, intr)
    save("ref_rays", pose=pose, intr=np.array(intr), H=np.int64(H), W=np.int64(W), rays_o=full["rays_o"],
         rays_d=full["rays_d"], xs=xs, ys=ys, c2w_b=c2w_b, c2w_a=c2w_a, **{k: v for k, v in ev.items()})


def gold_no_events():
    """`--negative_event_sampling` (nerf/utils.py:548-565): Trainer.train_step_events with the no-event pair of renders on,
    event-only and with the frame render, C_thres > 0 and = -1 (Cno falls back to 0.25), luma and RGB; and with the term
    gated off by epoch_start_noEvLoss.  The fake model hands out img1, img2, img3, img1, ... per render call."""
    import argparse as ap
    from nerf.utils import Trainer

    g = torch.Generator().manual_seed(171)
    B, N, Nn = 1, 48, 24
    img1 = torch.rand(B, N, 3, generator=g)
    img2 = (img1 + 0.3 * (torch.rand(B, N, 3, generator=g) - 0.5)).clamp(0, 1)
    img3 = torch.rand(B, N, 3, generator=g) * 0.1
    pols = torch.sign(torch.rand(B, N, generator=g) - 0.5)
    frames = torch.rand(B, N, 3, generator=g)
    imgs = [img1, img2, img3]

    class FakeModel:
        def __init__(self):
            self.calls, self.last = 0, []

        def render(self, o, d, **kw):
            im = imgs[self.calls % 3][:, : o.shape[1]].clone().requires_grad_(True)
            self.calls += 1
            self.last.append(im)
            return {"image": im, "depth": im[..., 0]}

    results = {}
    cfgs = {
        "neg_luma": dict(use_luma=1, C_thres=0.2, event_only=1, w_no_ev=0.7, epoch=2, start=0),
        "neg_rgb": dict(use_luma=0, C_thres=0.2, event_only=1, w_no_ev=1.0, epoch=2, start=0),
        "neg_normed": dict(use_luma=1, C_thres=-1, event_only=1, w_no_ev=2.0, epoch=2, start=0),
        "neg_both": dict(use_luma=1, C_thres=0.2, event_only=0, w_no_ev=0.7, epoch=2, start=0),
        "neg_gated": dict(use_luma=1, C_thres=0.2, event_only=1, w_no_ev=0.7, epoch=1, start=1),
    }
    for name, c in cfgs.items():
        t = Trainer.__new__(Trainer)
        t.device = torch.device("cpu")
        t.out_dim_color = 3
        t.use_luma, t.linlog, t.C_thres, t.event_only = c["use_luma"], 1, c["C_thres"], c["event_only"]
        t.log_implicit_C_thres = False
        t.negative_event_sampling = True
        t.w_no_ev = c["w_no_ev"]
        t.weight_loss_rgb = 1.0
        t.epoch, t.epoch_start_noEvLoss = c["epoch"], c["start"]
        t.criterion = torch.nn.MSELoss(reduction="none")
        t.opt = ap.Namespace()
        t.model = FakeModel()
        z, zn = torch.zeros(B, N, 3), torch.zeros(B, Nn, 3)
        data = {"images": frames, "rays_evs_o1": z, "rays_evs_d1": z, "rays_evs_o2": z, "rays_evs_d2": z, "pols": pols,
                "rays_o": z, "rays_d": z, "rays_no_evs_o1": zn, "rays_no_evs_d1": zn, "rays_no_evs_o2": zn,
                "rays_no_evs_d2": zn}
        delta, gt_pol, loss, _, losses = t.train_step_events(data)
        loss.backward()
        results[f"{name}_loss"] = loss
        results[f"{name}_delta"] = delta
        results[f"{name}_loss_no_evs"] = torch.as_tensor(float(losses["loss_no_evs"]))
        results[f"{name}_calls"] = np.int64(t.model.calls)
        for i, im in enumerate(t.model.last):
            results[f"{name}_g{i}"] = im.grad if im.grad is not None else torch.zeros_like(im)
    save("ref_no_event_loss", img1=img1, img2=img2, img3=img3, pols=pols, frames=frames, Nn=np.int64(Nn), **results)


def gold_misc():
    from activation import trunc_exp
    from encoding import FreqEncoder
    x = torch.linspace(-20, 20, 41).requires_grad_(True)
    y = trunc_exp(x)
    y.sum().backward()
    f = FreqEncoder(input_dim=3, max_freq_log2=5, N_freqs=6)
    p = pts(9, 81)
    save("ref_misc", x=x, trunc_exp=y, trunc_exp_grad=x.grad, p=p, freq=f(p))


def gold_sh_literals():
    """The reference's SH kernel is a literal table of 64 polynomials + 3 x 64 partial derivatives
    (shencoder/src/shencoder.cu:51-121 and :131-351).  This job PARSES those assignment statements at mint time and
    evaluates them in float64 numpy at fixed points (on and off the unit sphere) -- i.e. it runs the reference's own
    statement of the math, not ours.  Only the points and the evaluated numbers are stored."""
    import re
    src = open(os.path.join(ref_import.REFERENCE, "shencoder", "src", "shencoder.cu")).read().splitlines()
    body = src[26:383]                                   # kernel_sh: lines 27..383
    pat = re.compile(r"^\s*(outputs|dx|dy|dz)\[(\d+)\]\s*=\s*(.*?);")
    table = {"outputs": {}, "dx": {}, "dy": {}, "dz": {}}
    for line in body:
        m = pat.match(line)
        if not m:
            continue
        expr = re.sub(r"(\d+\.\d*(?:[eE][-+]?\d+)?|\d+)f\b", r"\1", m.group(3))     # 3.0f -> 3.0
        expr = expr.replace("pow(z, 3)", "(z*z*z)")
        table[m.group(1)][int(m.group(2))] = expr
    assert all(sorted(t) == list(range(64)) for t in table.values()), {k: len(v) for k, v in table.items()}
    g = torch.Generator().manual_seed(4242)
    d = (torch.rand(96, 3, generator=g, dtype=torch.float64) * 2 - 1).numpy()
    d[:64] /= np.linalg.norm(d[:64], axis=-1, keepdims=True)          # 64 unit directions, 32 raw points in [-1,1]^3
    d[0] = (0.0, 0.0, 1.0)
    d[1] = (1.0, 0.0, 0.0)
    d[2] = (0.0, -1.0, 0.0)
    d = d.astype(np.float32).astype(np.float64)                       # exactly representable in the kernels' fp32
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    env = dict(x=x, y=y, z=z, xy=x * y, xz=x * z, yz=y * z, x2=x * x, y2=y * y, z2=z * z)
    env.update(x4=env["x2"] ** 2, y4=env["y2"] ** 2, z4=env["z2"] ** 2)
    env.update(x6=env["x4"] * env["x2"], y6=env["y4"] * env["y2"], z6=env["z4"] * env["z2"])
    ev = lambda e: np.broadcast_to(np.asarray(eval(e, {"__builtins__": {}}, env), np.float64), x.shape)  # noqa: E731
    Y = np.stack([ev(table["outputs"][k]) for k in range(64)], -1)                        # [P, 64]
    J = np.stack([np.stack([ev(table[a][k]) for k in range(64)], -1) for a in ("dx", "dy", "dz")], 1)   # [P, 3, 64]
    save("ref_sh_literals", d=d.astype(np.float32), y=Y, dy_dx=J)


def gold_near_far_from_bound():
    """nerf/renderer.py:48-72 near_far_from_bound(type='cube') is the reference's own second statement of the slab
    test of near_far_from_aabb (raymarching.cu:94-158).  Documented deltas: `+1e-15` in the divisor, misses -> 1e9
    (kernel: FLT_MAX), min_near hard-coded to 0.05."""
    from nerf.renderer import near_far_from_bound
    out = {}
    for bound in (1, 2, 3):
        o, d = (t[0] for t in _rays(96, 300 + bound, bound))
        g = torch.Generator().manual_seed(310 + bound)
        o = torch.cat([o, (torch.rand(32, 3, generator=g) * 2 - 1) * bound * 0.9])      # origins inside the cube
        dd = torch.rand(32, 3, generator=g) * 2 - 1
        d = torch.cat([d, dd / dd.norm(dim=-1, keepdim=True)])
        # rays that miss the cube: far outside, pointing sideways
        o = torch.cat([o, torch.tensor([[5.0 * bound, 5.0 * bound, 0.1], [-4.0 * bound, 0.3, 6.0 * bound]])])
        d = torch.cat([d, torch.tensor([[0.0, 0.6, 0.8], [0.6, 0.8, 0.0]])])
        near, far = near_far_from_bound(o[None], d[None], bound, type="cube")
        out[f"o_b{bound}"], out[f"d_b{bound}"] = o, d
        out[f"near_b{bound}"], out[f"far_b{bound}"] = near.reshape(-1), far.reshape(-1)
    save("ref_near_far_from_bound", **out)


def gold_binding_signatures():
    """Argument kinds and names, in order, of the 20 functions the reference binds (raymarching/src/raymarching.h:7-19,
    gridencoder/src/gridencoder.h:12-13, shencoder/src/shencoder.h:9,12, ffmlp/src/ffmlp.h:8-14), parsed from those
    headers at mint time.  Data only: {module: {function: [[kind, name], ...]}}."""
    import json
    import re
    headers = {"_raymarching": "raymarching/src/raymarching.h", "_gridencoder": "gridencoder/src/gridencoder.h",
               "_shencoder": "shencoder/src/shencoder.h", "_ffmlp": "ffmlp/src/ffmlp.h"}
    kinds = {"at::Tensor": "Tensor", "uint32_t": "int", "size_t": "int", "float": "float", "bool": "bool"}
    out = {}
    for mod, rel in headers.items():
        text = open(os.path.join(ref_import.REFERENCE, rel)).read()
        text = re.sub(r"//[^\n]*", "", text)
        fns = {}
        for m in re.finditer(r"\bvoid\s+(\w+)\s*\(([^)]*)\)\s*;", text):
            params = []
            for a in filter(None, (x.strip() for x in m.group(2).split(","))):
                toks = a.replace("const", "").split()
                params.append([kinds[toks[0]], toks[1]])
            fns[m.group(1)] = params
        out[mod] = fns
    assert sum(len(v) for v in out.values()) == 20, {k: len(v) for k, v in out.items()}
    with open(os.path.join(OUT, "ref_binding_signatures.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("  wrote ref_binding_signatures.json", {k: len(v) for k, v in out.items()})


def gold_state_dict_schema():
    """state_dict layout (key -> shape, dtype) of the reference's two network classes with cuda_ray on, at the bounds
    of the BASELINE configs: what a reference `.pth` checkpoint's 'model' entry looks like (nerf/utils.py
    save_checkpoint stores model.state_dict() plus mean_count / mean_density when cuda_ray)."""
    import json
    schema = {}
    for mod, name in (("nerf.network", "network"), ("nerf.network_ff", "network_ff")):
        cls = __import__(mod, fromlist=["NeRFNetwork"]).NeRFNetwork
        for bound in (1, 2, 3):
            kw = dict(encoding="hashgrid", bound=bound, cuda_ray=True)
            if name == "network":
                kw["out_dim_color"] = 3
            model = cls(**kw)
            schema[f"{name}_bound{bound}"] = {k: [list(v.shape), str(v.dtype)] for k, v in model.state_dict().items()}
    with open(os.path.join(OUT, "ref_state_dict_schema.json"), "w") as f:
        json.dump(schema, f, indent=1, sort_keys=True)
    print("  wrote ref_state_dict_schema.json", {k: len(v) for k, v in schema.items()})


def gold_config0():
    """BASELINE configs[0]: configs/spiral1 shape on the PyTorch sampler -- nerf/network.py with frequency encodings for
    position and direction (encoding.py:5-43,54-55), cuda_ray off, 256 rays x 512 stratified samples, out_dim_color 1,
    bound 3, lr 0.005 (configs/spiral1/spiral1_enerf.txt), NeRFRenderer.run (nerf/renderer.py:150-278) + MSE + backward +
    Adam(betas=(0.9, 0.99), eps=1e-15) (main_nerf.py:211) for three steps, jitter on (torch's host generator, re-seeded
    per step).  Stored: rays, targets, the first step's image, the three losses, and a few parameters after the steps."""
    from nerf.network import NeRFNetwork
    model = NeRFNetwork(encoding="frequency", encoding_dir="frequency", bound=3, cuda_ray=False, out_dim_color=1)
    det_fill_(list(model.parameters()), 91, -0.25, 0.25)
    opt = torch.optim.Adam(model.get_params(0.005), betas=(0.9, 0.99), eps=1e-15)
    o, d = _rays(256, 92, 3)
    target = torch.rand(1, 256, 1, generator=torch.Generator().manual_seed(93))
    model.train()
    losses, image0 = [], None
    for it in range(3):
        torch.manual_seed(500 + it)
        opt.zero_grad(set_to_none=True)
        out = model.render(o, d, staged=False, bg_color=None, perturb=True, num_steps=512, upsample_steps=0,
                           out_dim_color=1)
        loss = torch.nn.functional.mse_loss(out["image"], target)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
        if it == 0:
            image0, depth0 = out["image"].detach().clone(), out["depth"].detach().clone()
    sd = model.state_dict()
    save("ref_config0_steps", rays_o=o, rays_d=d, target=target, image0=image0, depth0=depth0,
         losses=torch.stack(losses), in_dim=np.int64(model.in_dim), in_dim_dir=np.int64(model.in_dim_dir),
         **{"p_" + k.replace(".", "_"): v for k, v in sd.items() if k.endswith(".weight")})


def gold_checkpoint():
    """A checkpoint written by the reference's own Trainer.save_checkpoint(full=True) (nerf/utils.py:1295-1351) for a
    small model (frequency encodings: no hash table; cuda_ray on, so the dict carries mean_count / mean_density and the
    state_dict the occupancy buffers), with a LambdaLR schedule as main_nerf.py:212 builds it, after three optimizer
    steps; then one more step on the reference side, whose result a resumed run must reproduce.  Stored: the .pth
    itself (gzip: the 8 MB density grid is almost all zeros) and the after-resume parameters."""
    import gzip
    import io
    import tempfile
    from nerf.network import NeRFNetwork
    from nerf.utils import Trainer
    model = NeRFNetwork(encoding="frequency", encoding_dir="frequency", bound=1, cuda_ray=True, out_dim_color=3)
    det_fill_(list(model.parameters()), 95, -0.25, 0.25)
    g = torch.Generator().manual_seed(96)
    idx = torch.randint(0, model.density_grid.numel(), (500,), generator=g)
    model.density_grid.view(-1)[idx] = torch.rand(500, generator=g) * 20
    model.density_bitfield.view(-1)[idx // 8] = 255
    model.step_counter[:3] = torch.tensor([[1200, 64], [1100, 64], [1300, 64]], dtype=torch.int32)
    model.mean_count, model.mean_density, model.iter_density, model.local_step = 1200, 0.37, 3, 3
    t = Trainer.__new__(Trainer)
    t.name, t.model, t.ema, t.epoch, t.global_step, t.max_keep_ckpt = "ngp", model, None, 2, 3, 2
    t.stats = {"loss": [0.5, 0.25], "valid_loss": [], "results": [], "checkpoints": [], "best_result": None}
    t.optimizer = torch.optim.Adam(model.get_params(0.01), betas=(0.9, 0.99), eps=1e-15)
    t.lr_scheduler = torch.optim.lr_scheduler.LambdaLR(t.optimizer, lambda it: 0.1 ** min(it / 10, 1))
    t.scaler = torch.cuda.amp.GradScaler(enabled=False)
    x, d = pts(64, 97), pts(64, 98)

    def step():
        t.optimizer.zero_grad(set_to_none=True)
        sigma, color = model(x, d)
        (sigma.mean() + (color ** 2).mean()).backward()
        t.optimizer.step()
        t.lr_scheduler.step()
    for _ in range(3):
        step()
    with tempfile.TemporaryDirectory() as tmp:
        t.ckpt_path = tmp
        t.save_checkpoint(name="ngp_ep0002", full=True, remove_old=False)
        raw = open(os.path.join(tmp, "ngp_ep0002.pth"), "rb").read()
    with gzip.open(os.path.join(OUT, "ref_checkpoint_freq.pth.gz"), "wb", compresslevel=9) as f:
        f.write(raw)
    print(f"  wrote ref_checkpoint_freq.pth.gz ({len(raw)} B raw)")
    step()
    save("ref_checkpoint_resumed", x=x, d=d, lr_after=np.float64(t.optimizer.param_groups[0]["lr"]),
         **{"p_" + k.replace(".", "_"): v for k, v in model.state_dict().items() if k.endswith(".weight")})


def _summary(t):
    """A large state tensor as data small enough to keep: sha256 of its bytes, sum, and a strided sample."""
    import hashlib
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    flat = a.reshape(-1)
    return {"sha256": np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8),
            "sum": np.float64(flat.astype(np.float64).sum()), "sample": flat[:: max(1, flat.size // 4096)][:4096].copy()}


def gold_cuda_ray():
    """The reference's cuda_ray path END TO END in its own Python: NeRFRenderer.mark_untrained_grid, update_extra_state
    (full sweep and partial update), run_cuda in training (forward + backward through its raymarching autograd Functions)
    and the inference round loop -- nerf/renderer.py:281-560 and raymarching/raymarching.py, BOTH the reference's files,
    executed on CPU: `_raymarching` is the C oracle behind the reference's binding signatures (oracle/backend.py) and the
    wrappers' unconditional `.cuda()` moves are made no-ops for the duration of this function (torch.Tensor.cuda patched,
    nothing in /root/reference is touched).  What the fixture pins: enerf_amd's restatement of that Python -- renderer,
    sampler, the plain-tensor density update, the ten raymarching wrappers -- driven the same way over the same oracle
    (tests/test_host_cuda_ray_vs_reference.py), and through it the device-side passes the GPU tests compare with that route."""
    from . import backend as ob
    keep_rm = sys.modules.pop("raymarching", None)
    keep_cuda = torch.Tensor.cuda
    sys.modules["_raymarching"] = ob.as_module("_raymarching", ob.raymarching_backend)
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        import importlib
        import raymarching
        assert raymarching.__file__.startswith(ref_import.REFERENCE), raymarching.__file__
        import nerf.renderer as rr
        importlib.reload(rr)                               # bind the real package in place of the facade
        import nerf.network as rn
        importlib.reload(rn)
        torch.manual_seed(0)
        model = rn.NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3)
        det_fill_([p for n, p in model.named_parameters() if "embeddings" not in n], 71, -0.35, 0.35)
        det_fill_([model.encoder.embeddings], 72, -1.0, 1.0)
        z = {}
        # --- mark_untrained_grid: three cameras looking at the origin
        poses = []
        for k, (ax, ay) in enumerate(((0.0, 0.0), (0.6, 0.3), (-0.5, 0.9))):
            cz, sz = np.cos(ax), np.sin(ax); cy, sy = np.cos(ay), np.sin(ay)
            R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cz, -sz], [0, sz, cz]])
            T = np.eye(4, dtype=np.float32); T[:3, :3] = R; T[:3, 3] = R @ np.array([0, 0, -2.5 + 0.4 * k])
            poses.append(T)
        poses = np.stack(poses).astype(np.float32)
        intrinsic = np.array([60.0, 60.0, 32.0, 24.0], np.float32)
        model.mark_untrained_grid(poses, intrinsic)
        z["poses"], z["intrinsic"] = poses, intrinsic
        z["untrained_count"] = np.int64((model.density_grid == -1).sum())
        for k, v in _summary(model.density_grid).items():
            z["untrained_grid_" + k] = v
        # --- update_extra_state: two full sweeps, then a partial update; the random draws come from torch's global CPU stream
        model.train()
        torch.manual_seed(123)
        threads = torch.get_num_threads()
        for tag in ("full1", "full2", "partial"):
            if tag == "partial":
                model.iter_density = 16
                # `tmp_grid[cas, indices] = sigmas` with repeated indices (cells drawn twice): which write stays depends on
                # how index_put_ splits the work over threads (and is undefined on a GPU); one thread = the last one
                torch.set_num_threads(1)
            model.local_step = 3
            model.step_counter.zero_()
            model.step_counter[:3, 0] = torch.tensor([1000, 1200, 1100], dtype=torch.int32)
            model.update_extra_state()
            for k, v in _summary(model.density_grid).items():
                z[f"{tag}_grid_{k}"] = v
            for k, v in _summary(model.density_bitfield).items():
                z[f"{tag}_bits_{k}"] = v
            z[f"{tag}_mean_density"] = np.float64(model.mean_density)
            z[f"{tag}_mean_count"] = np.int64(model.mean_count)
            z[f"{tag}_iter_density"] = np.int64(model.iter_density)
        torch.set_num_threads(threads)
        # --- run_cuda, training: two steps (the second one takes the first one's slot of the step counter ring)
        o, d = _rays(40, 73, 2)
        z["rays_o"], z["rays_d"] = o, d
        for step, (perturb, force, gamma) in enumerate(((True, False, 0.0), (False, True, 1.0 / 256))):
            model.zero_grad()
            out = model.render(o, d, staged=False, bg_color=torch.full((3,), 0.25), perturb=perturb, force_all_rays=force,
                               dt_gamma=gamma, max_steps=256)
            loss = (out["image"] ** 2).sum() + 0.1 * out["depth"].sum()
            loss.backward()
            z[f"train{step}_image"], z[f"train{step}_depth"] = out["image"], out["depth"]
            z[f"train{step}_g_sigma0"] = model.sigma_net[0].weight.grad.clone()
            z[f"train{step}_g_color2"] = model.color_net[2].weight.grad.clone()
            g = model.encoder.embeddings.grad
            z[f"train{step}_g_emb_abs_sum"] = np.float64(g.abs().double().sum())
            z[f"train{step}_g_emb_l0"] = g[:4920].clone()
            z[f"train{step}_step_counter"] = model.step_counter[:4].clone()
            z[f"train{step}_local_step"] = np.int64(model.local_step)
        # --- Trainer.train_step_events (nerf/utils.py:482-573) on this model: two event renders + the frame render, luma /
        # lin-log / C_thres 0.2; its background is drawn from torch's stream
        import argparse as ap
        import nerf.utils as ru
        importlib.reload(ru)
        t = ru.Trainer.__new__(ru.Trainer)
        t.device = torch.device("cpu")
        t.out_dim_color = 3
        t.use_luma, t.linlog, t.C_thres, t.event_only = 1, 1, 0.2, 0
        t.log_implicit_C_thres = False
        t.negative_event_sampling = False
        t.weight_loss_rgb = 1.0
        t.epoch, t.epoch_start_noEvLoss = 1, 0
        t.criterion = torch.nn.MSELoss(reduction="none")
        t.opt = ap.Namespace()
        t.model = model
        o1, d1 = _rays(32, 74, 2)
        o2, d2 = o1 + 0.02, torch.nn.functional.normalize(d1 + 0.015, dim=-1)
        of, df = _rays(32, 75, 2)
        g = torch.Generator().manual_seed(76)
        data = {"images": torch.rand(1, 32, 3, generator=g), "rays_evs_o1": o1, "rays_evs_d1": d1, "rays_evs_o2": o2,
                "rays_evs_d2": d2, "pols": torch.sign(torch.rand(1, 32, generator=g) - 0.5), "rays_o": of, "rays_d": df}
        model.zero_grad()
        torch.manual_seed(321)
        delta, gt_pol, loss, _, losses = t.train_step_events(data)
        loss.backward()
        for k, v in data.items():
            z["ev_" + k] = v
        z["ev_loss"], z["ev_delta"] = loss, delta
        z["ev_loss_evs"], z["ev_loss_frames"] = losses["loss_evs"], losses["loss_frames"]
        z["ev_g_sigma0"] = model.sigma_net[0].weight.grad.clone()
        z["ev_g_color2"] = model.color_net[2].weight.grad.clone()
        z["ev_g_emb_abs_sum"] = np.float64(model.encoder.embeddings.grad.abs().double().sum())
        z["ev_g_emb_l0"] = model.encoder.embeddings.grad[:4920].clone()
        z["ev_step_counter"] = model.step_counter[:6].clone()
        z["ev_local_step"] = np.int64(model.local_step)
        # --- run_cuda, inference: the round loop (march_rays / composite_rays / compact_rays)
        model.eval()
        with torch.no_grad():
            for tag, gamma in (("infer", 0.0), ("infer_gamma", 1.0 / 128)):
                out = model.render(o, d, staged=False, bg_color=None, perturb=False, dt_gamma=gamma, max_steps=256)
                z[f"{tag}_image"], z[f"{tag}_depth"] = out["image"], out["depth"]
        save("ref_cuda_ray", **z)
    finally:
        torch.Tensor.cuda = keep_cuda
        sys.modules.pop("_raymarching", None)
        sys.modules.pop("raymarching", None)
        if keep_rm is not None:
            sys.modules["raymarching"] = keep_rm
        import importlib
        import nerf.renderer as rr
        importlib.reload(rr)
        import nerf.network as rn
        importlib.reload(rn)
        import nerf.utils as ru
        importlib.reload(ru)


def gold_cuda_ray_ff():
    """nerf/network_ff.py (hash grid + SH + two FFMLP nets) on the cuda_ray path of the reference's own renderer.py /
    raymarching.py, on CPU over the oracle (as gold_cuda_ray; `_ffmlp` is the oracle's rounded-half FFMLP behind the
    reference's ffmlp.py): one update_extra_state, a jittered training render with backward, an inference render."""
    from . import backend as ob
    keep_rm = sys.modules.pop("raymarching", None)
    keep_cuda = torch.Tensor.cuda
    sys.modules["_raymarching"] = ob.as_module("_raymarching", ob.raymarching_backend)
    torch.Tensor.cuda = lambda self, *a, **k: self
    import importlib
    try:
        import raymarching
        assert raymarching.__file__.startswith(ref_import.REFERENCE), raymarching.__file__
        import nerf.renderer as rr
        importlib.reload(rr)
        import nerf.network_ff as rn
        importlib.reload(rn)
        torch.manual_seed(0)
        model = rn.NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True)
        det_fill_([model.encoder.embeddings], 121, -1.0, 1.0)
        det_fill_([model.sigma_net.weights], 122, -0.3, 0.3)
        det_fill_([model.color_net.weights], 123, -0.3, 0.3)
        z = {}
        model.train()
        torch.manual_seed(124)
        model.update_extra_state()
        for k, v in _summary(model.density_bitfield).items():
            z["bits_" + k] = v
        z["mean_density"] = np.float64(model.mean_density)
        o, d = _rays(32, 125, 2)
        z["rays_o"], z["rays_d"] = o, d
        model.zero_grad()
        out = model.render(o, d, staged=False, bg_color=torch.full((3,), 0.25), perturb=True, force_all_rays=True,
                           max_steps=128)
        loss = (out["image"].float() ** 2).sum() + 0.1 * out["depth"].float().sum()
        loss.backward()
        z["train_image"], z["train_depth"] = out["image"].float(), out["depth"].float()
        z["g_sigma_w"] = model.sigma_net.weights.grad.float().clone()
        z["g_color_w"] = model.color_net.weights.grad.float().clone()
        z["g_emb_abs_sum"] = np.float64(model.encoder.embeddings.grad.abs().double().sum())
        z["g_emb_l0"] = model.encoder.embeddings.grad[:4920].float().clone()
        z["step_counter"] = model.step_counter[:2].clone()
        model.eval()
        with torch.no_grad():
            out = model.render(o, d, staged=False, bg_color=None, perturb=False, max_steps=128)
        z["infer_image"], z["infer_depth"] = out["image"].float(), out["depth"].float()
        save("ref_cuda_ray_ff", **z)
    finally:
        torch.Tensor.cuda = keep_cuda
        sys.modules.pop("_raymarching", None)
        sys.modules.pop("raymarching", None)
        if keep_rm is not None:
            sys.modules["raymarching"] = keep_rm
        import nerf.renderer as rr
        importlib.reload(rr)
        import nerf.network_ff as rn
        importlib.reload(rn)


def gold_train_epoch():
    """The reference's OWN training loop -- Trainer.train_one_epoch (nerf/utils.py:920-1015): update_extra_state every 16
    global steps, zero_grad, train_step_events (two run_cuda renders), GradScaler (disabled: fp32), Adam(betas=(0.9, 0.99),
    eps=1e-15) (main_nerf.py:211), LambdaLR stepped every step -- for 18 steps of event training on a cuda_ray hash-grid
    model, executed on CPU over the C oracle as gold_cuda_ray does (the reference's renderer.py and raymarching.py).  Stored:
    the data of every step, every step's loss, the learning rates, the sample budget and counters at the end, slices of the
    parameters after the epoch.  The Trainer object is made with __new__ and given what the loop reads."""
    from . import backend as ob
    keep_rm = sys.modules.pop("raymarching", None)
    keep_cuda = torch.Tensor.cuda
    sys.modules["_raymarching"] = ob.as_module("_raymarching", ob.raymarching_backend)
    torch.Tensor.cuda = lambda self, *a, **k: self
    import importlib
    try:
        import raymarching
        assert raymarching.__file__.startswith(ref_import.REFERENCE), raymarching.__file__
        import nerf.renderer as rr
        importlib.reload(rr)
        import nerf.network as rn
        importlib.reload(rn)
        import nerf.utils as ru
        importlib.reload(ru)
        import argparse as ap
        torch.manual_seed(0)
        model = rn.NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3)
        det_fill_([p for n, p in model.named_parameters() if "embeddings" not in n], 101, -0.35, 0.35)
        det_fill_([model.encoder.embeddings], 102, -0.5, 0.5)
        steps, N = 18, 24
        g = torch.Generator().manual_seed(103)
        batches = []
        for i in range(steps):
            o1, d1 = _rays(N, 200 + i, 2)
            batches.append({"images": torch.rand(1, N, 3, generator=g), "rays_evs_o1": o1, "rays_evs_d1": d1,
                            "rays_evs_o2": o1 + 0.02, "rays_evs_d2": torch.nn.functional.normalize(d1 + 0.015, dim=-1),
                            "pols": torch.sign(torch.rand(1, N, generator=g) - 0.5), "rays_o": o1, "rays_d": d1})

        class Loader(list):
            batch_size = 1
        t = ru.Trainer.__new__(ru.Trainer)
        t.log = lambda *a, **k: None
        t.model, t.device = model, torch.device("cpu")
        t.optimizer = torch.optim.Adam(model.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
        t.lr_scheduler = torch.optim.lr_scheduler.LambdaLR(t.optimizer, lambda it: 0.1 ** min(it / 30, 1))
        t.scheduler_update_every_step = True
        t.scaler = torch.cuda.amp.GradScaler(enabled=False)
        t.fp16 = False
        t.ema = None
        t.epoch, t.global_step, t.local_rank, t.world_size = 1, 0, 0, 1
        t.report_metric_at_train = False
        t.use_tensorboardX = False
        t.eval_interval = 0
        t.stats = {"loss": []}
        t.use_events = True
        t.out_dim_color = 3
        t.use_luma, t.linlog, t.C_thres, t.event_only = 1, 1, 0.2, 1
        t.log_implicit_C_thres = False
        t.negative_event_sampling = False
        t.weight_loss_rgb = 1.0
        t.epoch_start_noEvLoss = 0
        t.criterion = torch.nn.MSELoss(reduction="none")
        t.opt = ap.Namespace()
        losses, lrs = [], []
        inner = t.train_step_events

        def recording(data):
            out = inner(data)
            losses.append(out[2].detach().clone())
            lrs.append(t.optimizer.param_groups[0]["lr"])
            return out
        t.train_step_events = recording
        torch.manual_seed(777)
        t.train_one_epoch(Loader(batches))
        z = {"steps": np.int64(steps), "losses": torch.stack(losses), "lrs": np.asarray(lrs, np.float64),
             "final_lr": np.float64(t.optimizer.param_groups[0]["lr"]), "mean_count": np.int64(model.mean_count),
             "iter_density": np.int64(model.iter_density), "model_local_step": np.int64(model.local_step),
             "step_counter": model.step_counter.clone(), "mean_density": np.float64(model.mean_density),
             "epoch_loss": np.float64(t.stats["loss"][0])}
        for i, b in enumerate(batches):
            for k in ("images", "rays_evs_o1", "rays_evs_d1", "pols"):
                z[f"b{i}_{k}"] = b[k]
        sd = model.state_dict()
        z["p_sigma0"] = sd["sigma_net.0.weight"]
        z["p_color2"] = sd["color_net.2.weight"]
        z["p_emb_l0"] = sd["encoder.embeddings"][:4920]
        for k, v in _summary(model.density_bitfield).items():
            z["bits_" + k] = v
        save("ref_train_epoch", **z)
    finally:
        torch.Tensor.cuda = keep_cuda
        sys.modules.pop("_raymarching", None)
        sys.modules.pop("raymarching", None)
        if keep_rm is not None:
            sys.modules["raymarching"] = keep_rm
        import nerf.renderer as rr
        importlib.reload(rr)
        import nerf.network as rn
        importlib.reload(rn)
        import nerf.utils as ru
        importlib.reload(ru)


def gold_event_readers():
    """The reference's event readers run on containers made here: EventSlicer (utils/event_utils.py:223-383) over a dict
    that answers like the h5 file it expects ('events/{p,x,y,t}', 'ms_to_idx', 't_offset'), its millisecond index from the
    reference's compute_ms_to_idx (:389-408), windows incl. the edge cases; and load_contiguous_evs_batches_esim_ns
    (nerf/provider.py:27-82) over a directory of .npy event files written to /tmp."""
    import tempfile
    from utils.event_utils import EventSlicer, compute_ms_to_idx
    import nerf.provider as rp
    rng = np.random.default_rng(111)
    n = 4000
    t = np.sort(rng.integers(0, 60_000, n)).astype(np.int64)          # microseconds: duplicates, empty milliseconds
    t[1000:1040] = t[1000]                                             # a run of equal stamps
    t = np.sort(t)
    x, y = rng.integers(0, 64, n).astype(np.int16), rng.integers(0, 48, n).astype(np.int16)
    p = rng.integers(0, 2, n).astype(np.int8)
    ms_to_idx = compute_ms_to_idx(t * 1000)                            # the function takes nanoseconds
    z = {"t_us": t, "x": x, "y": y, "p": p, "ms_to_idx": ms_to_idx}
    for tag, off in (("plain", 0), ("offset", 1_234_567)):
        h5 = {"events/p": p, "events/x": x, "events/y": y, "events/t": t, "ms_to_idx": ms_to_idx}
        if off:
            h5["t_offset"] = np.array(off)
        sl = EventSlicer(h5)
        z[f"{tag}_t_final"] = np.int64(sl.get_final_time_us())
        wins = [(0, 1), (0, 1000), (999, 1001), (1500, 4321), (int(t[1000]), int(t[1000]) + 1), (int(t[1000]) - 1, int(t[1000])),
                (30_000, 30_500), (58_000, 59_000), (59_000, 60_000), (59_500, 61_000), (10, 59_999)]
        wins += [tuple(sorted(rng.integers(0, 59_000, 2).tolist())) for _ in range(24)]
        wins = [(a + off, b + off) for a, b in wins if a < b]
        res = []
        for a, b in wins:
            ev = sl.get_events(a, b)
            if ev is None:
                res.append((-1, -1, -1, -1))
            else:
                res.append((ev["t"].size, int(ev["t"][0]) if ev["t"].size else -1, int(ev["t"][-1]) if ev["t"].size else -1,
                            int(ev["x"].astype(np.int64).sum() + 7 * ev["y"].astype(np.int64).sum() + 13 * ev["p"].astype(np.int64).sum())))
        z[f"{tag}_windows"] = np.asarray(wins, np.int64)
        z[f"{tag}_results"] = np.asarray(res, np.int64)
    # esim event directories
    with tempfile.TemporaryDirectory(prefix="enerf_esim_", dir="/tmp") as d:
        files = []
        t0 = 0
        for k in range(7):
            m = int(rng.integers(20, 60))
            ts = np.sort(rng.integers(t0, t0 + 10_000_000, m)).astype(np.float64)
            t0 += 10_000_000
            # a fifth column the loader must drop; polarities -1 / +1 (the reference's own {0, 1} -> {-1, +1} mapping
            # multiplies four-column batches by a five-entry mask, utils/event_utils.py:144-145, and cannot run)
            ev = np.stack([rng.integers(0, 64, m), rng.integers(0, 48, m), ts, rng.integers(0, 2, m) * 2 - 1,
                           rng.integers(0, 9, m)], axis=1).astype(np.float64)
            np.save(os.path.join(d, f"{k:06d}.npy"), ev)
            files.append(ev)
        for tag, idxs in (("esim_a", [0, 2, 3, 6]), ("esim_b", [1, 4]), ("esim_c", [5])):
            out = rp.load_contiguous_evs_batches_esim_ns(d, idxs, hwf=(48, 64, 1.0))
            z[f"{tag}_idxs"] = np.asarray(idxs, np.int64)
            z[f"{tag}_sizes"] = np.asarray([len(b) for b in out], np.int64)
            z[f"{tag}_cat"] = np.concatenate([np.asarray(b, np.float64) for b in out])
        for k, ev in enumerate(files):
            z[f"esim_file{k}"] = ev
    save("ref_event_readers", **z)


def gold_collate():
    """EventNeRFDataset -- the reference's own class (nerf/provider.py:1105-1500) -- CONSTRUCTED and collated here.  What is
    stubbed is its input/output only: the parent's __init__ (image folders, pose files: :430-700) is replaced by one that
    sets the attributes it would leave behind, `load_event_data_esim` (the .npy reader) hands over event batches made
    here, the pose plot is a no-op.  Everything else is the reference's code: load_events_at_frame_idxs' no-event tables
    (:1283-1351), the constructor's per-pixel grouping loop (:1147-1199), the interpolators, and collate (:1364-1480) --
    successor filter, random window end, polarity sum, the un-accumulated variant, scipy's Slerp / cubic pose interpolation
    at the event times, get_event_rays, the no-event entries.  numpy's global draws are recorded as they are made, so that
    the restatement can be fed the same."""
    import argparse as ap
    from scipy.spatial.transform import Rotation as R
    import nerf.provider as rp
    rng = np.random.default_rng(81)
    Hs, Ws, n = 12, 16, 900
    ev = np.stack([rng.integers(0, Ws, n), rng.integers(0, Hs, n), np.sort(rng.uniform(1e6, 9e7, n)),
                   rng.choice([-1.0, 1.0], n)], axis=1).astype(np.float64)
    ev2 = ev.copy()
    ev2[:, 2] += 9e7                                                     # a second batch: only its first stamp is used (:1270)
    K = 24
    ts = np.linspace(0.0, 2e8, K)
    rots = R.from_euler("xyz", np.stack([0.3 * np.sin(np.arange(K) * 0.4), 0.2 * np.cos(np.arange(K) * 0.3),
                                         0.05 * np.arange(K)], axis=1))
    trans = np.stack([0.1 * np.arange(K), np.sin(np.arange(K) * 0.5), 0.3 * np.cos(np.arange(K) * 0.2)], axis=1)
    poses_hf = []
    for k in range(K):
        T = np.zeros((3, 4)); T[:, :3] = rots[k].as_matrix(); T[:, 3] = trans[k]
        poses_hf.append({"ts_ns": ts[k], "pose_c2w": T})
    z = {"events": ev.astype(np.float32), "events_next_first_ns": np.float64(ev2[0, 2]), "pose_ts": ts,
         "pose_R": rots.as_matrix(), "pose_t": trans}
    frames = torch.from_numpy(rng.random((2, Hs, Ws, 3)).astype(np.float32))
    z["frame_images"] = frames

    def parent_init(self, opt, device, type="train", downscale=1, n_test=10, select_frames=None):
        self.opt, self.device, self.type, self.training = opt, device, type, True
        self.frame_idxs = np.asarray([7, 9])
        self.poses_hf = poses_hf
        self.workspace = "/tmp"
        self.images_corrupted = False
        self.negative_event_sampling = opt.negative_event_sampling
        self.acc_max_num_evs = opt.acc_max_num_evs
        self.precompute_evs_poses = opt.precompute_evs_poses
        self.H, self.W, self.H_ev, self.W_ev = Hs, Ws, Hs, Ws
        self.intrinsics = np.array([14.0, 13.0, 8.0, 6.0])
        self.intrinsics_evs = np.array([14.0, 13.0, 8.0, 6.0])
        self.poses = torch.eye(4).unsqueeze(0).repeat(2, 1, 1)
        self.images = frames
        self.error_map = None
        self.num_rays = 16
        self.hotpixs = None
    keep = (rp.NGPDataset.__init__, rp.load_event_data_esim, rp.plotting_poses_hf)
    rp.NGPDataset.__init__ = parent_init
    rp.load_event_data_esim = lambda path, idxs, hwf=None, img_folder="images": [ev.copy(), ev2.copy()]
    rp.plotting_poses_hf = lambda *a, **k: None
    np_keep = (np.random.randint, np.random.rand, np.random.choice, np.random.random)
    try:
        for tag, accumulate, acc_max, negative in (("acc", True, 0, False), ("acc_max3", True, 3, False),
                                                   ("single", False, 0, False), ("acc_noev", True, 0, True)):
            drawn = {"randint": [], "rand": [], "choice": [], "random": []}

            def rec(name, fn):
                def wrapped(*a, **k):
                    r = fn(*a, **k)
                    drawn[name].append(np.array(r, copy=True))
                    return r
                return wrapped
            np.random.randint, np.random.rand = rec("randint", np_keep[0]), rec("rand", np_keep[1])
            np.random.choice, np.random.random = rec("choice", np_keep[2]), rec("random", np_keep[3])
            opt = ap.Namespace(accumulate_evs=accumulate, batch_size_evs=64, out_dim_color=3, datadir="/nonexistent",
                               mode="esim", negative_event_sampling=negative, acc_max_num_evs=acc_max,
                               precompute_evs_poses=False)
            np.random.seed(80)
            ds = rp.EventNeRFDataset(opt, torch.device("cpu"))
            if tag == "acc":            # the tables the constructor built for frame 7 (the grouping loop, :1147-1199)
                z["tab_events"] = ds.events[7]
                z["tab_xy_numEvs_Idx"] = np.asarray(ds.xy_numEvs_Idx[7], np.int64)
                z["tab_idx_no_successor"] = np.asarray(ds.idx_no_successor[7], np.int64)
                z["tab_num_successor_evs"] = np.asarray(ds.num_successor_evs[7], np.int64)
                z["tab_num_evs"] = np.int64(ds.num_evs[7])
            if negative:                # the no-event tables of frame 7 (:1283-1351) and the choices that thinned them
                ne = ds.no_evs[7]
                z["noev_n_chunks"] = np.int64(ne["tss_bds"]["N_ev_chunks"][0])
                z["noev_start_us"] = np.asarray(ne["tss_bds"]["start_time_us"], np.float64)
                z["noev_end_us"] = np.asarray(ne["tss_bds"]["end_time_us"], np.float64)
                for j, c in enumerate(ne["coords"]):
                    z[f"noev_coords{j}"] = c
                nch = int(z["noev_n_chunks"])
                for j in range(nch):
                    z[f"noev_choice{j}"] = np.asarray(drawn["choice"][j], np.int64)
                for name in drawn:
                    drawn[name] = []
                drawn_ctor_done = True
            for name in drawn:
                drawn[name] = []
            np.random.seed(82)
            torch.manual_seed(83)
            out = ds.collate([0])
            for k in ("rays_evs_o1", "rays_evs_d1", "rays_evs_o2", "rays_evs_d2", "pols", "rays_o", "rays_d", "images"):
                z[f"{tag}_{k}"] = out[k]
            if negative:
                for k in ("rays_no_evs_o1", "rays_no_evs_d1", "rays_no_evs_o2", "rays_no_evs_d2"):
                    z[f"{tag}_{k}"] = out[k]
            for name, lst in drawn.items():
                if lst:
                    z[f"{tag}_draw_{name}_first"] = np.asarray(lst[0])
                    rest = [np.asarray(v).reshape(-1) for v in lst[1:]]
                    z[f"{tag}_draw_{name}_rest"] = np.concatenate(rest) if rest else np.zeros(0)
    finally:
        rp.NGPDataset.__init__, rp.load_event_data_esim, rp.plotting_poses_hf = keep
        np.random.randint, np.random.rand, np.random.choice, np.random.random = np_keep
    save("ref_collate", **z)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    if not sys.dont_write_bytecode:
        print("re-run with python -B", file=sys.stderr)
        sys.exit(2)
    ref_import.install()
    os.makedirs(OUT, exist_ok=True)
    jobs = [gold_grid_wrapper, gold_sh_wrapper, gold_ffmlp_wrapper, gold_network, gold_network_ff,
            gold_composite_vs_run, gold_events, gold_no_events, gold_misc, gold_sh_literals, gold_near_far_from_bound,
            gold_binding_signatures, gold_state_dict_schema, gold_config0, gold_checkpoint, gold_cuda_ray, gold_collate, gold_train_epoch, gold_event_readers, gold_cuda_ray_ff]
    for j in jobs:
        if a.only and a.only not in j.__name__:
            continue
        print(j.__name__)
        j()


if __name__ == "__main__":
    main()
