"""One autograd node for `NeRFRenderer.run` with upsample_steps = 0 on the MI355X fp32 path: the stratified sampler every
shipped config of the reference trains and evaluates with (`cuda_ray = False`; sampler.render_stratified is the statement).

    rays -> near / far, T depths, clamped points          k_strat_points (bit-equal with sampler.stratified_depths + _points)
         -> hash grid -> sigma MLP -> sigma, geo_feat      enerf_grid_encode_forward (level-major), enerf_mlp32_forward_p
         -> alpha, w, opacity, depth, mask counts          k_strat_weights
         -> compact list of the samples with w > 1e-4      torch.cumsum of the counts (on the device: the host never reads it)
         -> [0 | geo_feat | SH(d)] of the compact rows     k_strat_color_input
         -> colour MLP + sigmoid on the compact rows       enerf_mlp32_forward_p under enerf_mlp32_valid_rows
         -> image = sum w rgb + (1 - opacity) bg           k_strat_composite

The backward runs the same chain in reverse: k_strat_composite_bwd (d sigma of every sample, d rgb of the compact rows),
the colour MLP's backward on the compact rows, k_strat_scatter_geo (geo_feat gradient back to the sigma net's rows), the
sigma MLP's backward (trunc_exp folded in), the grid backward.  It returns the gradients of the network's own parameters,
like fused_network._FusedNeRF, so optimisers and the event loop see nothing new.

The fp16 regime: a model whose `mlp_precision` is 3 -- TrainHarness(fp16=True) sets it for its
steps; for evaluation set `model.mlp_precision = 3` and call `model.render` -- runs both nets on fp16 operands with fp32
accumulation (enerf_mlp32_precision 3), keeps the colour rows, rgb, d rgb and the colour net's input gradient in fp16
(enerf_stratified_*_ex with ENERF_F16, enerf_mlp32_io16), rounds the directions to fp16 before the SH basis, and keeps
points, weights, compositing, the hash table and its gradient in fp32.  Autocast is still refused: under autocast the
statement runs, as it does in the reference.

What the PyTorch statement does with host synchronisations (`mask.any()`, boolean indexing) happens here on the device, so
a forward + backward can be captured in a CUDA graph.  Anything this does not serve -- CPU tensors, autocast, FFMLP nets,
upsampling, view directions off, out_dim_color > 3 -- keeps the statement (sampler.py).  A background model (bg_radius > 0)
is served in fp32: sampler.render_stratified passes the per-ray colours of background.py's node as bg_color
(`background_model=True`), and the node here returns their gradient (1 - opacity) g_image; in the fp16 regime and under
autocast it keeps the statement.
"""
import numpy as np
import torch
from torch.autograd import Function

from . import _lib as L
from . import fused_network as _fn
from . import gridencoder as _ge
from .backends import _gridencoder as _gb
from .fused_mlp import pad32

ENABLED = True
# renders taken by this route (tests assert that the route was taken)
stats = {"calls": 0}
# tests: keep the last render's weights [N,T], per-ray mask counts [N], sigma net outputs [N*T,16], sigma [N*T], colour rows
# [cap,32] and rgb [cap,C] in `last` (device tensors, never read here; the compact rows beyond incl[-1] are padding)
KEEP_LAST = False
last = None


def refusals(model, rays_o, rays_d, upsample_steps=0, bg_color=None, out_dim_color=None, background_model=False):
    """Why this route does not serve the call (empty: it does).  `background_model`: the caller renders the model's own
    per-ray background (background.py) and passes it as bg_color: bg_radius > 0 is then no refusal, and the tensor may
    carry a gradient (the node returns d bg)."""
    why = []
    if not ENABLED:
        why.append("disabled")
    if not (rays_o.is_cuda and rays_d.is_cuda):
        why.append("cpu")
    if rays_o.dtype != torch.float32 or rays_d.dtype != torch.float32:
        why.append("dtype")
    if rays_o.requires_grad or rays_d.requires_grad:
        why.append("ray gradients")
    if upsample_steps > 0:
        why.append("upsample_steps")
    if getattr(model, "bg_radius", -1) > 0 and not background_model:
        why.append("bg_radius")
    if background_model and getattr(model, "__dict__", {}).get("mlp_precision") not in (None, 0):   # (network_cfg's [4])
        why.append("background model precision")        # (the background's node is fp32: the fp16 / bf16 regimes refuse)
    if torch.is_autocast_enabled():
        why.append("autocast")
    if getattr(model, "disable_view_direction", True):
        why.append("disable_view_direction")
    c = getattr(model, "out_dim_color", 0)
    if not 1 <= c <= 3 or (out_dim_color is not None and out_dim_color != c):
        why.append("out_dim_color")
    if _fn.kind_of(model) != "linear" or model.color_net[-1].weight.shape[0] != c:
        why.append("network")
    elif not _ge._supports_layout():
        why.append("grid backend")
    if _background_form(bg_color, rays_o, c, background_model) is None:
        why.append("bg_color")
    return why


def supported(model, rays_o, rays_d, upsample_steps=0, bg_color=None, out_dim_color=None, background_model=False):
    return not refusals(model, rays_o, rays_d, upsample_steps, bg_color, out_dim_color, background_model)


def _background_form(bg, rays_o, C, may_need_grad=False):
    """"const": None or a number; "shared": a tensor of C values; "per_ray": one row of C per ray; None: anything else."""
    if bg is None or isinstance(bg, (int, float)):
        return "const"
    if not isinstance(bg, torch.Tensor) or bg.dtype != torch.float32 or (bg.requires_grad and not may_need_grad) \
            or bg.dim() < 1 or bg.shape[-1] != C or bg.device != rays_o.device:
        return None
    n = rays_o.numel() // 3
    if bg.numel() == C:
        return "shared"
    if bg.numel() == n * C and tuple(bg.shape[:-1]) in (tuple(rays_o.shape[:-1]), (n,)):
        return "per_ray"
    return None


def _background(bg, rays_o, N, C):
    """-> (bg as a contiguous [C] or [N, C] fp32 tensor, per_ray flag)"""
    form = _background_form(bg, rays_o, C, True)
    if form == "const":
        return torch.full((C,), 1.0 if bg is None else float(bg), dtype=torch.float32, device=rays_o.device), 0
    if form == "shared":
        return bg.reshape(C).contiguous(), 0
    return bg.reshape(N, C).contiguous(), 1


def render(model, rays_o, rays_d, num_steps, bg_color=None, perturb=False):
    """sampler.render_stratified for upsample_steps = 0 -> {"depth": [...], "image": [..., out_dim_color]}."""
    lead = rays_o.shape[:-1]
    ro = rays_o.contiguous().view(-1, 3)
    rd = rays_d.contiguous().view(-1, 3)
    N, T, C = ro.shape[0], int(num_steps), int(model.out_dim_color)
    dev = ro.device
    aabb = (model.aabb_train if model.training else model.aabb_infer).contiguous()
    # the jitter draws torch's stream exactly as sampler.stratified_depths does
    u = torch.rand((N, T), device=dev) if perturb else None
    bg, per_ray = _background(bg_color, rays_o, N, C)
    params = _fn.network_params(model)
    train = torch.is_grad_enabled() and (any(p.requires_grad for p in params) or bg.requires_grad)
    cfg = _fn.network_cfg(model)
    geo = dict(T=T, C=C, min_near=float(model.min_near), density_scale=float(model.density_scale), cfg=cfg)
    image, depth = _StratifiedRender.apply(ro, rd, u, bg, per_ray, aabb, geo, train, params[0],
                                           _fn.encoder_offsets(model), *params[1:])
    stats["calls"] += 1
    return {"depth": depth.view(*lead), "image": image.view(*lead, C)}


def _f32(x):
    return float(np.float32(x))


def render_forward(ro, rd, u, bg, per_ray, aabb, geo, train, embeddings, offsets, *weights):
    """The kernel sequence (no autograd) -> image [N,C], depth [N], and what the backward needs (None unless `train`)."""
    global last
    N, T, C = ro.shape[0], geo["T"], geo["C"]
    bound, per_level_scale, base_resolution, gridtype = geo["cfg"][:4]
    prec = geo["cfg"][4]
    dev = ro.device
    f32 = dict(dtype=torch.float32, device=dev)
    image = torch.empty(N, C, **f32)
    depth = torch.empty(N, **f32)
    if N == 0:
        return image, depth, None
    lib = L.lib()
    stream = L.stream_handle()
    B = N * T
    Bp = pad32(B)
    # host-rounded constants, as torch forms them: linspace's step (end - start) / (T - 1) and the reciprocal by which a
    # tensor is divided by a Python number
    lin_step = float(np.float32(1.0) / np.float32(T - 1)) if T > 1 else 0.0
    inv_T = float(np.float32(1.0) / np.float32(T))
    s_dens = geo["density_scale"]

    nears, fars = torch.empty(N, **f32), torch.empty(N, **f32)
    z = torch.empty(N, T, **f32)
    xyz = torch.empty(B, 3, **f32)
    L.check(lib.enerf_stratified_points(ro.data_ptr(), rd.data_ptr(), aabb.data_ptr(), N, T, geo["min_near"], lin_step,
                                        inv_T, u.data_ptr() if u is not None else None, nears.data_ptr(),
                                        fars.data_ptr(), z.data_ptr(), xyz.data_ptr(), stream), "stratified_points")

    # density: the grid in level-major order, the sigma net's 16 outputs [h0 | geo_feat] and sigma = exp(h0)
    S = float(np.log2(per_level_scale))
    affine = (float(bound), _f32(np.float32(1.0) / np.float32(2 * bound)))
    emb = embeddings.contiguous()
    feats = torch.empty(16, Bp, 2, **f32)
    _gb.grid_encode_forward(xyz, emb, offsets, feats, B, 3, 2, 16, S, base_resolution, False, feats, gridtype, layout=2,
                            affine=affine)
    seg_s, seg_c = _fn._weight_segments("linear", weights)
    h16 = torch.empty(B, 16, **f32)
    sigma = torch.empty(B, **f32)
    fb_s = torch.empty(1, Bp, 64, **f32) if train else None
    with _fn._precision(prec):
        L.check(lib.enerf_mlp32_forward_p(feats.data_ptr(), seg_s, 32, 0, B, 32, 16, 1, 0, 6,
                                          fb_s.data_ptr() if train else None, h16.data_ptr(), 1, 16, sigma.data_ptr(),
                                          None, stream), "mlp32_forward_p(sigma)")

    w = torch.empty(N, T, **f32)
    opacity = torch.empty(N, **f32)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    L.check(lib.enerf_stratified_weights(z.data_ptr(), sigma.data_ptr(), nears.data_ptr(), fars.data_ptr(), N, T, inv_T,
                                         s_dens, w.data_ptr(), opacity.data_ptr(), depth.data_ptr(), count.data_ptr(),
                                         stream), "stratified_weights")
    incl = torch.cumsum(count, 0, dtype=torch.int32)         # compact-list offsets; incl[N-1] = its length
    total_ptr = incl.data_ptr() + 4 * (N - 1)

    # colour on the compact rows only: capacity N*T, the MLP kernels stop at the device count's last 32-row tile
    # (fp16 regime: the colour rows, rgb and their gradients in half -- 64 B instead of 128 B per masked sample)
    f16 = prec == 3
    store, cdt = (L.F16, torch.float16) if f16 else (L.F32, torch.float32)
    cap = B
    capp = pad32(cap)
    cin = torch.empty(capp, 32, dtype=cdt, device=dev)
    L.check(lib.enerf_stratified_color_input_ex(w.data_ptr(), incl.data_ptr(), count.data_ptr(), h16.data_ptr(),
                                                rd.data_ptr(), N, T, cap, cin.data_ptr(), store, stream),
            "stratified_color_input")
    rgb = torch.empty(capp, C, dtype=cdt, device=dev)
    fb_c = torch.empty(2, capp, 64, **f32) if train and not f16 else None
    lib.enerf_mlp32_valid_rows(total_ptr)
    lib.enerf_mlp32_io16(1 if f16 else 0)
    try:
        with _fn._precision(prec):
            L.check(lib.enerf_mlp32_forward_p(cin.data_ptr(), seg_c, 31, 1, cap, 32, C, 2, 0, 3,
                                              fb_c.data_ptr() if fb_c is not None else None, rgb.data_ptr(), 0, 0, None,
                                              None, stream), "mlp32_forward_p(color)")
    finally:                                 # the row count and the I/O width are per call: never left behind
        lib.enerf_mlp32_io16(0)
        lib.enerf_mlp32_valid_rows(None)
    L.check(lib.enerf_stratified_composite_forward_ex(w.data_ptr(), incl.data_ptr(), count.data_ptr(),
                                                      opacity.data_ptr(), rgb.data_ptr(), bg.data_ptr(), per_ray, N, T, C,
                                                      image.data_ptr(), store, stream), "stratified_composite_forward")
    if KEEP_LAST:
        last = dict(w=w, count=count, incl=incl, h16=h16, sigma=sigma, cin=cin, rgb=rgb)
    if not train:
        return image, depth, None
    sv = dict(rd=rd, bg=bg, per_ray=per_ray, N=N, T=T, C=C, B=B, cap=cap, inv_T=inv_T, s_dens=s_dens, z=z, xyz=xyz,
              nears=nears, fars=fars, opacity=opacity, sigma=sigma, h16=h16, feats=feats, fb_s=fb_s, w=w, count=count, incl=incl, cin=cin,
              rgb=rgb, fb_c=fb_c, seg_s=seg_s, seg_c=seg_c, weights=weights, emb=emb, offsets=offsets, param=embeddings,
              S=S, H=base_resolution, gridtype=gridtype, affine=affine, prec=prec, store=store, cdt=cdt)
    return image, depth, sv


def render_backward(sv, g_image, g_depth):
    """-> (embedding gradient or None when it was added into the parameter's .grad, *the five MLP weight gradients)"""
    N, T, C, B, cap = sv["N"], sv["T"], sv["C"], sv["B"], sv["cap"]
    dev = sv["z"].device
    f32 = dict(dtype=torch.float32, device=dev)
    lib = L.lib()
    stream = L.stream_handle()
    Bp, capp = pad32(B), pad32(cap)
    g_image = torch.zeros(N, C, **f32) if g_image is None else g_image.float().contiguous().view(N, C)
    g_depth = None if g_depth is None else g_depth.float().contiguous().view(N)
    g_sigma = torch.empty(B, **f32)
    store, cdt = sv["store"], sv["cdt"]
    g_rgb = torch.empty(capp, C, dtype=cdt, device=dev)
    incl, count = sv["incl"], sv["count"]
    L.check(lib.enerf_stratified_composite_backward_ex(
        g_image.data_ptr(), g_depth.data_ptr() if g_depth is not None else None, sv["z"].data_ptr(),
        sv["sigma"].data_ptr(), sv["w"].data_ptr(), sv["nears"].data_ptr(), sv["fars"].data_ptr(), incl.data_ptr(),
        count.data_ptr(), sv["rgb"].data_ptr(), sv["bg"].data_ptr(), sv["per_ray"], N, T, C, sv["inv_T"], sv["s_dens"],
        cap, g_sigma.data_ptr(), g_rgb.data_ptr(), store, stream), "stratified_composite_backward")

    dw, (dseg_s, dseg_c) = _fn._grad_segments("linear", dev, C)
    dx = torch.empty(capp, 32, dtype=cdt, device=dev)
    # (under a valid-row count the colour backward is the fused kernel, which does not touch `bb`; the 16-bit form
    #  recomputes the hidden activations and reads no `fb`)
    bb_c = torch.empty(1, **f32)
    fb_c = sv["fb_c"]
    lib.enerf_mlp32_valid_rows(incl.data_ptr() + 4 * (N - 1))
    lib.enerf_mlp32_io16(1 if store == L.F16 else 0)
    try:
        with _fn._precision(sv["prec"]):
            L.check(lib.enerf_mlp32_backward_p(g_rgb.data_ptr(), sv["cin"].data_ptr(), sv["seg_c"], dseg_c, 31, 1, 1,
                                               fb_c.data_ptr() if fb_c is not None else None, cap, 32, C, 2, 0,
                                               bb_c.data_ptr(), dx.data_ptr(), 0, 0, sv["rgb"].data_ptr(), C, None, None,
                                               0, stream), "mlp32_backward_p(color)")
    finally:
        lib.enerf_mlp32_io16(0)
        lib.enerf_mlp32_valid_rows(None)
    dh16 = torch.empty(B, 16, **f32)
    L.check(lib.enerf_stratified_scatter_geo_grad_ex(sv["w"].data_ptr(), incl.data_ptr(), count.data_ptr(),
                                                     dx.data_ptr(), N, T, dh16.data_ptr(), store, stream),
            "stratified_scatter_geo_grad")
    dfeat = torch.empty(16, Bp, 2, **f32)
    bb_s = torch.empty(1, Bp, 64, **f32)
    with _fn._precision(sv["prec"]):
        L.check(lib.enerf_mlp32_backward_p(dh16.data_ptr(), sv["feats"].data_ptr(), sv["seg_s"], dseg_s, 32, 0, 1,
                                           sv["fb_s"].data_ptr(), B, 32, 16, 1, 0, bb_s.data_ptr(), dfeat.data_ptr(), 1, 16,
                                           None, 0, g_sigma.data_ptr(), sv["h16"].data_ptr(), 16, stream),
                "mlp32_backward_p(sigma)")
    param, emb = sv["param"], sv["emb"]
    target = _ge.param_grad_target(param, torch.float32)
    direct = target is not None
    g_emb = target if direct else torch.zeros_like(emb)
    _gb.grid_encode_backward(dfeat, sv["xyz"], emb, sv["offsets"], g_emb, B, 3, 2, 16, sv["S"], sv["H"], False, dfeat,
                             dfeat, sv["gridtype"], layout=2, affine=sv["affine"])
    return (None if direct else g_emb,) + _fn.unpack_weight_grads(dw, C)


class _StratifiedRender(Function):
    @staticmethod
    def forward(ctx, ro, rd, u, bg, per_ray, aabb, geo, train, embeddings, offsets, *weights):
        image, depth, sv = render_forward(ro, rd, u, bg, per_ray, aabb, geo, train, embeddings, offsets, *weights)
        ctx.sv = sv
        ctx.set_materialize_grads(False)     # (an unused depth must add no depth term: t is NaN on rays that miss)
        return image, depth

    @staticmethod
    def backward(ctx, g_image, g_depth):
        sv = ctx.sv
        ctx.sv = None
        g_bg = None
        if ctx.needs_input_grad[3] and g_image is not None:
            # image = sum w rgb + (1 - opacity) bg: asked for by the background model's per-ray colours only
            g_bg = (1 - sv["opacity"]).unsqueeze(-1) * g_image.float().reshape(sv["N"], sv["C"])
        g = render_backward(sv, g_image, g_depth)
        return (None,) * 3 + (g_bg,) + (None,) * 4 + (g[0], None) + tuple(g[1:])
