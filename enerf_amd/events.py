"""The event-loss side of the hot path's caller, re-stated from the reference:

  get_rays / get_event_rays     nerf/utils.py:110-174, 184-216
  rgb_to_luma / lin_log         utils/event_utils.py:23-66
  event_loss / train_step_events   nerf/utils.py:482-573  (Trainer.train_step_events)

`train_step_events` takes the model plus a plain options object instead of a Trainer, but renders, converts and
penalises exactly as the reference does (two renders sharing one random background colour; (lin-)log intensity
difference against polarity * C_thres, or the normalised variant when C_thres == -1).
"""
import numpy as np
import torch


def get_rays(poses, intrinsics, H, W, N=-1, inds=None):
    """poses [B,4,4] cam2world, intrinsics (fx,fy,cx,cy) -> rays_o, rays_d [B,N,3] (+ inds [B,N] when sampled).
    Pixel centres are integer coordinates (no +0.5), as in the reference."""
    device = poses.device
    B = poses.shape[0]
    fx, fy, cx, cy = intrinsics
    i, j = torch.meshgrid(torch.linspace(0, W - 1, W, device=device), torch.linspace(0, H - 1, H, device=device),
                          indexing="ij")
    i = i.t().reshape([1, H * W]).expand([B, H * W])
    j = j.t().reshape([1, H * W]).expand([B, H * W])
    results = {}
    if N > 0:
        N = min(N, H * W)
        if inds is None:
            inds = torch.randint(0, H * W, size=[N], device=device)
        inds = inds.expand([B, N])
        i = torch.gather(i, -1, inds)
        j = torch.gather(j, -1, inds)
        results["inds"] = inds
    zs = torch.ones_like(i)
    xs = (i - cx) / fx * zs
    ys = (j - cy) / fy * zs
    directions = torch.stack((xs, ys, zs), dim=-1)
    directions = directions / torch.norm(directions, dim=-1, keepdim=True)
    rays_d = directions @ poses[:, :3, :3].transpose(-1, -2)
    rays_o = poses[..., :3, 3][..., None, :].expand_as(rays_d)
    results["rays_o"] = rays_o
    results["rays_d"] = rays_d
    return results


def get_event_rays(xs, ys, c2w_before, c2w_at, intrinsics):
    """Per-event ray pairs: pixel (xs, ys) seen from the pose just before and at the event. c2w_* [B,Nevs,3,4]."""
    fx, fy, cx, cy = intrinsics
    zs = torch.ones_like(xs)
    us = (xs - cx) / fx * zs
    vs = (ys - cy) / fy * zs
    dirs_cams = torch.stack((us, vs, zs), dim=-1)
    dirs_cams = dirs_cams / torch.norm(dirs_cams, dim=-1, keepdim=True)
    return {
        "rays_evs_o1": c2w_before[..., :3, 3],
        "rays_evs_d1": torch.sum(dirs_cams[..., None, :] * c2w_before[..., :3, :3], axis=-1),
        "rays_evs_o2": c2w_at[..., :3, 3],
        "rays_evs_d2": torch.sum(dirs_cams[..., None, :] * c2w_at[..., :3, :3], axis=-1),
    }


_luma_factors = {}


def rgb_to_luma(rgb, esim=True):
    """[..., 3] -> [..., 1]; BT.601 weights for esim, BT.709 otherwise.  (utils/event_utils.py:23-33 builds the
    weight tensor on every call; here it is built once per device -- on a GPU that construction is a synchronous
    host-to-device copy in the middle of the step.)"""
    key = (rgb.device, bool(esim))
    factors = _luma_factors.get(key)
    if factors is None:
        w = (0.299, 0.587, 0.114) if esim else (0.2126, 0.7152, 0.0722)
        factors = _luma_factors[key] = torch.tensor(w, dtype=torch.float32, device=rgb.device)
    return torch.sum(rgb * factors[None, :], axis=-1)[..., None]


def lin_log(color, linlog_thres=20):
    """Linear below `linlog_thres`, natural log above, continuous at the threshold."""
    lin_slope = np.log(linlog_thres) / linlog_thres
    return torch.where(color < linlog_thres, lin_slope * color, torch.log(color))


class EventOptions:
    """The subset of the reference's CLI namespace the event step reads (main_nerf.py:97-185)."""

    def __init__(self, **kw):
        self.out_dim_color = 3
        self.use_luma = True
        self.linlog = True
        self.log_thres = 1e-7   # nerf/utils.py:349
        self.C_thres = 0.2
        self.event_only = True
        self.weight_loss_rgb = 1.0
        self.render_kwargs = {}
        # --negative_event_sampling (main_nerf.py; nerf/utils.py:340-345,548): off in every shipped config
        self.negative_event_sampling = False
        self.w_no_ev = 1.0
        self.epoch = 1
        self.epoch_start_noEvLoss = 0
        self.__dict__.update(kw)


def event_loss(image1, image2, pols, opt):
    """(lin-)log intensity change between two renders vs polarity; returns (loss, delta_linlog)."""
    if opt.use_luma:
        l1 = rgb_to_luma(image1, esim=True)
        l2 = rgb_to_luma(image2, esim=True)
    else:
        l1, l2 = image1, image2
    if opt.linlog:
        p1 = lin_log(l1 * 255, linlog_thres=20)
        p2 = lin_log(l2 * 255, linlog_thres=20)
    else:
        thres = torch.as_tensor(opt.log_thres, dtype=l1.dtype, device=l1.device)
        p1 = torch.log(torch.maximum(l1 * 255, thres))
        # the reference evaluates the second term on the *first* luma when use_luma is set (nerf/utils.py:500)
        p2 = torch.log(torch.maximum((l1 if opt.use_luma else l2) * 255, thres))
    delta = p2 - p1
    gt_pol = pols[..., None]
    w = 1.0
    if opt.C_thres != -1:
        loss = w * torch.mean((delta - gt_pol * opt.C_thres) ** 2)
    else:
        EPS = 1e-9
        w *= 20
        if not opt.event_only:
            w *= 20
        dn = delta / (torch.linalg.norm(delta, dim=1, keepdim=True) + EPS)
        pn = gt_pol / (torch.linalg.norm(gt_pol, dim=1, keepdim=True) + EPS)
        loss = w * torch.mean((dn - pn) ** 2)
    return loss, delta


def no_event_loss(image1, image2, opt):
    """The no-event term (nerf/utils.py:548-565): where no event fired between two times the (lin-)log intensity may not
    have changed by more than the contrast threshold: w_no_ev * mean(relu(|L2 - L1| - C)), C = C_thres if > 0 else 0.25.
    The reference uses lin_log here whatever `linlog` says."""
    if opt.use_luma:
        p1 = lin_log(rgb_to_luma(image1, esim=True) * 255, linlog_thres=20)
        p2 = lin_log(rgb_to_luma(image2, esim=True) * 255, linlog_thres=20)
    else:
        p1 = lin_log(image1 * 255, linlog_thres=20)
        p2 = lin_log(image2 * 255, linlog_thres=20)
    cno = opt.C_thres if opt.C_thres > 0 else 0.25
    return opt.w_no_ev * torch.mean(torch.relu(torch.abs(p2 - p1) - cno))


def wants_no_event_term(opt):
    return bool(getattr(opt, "negative_event_sampling", False)) and opt.epoch > opt.epoch_start_noEvLoss


def _fused_images(image1, image2):
    """Whether the loss kernels of csrc/event_pairs.hip take these two renders: on the device, fp32, the same shape,
    1..3 channels."""
    return (image1.is_cuda and image1.dtype == image2.dtype == torch.float32 and image1.shape == image2.shape
            and 1 <= image1.shape[-1] <= 3)


def event_loss_with_grads(image1, image2, pols, opt):
    """-> (loss, delta, d loss / d image1, d loss / d image2).  On the device, fp32, images of 1..3 channels (luma:
    three): one launch (enerf_event_loss_fwd_bwd_c, csrc/event_pairs.hip) in place of the ~50 elementwise / reduction
    launches of event_loss + autograd; anything else goes through those.  The normalised loss (C_thres == -1) takes its
    norms per batch entry: the kernel serves one entry, [1,N,C] images with [1,N] polarities (all the reference's collate
    makes), and is handed the reference's weight -- 20, times 20 when frames are trained too -- as `upstream`."""
    C = image1.shape[-1]
    normalised = opt.C_thres == -1
    fused = (_fused_images(image1, image2) and pols.dtype == torch.float32 and pols.numel() * C == image1.numel()
             and (not opt.use_luma or C == 3)
             and (not normalised or (image1.dim() == 3 and image1.shape[0] == 1 and pols.dim() == 2)))
    if fused:
        from . import _lib as L
        a, b, p = image1.detach().contiguous(), image2.detach().contiguous(), pols.contiguous()
        n = p.numel()
        g1, g2 = torch.empty_like(a), torch.empty_like(b)
        delta = torch.empty(*a.shape[:-1], 1 if opt.use_luma else C, dtype=torch.float32, device=a.device)
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        upstream = 1.0 if not normalised else (20.0 if opt.event_only else 400.0)
        L.check(L.lib().enerf_event_loss_fwd_bwd_c(a.data_ptr(), b.data_ptr(), p.data_ptr(), n, int(bool(opt.use_luma)),
                                                   int(bool(opt.linlog)), float(opt.C_thres), float(opt.log_thres),
                                                   upstream, g1.data_ptr(), g2.data_ptr(), delta.data_ptr(),
                                                   loss.data_ptr(), C, L.stream_handle()), "event_loss_fwd_bwd")
        return loss, delta, g1, g2
    a = image1.detach().requires_grad_(True)
    b = image2.detach().requires_grad_(True)
    with torch.enable_grad():
        loss, delta = event_loss(a, b, pols, opt)
        g1, g2 = torch.autograd.grad(loss, [a, b], allow_unused=True)
    g1 = torch.zeros_like(a) if g1 is None else g1
    g2 = torch.zeros_like(b) if g2 is None else g2
    return loss.detach(), delta.detach(), g1, g2


def no_event_loss_with_grads(image1, image2, opt):
    """-> (loss, d loss / d image1, d loss / d image2) of no_event_loss.  On the device, fp32, images of 1..3 channels
    (luma: three): one launch (enerf_no_event_loss_fwd_bwd_c); anything else goes through no_event_loss + autograd."""
    C = image1.shape[-1]
    if _fused_images(image1, image2) and image1.numel() > 0 and (not opt.use_luma or C == 3):
        from . import _lib as L
        a, b = image1.detach().contiguous(), image2.detach().contiguous()
        g1, g2 = torch.empty_like(a), torch.empty_like(b)
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        cno = opt.C_thres if opt.C_thres > 0 else 0.25
        L.check(L.lib().enerf_no_event_loss_fwd_bwd_c(a.data_ptr(), b.data_ptr(), a.numel() // C, int(bool(opt.use_luma)),
                                                      float(cno), float(opt.w_no_ev), g1.data_ptr(), g2.data_ptr(),
                                                      loss.data_ptr(), C, L.stream_handle()), "no_event_loss_fwd_bwd")
        return loss, g1, g2
    a = image1.detach().requires_grad_(True)
    b = image2.detach().requires_grad_(True)
    with torch.enable_grad():
        loss = no_event_loss(a, b, opt)
        g1, g2 = torch.autograd.grad(loss, [a, b])
    return loss.detach(), g1, g2


def train_step_events(model, data, opt, criterion=None, bg_color=None, bg_color_no_evs=None, return_terms=False):
    """One event training step's forward: two renders (+ optional frame render, + optional no-event pair of renders)
    -> (loss, delta).  nerf/utils.py:482-573.  `bg_color` / `bg_color_no_evs` [B,1,C] replace the step's random
    background draws (tests).  With `return_terms` a third value, the terms as the reference logs them (its
    `losses_indiv`): dict(loss_evs, loss_frames (unweighted, None without the term), loss_no_evs (None without the
    term)), detached -- the same dict train_step_events_manual hands out."""
    images = data["images"]
    B = images.shape[0]
    dev = data["rays_evs_o1"].device
    # the reference draws this on the host and copies it over (nerf/utils.py:497); a pageable host->device copy
    # drains the stream every step, so the same U[0,1) draw is made on the device
    bg = torch.rand((B, 1, opt.out_dim_color), device=dev) if bg_color is None else bg_color
    kw = dict(opt.render_kwargs)
    kw.setdefault("out_dim_color", opt.out_dim_color)
    out1 = model.render(data["rays_evs_o1"], data["rays_evs_d1"], staged=False, bg_color=bg, perturb=True, **kw)
    out2 = model.render(data["rays_evs_o2"], data["rays_evs_d2"], staged=False, bg_color=bg, perturb=True, **kw)
    loss, delta = event_loss(out1["image"], out2["image"], data["pols"], opt)
    terms = dict(loss_evs=loss.detach(), loss_frames=None, loss_no_evs=None)
    if not opt.event_only:
        C = images.shape[-1]
        if C == 4:
            bg_color = torch.rand_like(images[..., :opt.out_dim_color])
            gt = images[..., :opt.out_dim_color] * images[..., opt.out_dim_color:] + \
                bg_color * (1 - images[..., opt.out_dim_color:])
        else:
            bg_color, gt = None, images
        out = model.render(data["rays_o"], data["rays_d"], staged=False, bg_color=bg_color, perturb=True, **kw)
        crit = criterion if criterion is not None else torch.nn.MSELoss(reduction="none")
        loss_frames = crit(out["image"], gt).mean()
        terms["loss_frames"] = loss_frames.detach()
        loss = loss + opt.weight_loss_rgb * loss_frames
    if wants_no_event_term(opt):
        # two more renders at pixels / times without events, a fresh background draw (nerf/utils.py:548-565)
        bg_no = torch.rand((B, 1, opt.out_dim_color), device=dev) if bg_color_no_evs is None else bg_color_no_evs
        n1 = model.render(data["rays_no_evs_o1"], data["rays_no_evs_d1"], staged=False, bg_color=bg_no, perturb=True, **kw)
        n2 = model.render(data["rays_no_evs_o2"], data["rays_no_evs_d2"], staged=False, bg_color=bg_no, perturb=True, **kw)
        loss_no = no_event_loss(n1["image"], n2["image"], opt)
        terms["loss_no_evs"] = loss_no.detach()
        loss = loss + loss_no
    if return_terms:
        return loss, delta, terms
    return loss, delta


def frame_background(images, C, bg_color_frames=None):
    """The frame render's background in an event step with frames (nerf/utils.py:536-540): a per-pixel draw for alpha
    images (`bg_color_frames` replaces the draw), the renderer's default white otherwise."""
    if images.shape[-1] == C + 1:
        return torch.rand_like(images[..., :C]) if bg_color_frames is None else bg_color_frames
    return 1


def train_step_events_manual(model, data, opt, after_forward=None, bg_color=None, defer_table=False,
                             after_mlp_backward=None, bg_color_no_evs=None, bg_color_frames=None, return_terms=False):
    """The event step with its renders driven without autograd (fused_render.render_train_raw / backward_raw): the
    event losses and their image gradients come from event_loss_with_grads / no_event_loss_with_grads (one launch each
    on the device), and the gradients are handed to the renders' closed backward; with `event_only` off the frame render
    sits third, as the reference's (its counter slot and its background draw land where the reference's do), and its loss,
    gradient and alpha mix are formed inside its compositing launch (fused_render.backward_raw(frames=...)) with the
    weight `weight_loss_rgb`.  Same values as train_step_events + loss.backward() (nerf/utils.py:482-567); leaves the
    gradients in p.grad and returns (loss, delta) -- with `return_terms` a third value, the terms as the reference logs
    them: dict(loss_evs, loss_frames (unweighted, None without the term), loss_no_evs (None without the term)).
    `after_forward()` is called once every forward is queued, `after_mlp_backward()` once the last render's MLP backward
    kernels are.  `bg_color` / `bg_color_frames` / `bg_color_no_evs` replace the step's draws (tests)."""
    from . import fused_network as fnet
    from . import fused_render as fr
    images = data["images"]
    B = images.shape[0]
    dev = data["rays_evs_o1"].device
    bg = torch.rand((B, 1, opt.out_dim_color), device=dev) if bg_color is None else bg_color
    kw = {k: v for k, v in opt.render_kwargs.items() if k in ("dt_gamma", "max_steps")}
    shape = data["rays_evs_o1"].shape[:-1]
    img1, ctx1 = fr.render_train_raw(model, data["rays_evs_o1"], data["rays_evs_d1"], bg, True, **kw)
    img2, ctx2 = fr.render_train_raw(model, data["rays_evs_o2"], data["rays_evs_d2"], bg, True, **kw)
    ctxs = [ctx1, ctx2]
    frames = None
    if not opt.event_only:
        # the frame render (nerf/utils.py:531-546): composited by its backward call, in the launch that forms the term
        bg_frames = frame_background(images, opt.out_dim_color, bg_color_frames)
        _, ctxf = fr.render_train_raw(model, data["rays_o"], data["rays_d"], bg_frames, True, composite=False, **kw)
        frames = dict(pixels=images, weight=float(opt.weight_loss_rgb),
                      err_out=torch.empty(ctxf["N"], dtype=torch.float32, device=dev) if return_terms else None)
        loss_frames_w = torch.zeros((), dtype=torch.float32, device=dev)
        ctxs.append(ctxf)
    no_ev = wants_no_event_term(opt)
    if no_ev:
        # the no-event pair of renders (nerf/utils.py:548-551): same closed-form route, its own background draw
        bg_no = torch.rand((B, 1, opt.out_dim_color), device=dev) if bg_color_no_evs is None else bg_color_no_evs
        nshape = data["rays_no_evs_o1"].shape[:-1]
        img3, ctx3 = fr.render_train_raw(model, data["rays_no_evs_o1"], data["rays_no_evs_d1"], bg_no, True, **kw)
        img4, ctx4 = fr.render_train_raw(model, data["rays_no_evs_o2"], data["rays_no_evs_d2"], bg_no, True, **kw)
        ctxs += [ctx3, ctx4]
    if after_forward is not None:
        after_forward()                                 # e.g. the next step's two marches on a side stream
    C = img1.shape[-1]
    loss, delta, g1, g2 = event_loss_with_grads(img1.view(*shape, C), img2.view(*shape, C), data["pols"], opt)
    grads = [g1, g2]
    loss_evs, loss_no = loss, None
    if frames is not None:
        grads.append(None)                              # (the frame render's gradient is formed by its own backward)
    if no_ev:
        loss_no, g3, g4 = no_event_loss_with_grads(img3.view(*nshape, C), img4.view(*nshape, C), opt)
        loss = loss + loss_no
        grads += [g3, g4]
    params = fnet.network_params(model)
    emb = params[0]
    keep = emb.grad if defer_table else None            # (deferred flush: the dense buffer is kept, and kept clean)
    for p in params:
        p.grad = None
    if defer_table:
        emb.grad = keep if keep is not None else torch.zeros_like(emb)
    # defer_table: every render's table gradients stay record lists for FusedAdam.step_grid_table (one flush)
    total = sum(c["M"] for c in ctxs) if defer_table else 0
    dw = None
    for i, (c, g) in enumerate(zip(ctxs, grads)):
        last = i == len(ctxs) - 1
        if g is None:
            g_emb, dwi = fr.backward_raw(c, frames=frames, loss_out=loss_frames_w, raw=True, defer_table=total,
                                         after_mlp=after_mlp_backward if last else None)
        else:
            g_emb, dwi = fr.backward_raw(c, g_image=g, raw=True, defer_table=total,
                                         after_mlp=after_mlp_backward if last else None)
        if g_emb is not None:                           # the first backward's buffer; later ones add straight into it
            if emb.grad is None:                        # ... unless they could not (then they return their own)
                emb.grad = g_emb
            else:
                emb.grad.add_(g_emb)
        dw = dwi if dw is None else dw.add_(dwi)
    kind = ctx1["sv"]["kind"]
    for p, g in zip(params[1:], fnet.unpack_weight_grads(dw, ctx1["sv"]["out_c"], kind)):
        p.grad = g.view_as(p)
    if frames is not None:
        loss = loss + loss_frames_w                     # (complete once the frame render's backward is queued)
    if return_terms:
        terms = dict(loss_evs=loss_evs.detach(), loss_no_evs=loss_no,
                     loss_frames=None if frames is None else frames["err_out"].mean())
        return loss.detach(), delta, terms
    return loss.detach(), delta
