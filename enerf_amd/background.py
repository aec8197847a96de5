"""One autograd node for the background model of `NeRFNetwork(bg_radius > 0)` on the MI355X fp32 path.

    rays -> polar coordinates of the exit from the sphere of radius bg_radius      (polar_from_ray's arithmetic)
         -> 2-D multiresolution grid of (p + 1) / 2 (encoder_bg)                   (gridencoder's D = 2 arithmetic)
         -> [SH(d) or zeros | grid] -> bg_net (64 hidden, bias-free) -> sigmoid    (fp32, weights in LDS)

one launch forward (enerf_background_forward) and one launch plus a small reduce backward (enerf_background_backward), in
place of `NeRFNetwork.background(polar_from_ray(...), rays_d)`: polar_from_ray, the SH encoder, `e * 1`, the grid encoder,
cat, two nn.Linear with a ReLU, sigmoid -- and the same again backwards with a zero-filled table gradient.  The backward
keeps nothing but the rays from the forward.  It returns the gradients of the network's own parameters, like
fused_network._FusedNeRF, so optimisers see nothing new.

Anything this does not serve keeps the statement: CPU tensors, autocast (hence the fp16 regime), ray gradients, a
background net that is not two bias-free layers of hidden width 64, a direction encoder that is not SH of degree 4, a
background encoder that is not a 2-D GridEncoder with level_dim 2 and at most MAX_LEVELS levels.
"""
import numpy as np
import torch
from torch.autograd import Function

from . import _lib as L
from . import gridencoder as _ge

ENABLED = True
# backgrounds computed by this route (tests assert that the route was taken)
stats = {"calls": 0}
MAX_LEVELS = 8          # csrc/background.hip: kBgMaxLevels
HIDDEN = 64


def refusals(model, rays_o, rays_d):
    """Why this route does not serve the call (empty: it does)."""
    why = []
    if not ENABLED:
        why.append("disabled")
    if not (rays_o.is_cuda and rays_d.is_cuda):
        why.append("cpu")
    if rays_o.dtype != torch.float32 or rays_d.dtype != torch.float32:
        why.append("dtype")
    if rays_o.requires_grad or rays_d.requires_grad:
        why.append("ray gradients")
    if torch.is_autocast_enabled():
        why.append("autocast")
    net = getattr(model, "bg_net", None)
    if net is None:
        why.append("no bg_net")
        return why
    enc = getattr(model, "encoder_bg", None)
    if not (isinstance(enc, _ge.GridEncoder) and enc.input_dim == 2 and enc.level_dim == 2
            and 1 <= enc.num_levels <= MAX_LEVELS and enc.embeddings.dtype == torch.float32
            and enc.embeddings.device == rays_o.device):
        why.append("encoder_bg")
    from .shencoder import SHEncoder
    enc_dir = getattr(model, "encoder_dir", None)
    if not (isinstance(enc_dir, SHEncoder) and enc_dir.degree == 4):
        why.append("encoder_dir")
    c = getattr(model, "out_dim_color", 0)
    if not 1 <= c <= 3:
        why.append("out_dim_color")
    k = 16 + 2 * getattr(enc, "num_levels", 0)
    layers = list(net)
    if not (len(layers) == 2 and all(isinstance(l, torch.nn.Linear) and l.bias is None
                                     and l.weight.dtype == torch.float32 and l.weight.device == rays_o.device
                                     for l in layers)
            and tuple(layers[0].weight.shape) == (HIDDEN, k) and tuple(layers[1].weight.shape) == (c, HIDDEN)):
        why.append("bg_net")
    return why


def supported(model, rays_o, rays_d):
    return not refusals(model, rays_o, rays_d)


def _geometry(enc):
    """(L, S, H, gridtype) as enerf_grid_encode_forward takes them (gridencoder._grid_encode.forward)."""
    return int(enc.num_levels), float(np.log2(enc.per_level_scale)), int(enc.base_resolution), int(enc.gridtype_id)


def forward_raw(rays_o, rays_d, radius, geo, use_dirs, embeddings, offsets, w0, w1, trace=None):
    """The forward launch -> bg [N, C].  `trace` (tests): an [N, 2 + 16 + 2L] fp32 buffer for the polar pair and the MLP's
    input row."""
    N, C = rays_o.shape[0], w1.shape[0]
    Lv, S, H, gridtype = geo
    bg = torch.empty(N, C, dtype=torch.float32, device=rays_o.device)
    L.check(L.lib().enerf_background_forward(
        rays_o.data_ptr(), rays_d.data_ptr(), float(radius), N, embeddings.data_ptr(), offsets.data_ptr(), Lv, 2, S, H,
        gridtype, 1 if use_dirs else 0, w0.data_ptr(), w1.data_ptr(), w0.shape[0], C, bg.data_ptr(),
        trace.data_ptr() if trace is not None else None, L.stream_handle()), "background_forward")
    return bg


def backward_raw(rays_o, rays_d, radius, geo, use_dirs, embeddings, offsets, w0, w1, grad_image, weights_sum, g_emb):
    """The backward launch (+ reduce): adds into g_emb, -> (grad_w0, grad_w1).  weights_sum None: factor 1."""
    N, C = rays_o.shape[0], w1.shape[0]
    Lv, S, H, gridtype = geo
    g_w0, g_w1 = torch.empty_like(w0), torch.empty_like(w1)
    if N == 0:
        return g_w0.zero_(), g_w1.zero_()
    L.check(L.lib().enerf_background_backward(
        rays_o.data_ptr(), rays_d.data_ptr(), float(radius), N, embeddings.data_ptr(), offsets.data_ptr(), Lv, 2, S, H,
        gridtype, 1 if use_dirs else 0, w0.data_ptr(), w1.data_ptr(), w0.shape[0], C, grad_image.data_ptr(),
        weights_sum.data_ptr() if weights_sum is not None else None, g_w0.data_ptr(), g_w1.data_ptr(), g_emb.data_ptr(),
        L.stream_handle()), "background_backward")
    return g_w0, g_w1


class _Background(Function):
    """The project's idiom for its fused nodes (gridencoder._grid_encode, fused_network._FusedNeRF), with its two caveats:
    the tensors are kept on ctx, not through save_for_backward, so a parameter modified in place between forward and
    backward is not noticed; and where gridencoder.param_grad_target applies (opt-in, see there) the table gradient is
    added straight into the parameter's .grad and None is returned for it, so torch.autograd.grad would then mutate
    .grad and report no gradient for the table."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, radius, geo, use_dirs, offsets, embeddings, w0, w1):
        emb, w0c, w1c = embeddings.contiguous(), w0.contiguous(), w1.contiguous()
        bg = forward_raw(rays_o, rays_d, radius, geo, use_dirs, emb, offsets, w0c, w1c)
        ctx.sv = (rays_o, rays_d, radius, geo, use_dirs, offsets, embeddings, emb, w0c, w1c)
        return bg

    @staticmethod
    def backward(ctx, g_bg):
        rays_o, rays_d, radius, geo, use_dirs, offsets, param, emb, w0, w1 = ctx.sv
        ctx.sv = None
        g_bg = g_bg.float().contiguous().view(rays_o.shape[0], w1.shape[0])
        target = _ge.param_grad_target(param, torch.float32)
        direct = target is not None
        g_emb = target if direct else torch.zeros_like(emb)
        g_w0, g_w1 = backward_raw(rays_o, rays_d, radius, geo, use_dirs, emb, offsets, w0, w1, g_bg, None, g_emb)
        return (None,) * 6 + (None if direct else g_emb, g_w0, g_w1)


def background_from_rays(model, rays_o, rays_d):
    """rays [N,3] fp32 on the device -> bg [N, out_dim_color] through the native node (the caller has asked `supported`)."""
    enc = model.encoder_bg
    bg = _Background.apply(rays_o.contiguous().view(-1, 3), rays_d.contiguous().view(-1, 3), float(model.bg_radius),
                           _geometry(enc), not model.disable_view_direction, enc.offsets, enc.embeddings,
                           model.bg_net[0].weight, model.bg_net[1].weight)
    stats["calls"] += 1
    return bg
