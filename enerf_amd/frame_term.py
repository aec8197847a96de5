"""The frame term of a training step, stated in torch: what enerf_composite_rays_train_fwd_bwd_frames_c (csrc/raymarching.hip)
forms inside the compositing launch, from the blended image on.

  Trainer.train_step        nerf/utils.py:595-604, 634   ground truth mixed on the step's background, per-ray error, mean
  Trainer.train_step_events nerf/utils.py:546            the term's weight (weight_loss_rgb)

This is the CPU path of the term and the yardstick the GPU tests hold the kernel to (in fp64); nothing on the hot path
calls it.
"""
import torch


def frame_ground_truth(pixels, bg, C):
    """pixels [..., C] -> themselves; [..., C + 1] (colours, alpha) -> colours * a + bg * (1 - a), in torch's operation
    order (nerf/utils.py:596).  bg: a number, one colour [C] or a colour per pixel [..., C]."""
    if pixels.shape[-1] == C:
        return pixels
    if pixels.shape[-1] != C + 1:
        raise ValueError(f"pixels: expected {C} or {C + 1} channels, got {pixels.shape[-1]}")
    a = pixels[..., C:]
    return pixels[..., :C] * a + bg * (1 - a)


def frame_term_statement(out_image, pixels, bg, weight):
    """-> (gt [..., C], err [...], loss, g_out_image [..., C]) of the frame term on a blended render `out_image` [..., C]:

        gt   = frame_ground_truth(pixels, bg)
        err  = ((out_image - gt) ** 2).mean(-1)               the per-ray error (what the error map takes)
        loss = weight * err.mean()                            the term as it enters the step's loss
        g_out_image = d loss / d out_image = weight * 2 / (C * rays) * (out_image - gt)

    in the tensors' own dtype."""
    C = out_image.shape[-1]
    gt = frame_ground_truth(pixels, bg, C)
    diff = out_image - gt
    err = (diff ** 2).mean(-1)
    loss = weight * err.mean()
    g = diff * (weight * 2.0 / diff.numel())
    return gt, err, loss, g
