"""The implicit contrast threshold of an event step: the reference's `estimate_C_thres_from_pol_dL`
(utils/event_utils.py:69-107), which Trainer.train_step_events calls with `--log_implicit_C_thres 1` (the default) and
train_one_epoch writes as train/est_C_med_* (nerf/utils.py:511-515, 985-989).

The four medians of delta_linlog / polarity -- over the positive events, the negative ones, and the sign-consistent
subsets of both -- are the contrast threshold the renders imply; the shipped configs fix C_thres per scene, and this
curve shows whether that choice fits.

  estimate_C_thres_statement   the reference function, operation by operation (the CPU path, and what the kernel is held to)
  estimate_C_thres             one launch of enerf_event_c_estimate on the device, nothing read back; the statement
                               for whatever that does not serve

A named deviation: the reference's call site hands the function [B,N,1] / [B,N,C] tensors, on which its
`[:, 0]` indexing reads the first EVENT's polarity instead of every event's.  What is built here is the function as its
docstring states it, (N,1) / (N,C), applied to the one batch entry the collate makes.
"""
import torch

from .events import rgb_to_luma

NAMES = ("median_on", "median_off", "median_on_sign", "median_off_sign")


def estimate_C_thres_statement(pols, delta, esim=True, with_counts=False):
    """(N,1) polarities, (N,1 or 3) intensity differences -> dict of the four medians (0-dim tensors): the reference's
    function operation by operation.  Kept as they are: the luma branch tests the number of EVENTS (`shape[0] == 3`),
    not of channels; an empty class becomes `torch.Tensor([0])` (a CPU tensor whatever the inputs' device); with C
    channels and no luma the median runs over all n * C quotients and the sign conditions read channel 0.
    `with_counts`: -> (dict, the four numbers of quotients)."""
    if delta.shape[0] == 3:
        delta = rgb_to_luma(delta, esim=esim)
    pol0, d0 = pols[:, 0], delta[:, 0]
    on = torch.where(pol0 > 0)[0]
    q_on = delta[on] / pols[on]
    on_sign = torch.where((pol0 > 0) & (d0 >= 0))[0]
    q_on_sign = delta[on_sign] / pols[on_sign]
    off = torch.where(pol0 < 0)[0]
    q_off = delta[off] / pols[off]
    off_sign = torch.where((pol0 < 0) & (d0 <= 0))[0]
    q_off_sign = delta[off_sign] / pols[off_sign]
    classes = [q_on, q_off, q_on_sign, q_off_sign]                   # (the order of NAMES)
    counts = [int(q.numel()) for q in classes]
    classes = [torch.Tensor([0]) if q.shape[0] < 1 else q for q in classes]
    est = {name: torch.median(q) for name, q in zip(NAMES, classes)}
    return (est, counts) if with_counts else est


def _one_entry(pols, delta):
    """[N,1] / [N] with [N,C], or the event step's [1,N] / [1,N,1] with [1,N,C] -> ([N,1], [N,C])."""
    if delta.dim() == 3:
        if delta.shape[0] != 1:
            raise ValueError(f"estimate_C_thres: one batch entry (the reference's collate makes one), got {delta.shape[0]}")
        if pols.dim() < 2 or pols.shape[0] != 1:
            raise ValueError(f"estimate_C_thres: polarities {tuple(pols.shape)} beside deltas {tuple(delta.shape)}")
        delta, pols = delta[0], pols[0]
    if delta.dim() != 2:
        raise ValueError(f"estimate_C_thres: deltas [N,C] or [1,N,C], got {tuple(delta.shape)}")
    pols = pols.reshape(-1, 1)
    if pols.shape[0] != delta.shape[0]:
        raise ValueError(f"estimate_C_thres: {pols.shape[0]} polarities beside {delta.shape[0]} deltas")
    return pols, delta


def estimate_C_thres(pols, delta, out=None):
    """-> (medians [4] fp32 in the order of NAMES, counts [4] int32: the quotients each median was taken over), on the
    inputs' device.  fp32 inputs on the device with N != 3 and 1..3 channels: ONE launch (enerf_event_c_estimate,
    csrc/event_pairs.hip) on the current stream and no host synchronisation -- the reference's statement is four
    torch.where calls, each a read-back of a data-dependent shape.  Everything else (the CPU, other dtypes, N == 3 where
    the reference forms a luma) takes estimate_C_thres_statement.  `out`: 8 contiguous fp32 values to write into -- the
    medians, then the counts' int32 bits (a row of TrainLog's ring); the returned tensors are views of it."""
    pols, delta = _one_entry(pols, delta)
    N, C = delta.shape
    dev = delta.device
    if out is None:
        out = torch.empty(8, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.numel() != 8 or not out.is_contiguous() or out.device != dev:
        raise ValueError("estimate_C_thres: `out` is 8 contiguous fp32 values on the inputs' device")
    med, cnt = out[:4], out[4:].view(torch.int32)
    if (delta.is_cuda and pols.device == dev and delta.dtype == pols.dtype == torch.float32 and N != 3 and 1 <= C <= 3):
        from . import _lib as L
        d, p = delta.detach().contiguous(), pols.detach().contiguous()
        L.check(L.lib().enerf_event_c_estimate(d.data_ptr(), p.data_ptr(), N, C, med.data_ptr(), cnt.data_ptr(),
                                               L.stream_handle()), "event_c_estimate")
        return med, cnt
    est, counts = estimate_C_thres_statement(pols.detach(), delta.detach(), with_counts=True)
    med.copy_(torch.stack([est[n].detach().to(torch.float32).cpu() for n in NAMES]))
    cnt.copy_(torch.tensor(counts, dtype=torch.int32))
    return med, cnt
