"""Data-parallel tails of the closed-form RGB step, as plain functions of the TrainHarness `h`.
The step leaves `h._raw_grads` = (table gradient, or None when it sits in embeddings.grad; the MLPs' flat dW); `finish`
averages both across ranks and takes the optimizer step by one of three tails, built from the same pieces.  Every rank
runs the same tail, and a tail issues its collectives in one fixed order: ranks deadlock or diverge otherwise."""
import time
from types import SimpleNamespace

import torch
import torch.distributed as dist


_DONE = SimpleNamespace(wait=lambda: None)


def _active():
    return dist.is_available() and dist.is_initialized()


def table_slice(n, rank, world):
    """(lo, hi, shard): rank's slice [lo, hi) of a flat table of n elements cut into `world` pieces of `shard` =
    ceil(n / world) rounded up to a multiple of 4 (FusedAdam ranges start on multiples of 4 elements), clipped to n:
    trailing slices may come out short or empty.  The cut is even when shard * world == n."""
    shard = -(-n // world)
    shard += (-shard) % 4
    return min(rank * shard, n), min((rank + 1) * shard, n), shard


def gather_slices(flat, lo, hi, shard, world, rank, *, in_place_ok, async_op=False):
    """All-gather: slice r of `flat` (table_slice's geometry) <- rank r's.  in_place_ok (RCCL, even cut): in place.
    Otherwise equal-sized pieces padded to `shard`, for any backend and ragged cuts, and every piece but this rank's own
    is copied back with its clipped bounds.  -> a handle; the gather is complete after its wait()."""
    if in_place_ok:
        work = dist.all_gather_into_tensor(flat, flat[lo:hi], async_op=async_op)
        return work if async_op else _DONE
    n = flat.numel()
    send = torch.zeros(shard, dtype=flat.dtype, device=flat.device)
    send[:hi - lo] = flat[lo:hi]
    pieces = [torch.empty(shard, dtype=flat.dtype, device=flat.device) for _ in range(world)]
    work = dist.all_gather(pieces, send, async_op=async_op)

    def wait():
        if async_op:
            work.wait()
        for r, piece in enumerate(pieces):
            a, b = min(r * shard, n), min((r + 1) * shard, n)
            if r != rank and b > a:
                flat[a:b].copy_(piece[:b - a])
    return SimpleNamespace(wait=wait)


def adopt_raw_grads(h):
    """Take over what the step left in h._raw_grads -> (embeddings, their flat gradient, flat dW); the gradient buffer
    is embeddings.grad afterwards either way (None from the step: the kept buffer, the grid backward added into it)."""
    g_emb, dw = h._raw_grads
    h._raw_grads = None
    emb = h.model.encoder.embeddings
    if g_emb is not None:
        emb.grad = g_emb
    return emb, emb.grad.view(-1), dw


def start_mlp(dw, nccl):
    """The MLP gradients travel as the backward's one flat dW buffer.  RCCL averages in the collective; gloo only sums."""
    return dist.all_reduce(dw, op=dist.ReduceOp.AVG if nccl else dist.ReduceOp.SUM, async_op=True)


def finish_mlp(h, dw, work, nccl, world):
    """-> the small parameters with their averaged gradients installed, for step_now(only=) / step_grid_table(extra=)."""
    from . import fused_network
    work.wait()
    if not nccl:
        dw.mul_(1.0 / world)
    m = h.model
    small = fused_network.network_params(m)[1:]
    for p, g in zip(small, fused_network.unpack_weight_grads(dw, getattr(m, "out_dim_color", 3),
                                                             fused_network.kind_of(m))):
        p.grad = g.view_as(p)
    return small


def allreduce_tail(h, issue_prefetch=None):
    """The hash-table gradient is all-reduced in `comm_chunks` pieces and Adam runs on each piece as it lands (the
    optimizer pass over the table hides under the remaining collectives)."""
    emb, flat, dw = adopt_raw_grads(h)
    nccl = dist.get_backend() == "nccl"
    op = dist.ReduceOp.AVG if nccl else dist.ReduceOp.SUM
    world = dist.get_world_size()
    n = flat.numel()
    step = table_slice(n, 0, h.comm_chunks)[2]
    bounds = [(lo, min(lo + step, n)) for lo in range(0, n, step)]
    if h.comm_dtype is None:
        wire = [flat[lo:hi] for lo, hi in bounds]
    else:                                                # opt-in: the table gradient crosses xGMI in 16 bits
        wire = [flat[lo:hi].to(h.comm_dtype) for lo, hi in bounds]
    works = [dist.all_reduce(t, op=op, async_op=True) for t in wire]
    w_dw = start_mlp(dw, nccl)
    if issue_prefetch is not None:
        issue_prefetch(background=False)                  # marches while the gradients are on the wire
    for (lo, hi), t, w in zip(bounds, wire, works):
        w.wait()
        if h.comm_dtype is not None:
            flat[lo:hi].copy_(t)
        if not nccl:
            flat[lo:hi].mul_(1.0 / world)
        h.opt.step_now(only=[emb], ranges={emb: (lo, hi)}, zero_grads=True)
    h._cleared_grad = emb.grad                            # every piece cleared by its Adam pass: kept for the next step
    h.opt.step_now(only=finish_mlp(h, dw, w_dw, nccl, world))


def sharded_tail(h, issue_prefetch=None):
    """The other tail (SURVEY.md 8e "scaling risk (b)"): the table gradient is reduce-scattered, every rank runs Adam on
    its own 1/N of the table only (the 28 B/element optimizer pass shrinks N-fold) and the updated slices are
    all-gathered into every replica's table.  Same bytes on the wire as the ring all-reduce (2 (N-1)/N x 52 MB), but the
    gather half moves parameters, which the next step needs only at its first grid encode.  Replicas stay bit-identical:
    every element is updated by exactly one rank and copied to the others.  The MLP gradients (37 KB) keep their
    all-reduce; their Adam runs everywhere."""
    emb, flat, dw = adopt_raw_grads(h)
    world, rank = dist.get_world_size(), dist.get_rank()
    nccl = dist.get_backend() == "nccl"
    lo, hi, shard = table_slice(flat.numel(), rank, world)
    in_place = nccl and shard * world == flat.numel()
    w_dw = start_mlp(dw, nccl)
    if in_place:
        mine = torch.empty(shard, dtype=flat.dtype, device=flat.device)
        work = dist.reduce_scatter_tensor(mine, flat, op=dist.ReduceOp.AVG, async_op=True)
    else:                                                 # gloo has no reduce-scatter; ragged tables: all-reduce
        work = dist.all_reduce(flat, op=dist.ReduceOp.AVG if nccl else dist.ReduceOp.SUM, async_op=True)
        mine = None
    if issue_prefetch is not None:
        issue_prefetch(background=False)
    work.wait()
    if mine is not None:
        flat[lo:hi].copy_(mine)
    elif not nccl:
        flat[lo:hi].mul_(1.0 / world)
    if hi > lo:
        h.opt.step_now(only=[emb], ranges={emb: (lo, hi)}, zero_grads=True, advance=True)
    # this rank's local contributions to the other slices are spent: clear them for the next step
    flat[:lo].zero_()
    flat[hi:].zero_()
    h._cleared_grad = emb.grad
    gather = gather_slices(emb.data.view(-1), lo, hi, shard, world, rank, in_place_ok=in_place, async_op=True)
    h.opt.step_now(only=finish_mlp(h, dw, w_dw, nccl, world))       # (under the gather)
    gather.wait()


def owner_range(h):
    """(lo, hi, world) of this rank's slice of the flat table for the fused sharded tail, or None when that tail does
    not apply (all-reduce tail, ragged shards, 16-bit wire format, an optimizer without the record-list pass).  Where it
    applies -- n % world == 0 and (n // world) % 4 == 0 -- table_slice's cut IS the exact division n // world."""
    if not (h.fused_sharded and h.comm_mode == "sharded" and h.comm_dtype is None and h.avg is not None
            and hasattr(h.opt, "step_grid_table") and not h.use_graphs and _active()):
        return None
    emb = getattr(getattr(h.model, "encoder", None), "embeddings", None)
    if emb is None or getattr(h.model.encoder, "level_dim", 0) != 2:
        return None
    world, rank = dist.get_world_size(), dist.get_rank()
    # measurement aid (tools/dp_tail_overhead.py): a one-rank world that OWNS only 1 / N of the table, i.e. pays an
    # N-rank world's dense route for the other (N - 1) / N (the collectives degenerate; nothing is averaged)
    pretend = int(getattr(h, "pretend_world", 0) or 0)
    if pretend > 1 and world == 1:
        world = pretend
    lo, hi, shard = table_slice(emb.numel(), rank, world)
    if shard * world != emb.numel():
        return None
    return lo, hi, world


def sharded_fused_tail(h, own, issue_prefetch=None):
    """The sharded tail with the one-GPU flush kept for this rank's own slice: the backward left the slice's tiles as
    record lists and made only the rest of the gradient dense (enerf_grid_owner_range, set and cleared by the caller);
    the dense buffer is reduce-scattered in place (SUM: this rank's slice receives the OTHER ranks' share), the
    optimizer pass sums its own lists in LDS on top of it, divides by the number of ranks, updates the slice and clears
    the buffer, and the slices are all-gathered in place.  Same update as sharded_tail up to the order of the fp32 sums."""
    lo, hi, world = own
    emb, flat, dw = adopt_raw_grads(h)
    nccl = dist.get_backend() == "nccl"
    w_dw = start_mlp(dw, nccl)
    # SUM, not AVG: the optimizer pass applies 1 / ranks to dense share + own lists together (and a one-rank world's
    # in-place SUM is free where RCCL's AVG runs a scaling kernel over the 52 MB)
    real = dist.get_world_size() == world                 # (False: tools/dp_tail_overhead.py's pretend world)
    if nccl:                                              # in place: slice r of the buffer <- sum of everybody's
        work = dist.reduce_scatter_tensor(flat[lo:hi], flat if real else flat[lo:hi], op=dist.ReduceOp.SUM,
                                          async_op=True)
    else:                                                 # gloo has no reduce-scatter
        work = dist.all_reduce(flat, op=dist.ReduceOp.SUM, async_op=True)
    if issue_prefetch is not None:
        issue_prefetch(background=False)
    work.wait()
    enc = h.model.encoder
    h.opt.step_grid_table(emb, enc.offsets, enc.level_dim, extra=finish_mlp(h, dw, w_dw, nccl, world))
    h._cleared_grad = emb.grad                            # cleared everywhere by the optimizer pass
    p = emb.data.view(-1)
    if nccl and not real:
        dist.all_gather_into_tensor(p[lo:hi], p[lo:hi])
    else:                                                 # (the cut is exact: gloo's pieces carry no padding)
        gather_slices(p, lo, hi, hi - lo, world, dist.get_rank(), in_place_ok=nccl).wait()


def finish(h, own, issue_prefetch=None):
    """The tail of one data-parallel step.  own: owner_range(h) as it was set for the step's backward.  -> the name of
    the tail that ran."""
    if own is not None:
        sharded_fused_tail(h, own, issue_prefetch)
        return "sharded_fused"
    if h.comm_mode == "sharded":
        sharded_tail(h, issue_prefetch)
        return "sharded"
    allreduce_tail(h, issue_prefetch)
    return "allreduce"


def gather_sharded_optimizer_state(h):
    """After steps taken with a sharded tail every rank holds current Adam moments only for its own slice of the table.
    Before anything that needs them whole -- switching back to the all-reduce tail, saving a checkpoint -- the slices
    are all-gathered (2 x 52 MB, once; the padded form on every backend)."""
    emb = getattr(getattr(h.model, "encoder", None), "embeddings", None)
    opt = getattr(h, "opt", None)
    st = opt.state.get(emb) if emb is not None and opt is not None else None
    if not st or not _active() or dist.get_world_size() == 1:
        return
    world, rank = dist.get_world_size(), dist.get_rank()
    lo, hi, shard = table_slice(emb.numel(), rank, world)
    for key in ("exp_avg", "exp_avg_sq"):
        gather_slices(st[key].view(-1), lo, hi, shard, world, rank, in_place_ok=False).wait()


def timed_window(step_fn, first_i, window, dev):
    """`window` steps of step_fn(i) from i = first_i between device synchronisations, all ranks starting together; the
    slowest rank's time counts (MAX all-reduce: the same figure on every rank).  -> (ms per step, next i)"""
    sync = (lambda: torch.cuda.synchronize(dev)) if dev.type == "cuda" else (lambda: None)
    sync()
    dist.barrier()
    t0 = time.perf_counter()
    for i in range(first_i, first_i + window):
        step_fn(i)
    sync()
    dt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
    dist.all_reduce(dt, op=dist.ReduceOp.MAX)
    return float(dt.item()) / window * 1e3, first_i + window


def tune_comm(h, step_fn, candidates=(1, 2, 4, 8), window=None):
    """Pick `comm_chunks`, the tail and the march placement by measurement: how the table gradient is best cut depends
    on the link topology and the number of ranks (per-collective latency against Adam / collective overlap).  Each
    candidate runs one timed_window of one update_extra_state period, so every window holds the same work.
    -> {chunks: ms_per_step}, {} when there is nothing to tune."""
    if h.avg is None or not _active() or dist.get_world_size() == 1:
        return {}
    window = int(window or h.update_interval)
    dev = next(h.model.parameters()).device
    i = 0
    timings = {}
    h.comm_mode = "allreduce"
    for k, c in enumerate((candidates[0],) + tuple(candidates)):       # the first window only warms up
        h.comm_chunks = int(c)
        ms, i = timed_window(step_fn, i, window, dev)
        if k:
            timings[int(c)] = ms
    h.comm_chunks = min(timings, key=timings.get)
    # the other tail: reduce-scatter -> Adam on this rank's slice -> all-gather (two windows: the first warms up)
    h.comm_mode = "sharded"
    for _ in range(2):
        sharded_ms, i = timed_window(step_fn, i, window, dev)
    h.gather_sharded_optimizer_state()                    # whichever tail runs next starts from whole moments
    h.comm_mode = "sharded" if sharded_ms < timings[h.comm_chunks] else "allreduce"
    # with the cut settled: where the next batch's march is issued (beside the backward, or beside the collectives)
    placements = {}
    for at in ("forward", "mlp_backward", "collectives"):
        h.prefetch_at = at
        placements[at], i = timed_window(step_fn, i, window, dev)
    h.prefetch_at = min(placements, key=placements.get)
    h.tuned = {"chunks_ms_per_step": dict(timings), "sharded_ms_per_step": sharded_ms,
               "mode": h.comm_mode, "prefetch_at_ms_per_step": placements}
    return timings


def probe_comm_dtype(h, step_fn, dtype=torch.bfloat16, window=None, first_step=0):
    """ms per step over one window with the table gradient on the wire in `dtype` (the opt-in `comm_dtype`), for
    reporting next to the fp32 figure; the setting itself is restored.  None on one rank."""
    if h.avg is None or not _active() or dist.get_world_size() == 1:
        return None
    keep, h.comm_dtype = h.comm_dtype, dtype
    dev = next(h.model.parameters()).device
    try:
        return timed_window(step_fn, first_step, int(window or h.update_interval), dev)[0]
    finally:
        h.comm_dtype = keep
