"""One autograd node for a whole training render on the MI355X fp32 path (the `self.training` branch of
NeRFRenderer.run_cuda, nerf/renderer.py:318-353 of the reference):

    near_far_from_aabb -> march_rays_train -> network (fused_network) -> composite_rays_train
    -> image + (1 - weights_sum) * bg_color,  depth normalised to [0,1]

Every kernel is the library's; what the node removes is the autograd / dispatcher traffic between them (four Function
nodes, a dozen elementwise launches), which is what bounds a 4096-ray step once the kernels are fast.  Values are those
of the op-by-op route; `tests/test_gpu_training.py` compares the two.
"""
import contextlib

import torch
from torch.autograd import Function

from . import _lib as L
from . import fused_network as fnet
from . import raymarching as _rm
from .backends import _raymarching as _rb

ENABLED = True


def channels(model):
    """Colour channels of the model's renders: the colour net's output width (NeRFNetwork: out_dim_color; FFMLP: 3)."""
    return int(getattr(model, "out_dim_color", 3))


def supported(model, rays_o, rays_d, bg_color, dt_gamma, background_model=False):
    """`background_model`: bg_color is the model's own per-ray background (background.py): bg_radius > 0 is then no
    refusal, and the tensor may carry a gradient (the node returns d bg)."""
    C = channels(model)
    if not 1 <= C <= 3:                           # the compositing kernels serve 1..3 channels
        return False
    if not (ENABLED and fnet.ENABLED and model.training and model.cuda_ray and (background_model or model.bg_radius <= 0)
            and rays_o.is_cuda and rays_o.dtype == torch.float32 and rays_d.dtype == torch.float32
            and not torch.is_autocast_enabled() and not rays_o.requires_grad and not rays_d.requires_grad
            and _rm._DEVICE == "cuda" and torch.is_grad_enabled()):
        return False
    if isinstance(bg_color, torch.Tensor):
        # the composite kernels take a scalar, one colour or one colour per ray, fp32 and dense; anything else the reference's
        # `image + (1 - ws)[:, None] * bg_color` would broadcast goes the op-by-op route
        if ((bg_color.requires_grad and not background_model) or not bg_color.is_cuda or bg_color.dtype != torch.float32
                or not bg_color.is_contiguous() or bg_color.numel() not in (1, C, C * rays_o.view(-1, 3).shape[0])):
            return False
    probe = rays_o.view(-1, 3)
    return fnet.supported(model, probe, probe)


_BOX_FOR = {}        # device index -> key of the bitfield the library's occupied box was last computed for
_BOX_TOKENS = iter(range(1, 1 << 62))


def occupied_box_flag(model):
    """-> the marcher flag (4) that enables the occupied-box test, after making sure the library's box belongs to this
    model's current bitfield: recomputed on the current stream when another model used the box last, or when this
    model's bitfield changed storage, torch version (copy_, load_state_dict) or the package's raw-write epoch
    (packbits, update_extra_state).  The model carries a unique token, so a new model whose bitfield happens to land
    on a freed one's address is never mistaken for it."""
    bf = model._buffers["density_bitfield"]
    token = model.__dict__.get("_occ_box_token")
    if token is None:
        token = model.__dict__["_occ_box_token"] = next(_BOX_TOKENS)
    key = (token, bf.data_ptr(), bf._version, _rm.BITFIELD_EPOCH[0], int(model.cascade), int(model.grid_size),
           float(model.bound))
    if _BOX_FOR.get(bf.device.index) != key:
        _rb.occupied_box_update(bf, model.cascade, model.grid_size, model.bound)
        _BOX_FOR[bf.device.index] = key
    return 4


class _Stage(dict):
    """A march stage's buffers.  When its kernels were issued on a launch stream, the buffers (allocated from the
    consumer stream's pool, see march_stage) must not be recycled before that stream is done with them: a stage that
    is consumed hands its "ready" event to the consumer, which waits for it; one that is dropped unconsumed -- the
    rays never came, the bitfield changed, the model was deleted -- makes the current stream wait here, before its
    tensors go back to the pool."""

    def __del__(self):
        ready = self.get("ready")
        if ready is not None:
            try:
                torch.cuda.current_stream().wait_event(ready)
            except Exception:           # interpreter shutdown
                pass


def _budget_rows(count):
    """A sample count rounded as the reference rounds its budget (raymarching.py:186-189, align = 128)."""
    return count + (128 - count % 128)


def _cold_crop(model, m, N, max_steps):
    """The reference's crop of its N * max_steps rows to a count of m samples; remembered on the model, for the cold
    window's later reservations."""
    rows = model._cold_rows = min(_budget_rows(m), N * int(max_steps))
    return rows


def _ray_bufs(N, dev):
    """What a march of N rays fills per ray."""
    return dict(nears=torch.empty(N, dtype=torch.float32, device=dev), fars=torch.empty(N, dtype=torch.float32, device=dev),
                rays=torch.empty(N, 3, dtype=torch.int32, device=dev))


def _sample_bufs(rows, dev):
    """One set of sample buffers of `rows` rows, uninitialised: the write pass zero-fills the rows no ray writes."""
    f32 = dict(dtype=torch.float32, device=dev)
    return dict(xyzs=torch.empty(rows, 3, **f32), dirs=torch.empty(rows, 3, **f32), deltas=torch.empty(rows, 2, **f32))


def _write_pass(model, pre, rays_o, rays_d, perturb, dt_gamma, max_steps, rows):
    """The write pass of the stage `pre`, whose count pass has run, into fresh buffers of `rows` rows -> the stage."""
    bufs = _sample_bufs(rows, rays_o.device)
    _rb.march_rays_train_write(rays_o, rays_d, model._buffers["density_bitfield"], model.bound, float(dt_gamma),
                               int(max_steps), rays_o.shape[0], model.cascade, model.grid_size, rows, pre["nears"],
                               pre["fars"], bufs["xyzs"], bufs["dirs"], bufs["deltas"], pre["rays"], pre["counter"],
                               bool(perturb), 1)
    pre.update(bufs, M=rows)
    return pre


def march_stage(model, rays_o, rays_d, counter, mean_count, perturb, force_all_rays, dt_gamma, max_steps,
                background=False, defer=False, launch_stream=None, after_signal=False):
    """near_far_from_aabb + march_rays_train: everything of a training render that does not read the parameters.
    Returns the sample buffers; a data-parallel harness runs it for the NEXT batch while the gradient all-reduce of
    the current step is in flight (TrainHarness.prefetch_march).

    While no sample budget exists (`mean_count <= 0`: the first update_extra_state window; or `force_all_rays`) the
    reference's wrapper allocates and zero-fills N * max_steps rows, marches, reads the count back and crops
    (raymarching/raymarching.py:195-228).  The marcher here counts before it writes, so only the count pass runs first;
    its total comes back through pinned memory and the write pass goes into buffers of exactly the cropped size
    (same rows, same `rays` / `counter`: the drop rule still sees min(cropped size, N * max_steps)).  With `defer` the
    read-back is left to finish_march(): a stage issued ahead of its step has long finished by then, so the wait is
    free and the cold window runs the same launch sequence as the budgeted steady state -- write pass included, into
    rows reserved from the previous render's count (kept when the count that comes back fits).

    `launch_stream`: the kernels are issued on that stream (ordered after everything queued so far on the current
    one) while every buffer is allocated HERE, from the current stream's pool: the consumer is the current stream,
    which waits for the stage's event before it reads and frees in its own order -- nothing has to be
    `record_stream`-ed, and no buffer's release puts an event record (a barrier packet, ~15 us of idle queue) between
    two kernels of the training step."""
    N = rays_o.shape[0]
    dev = rays_o.device
    budgeted = not (force_all_rays or mean_count <= 0)
    pre = _Stage(_ray_bufs(N, dev), counter=counter)
    nears, fars, rays = pre["nears"], pre["fars"], pre["rays"]
    spec_rows = 0
    if budgeted:
        M = _budget_rows(mean_count)
        samples = _sample_bufs(M, dev)           # (the write pass zero-fills the rows no ray writes)
    if not budgeted and defer and not force_all_rays:
        # no budget yet, but the previous render's count is known: its rows + 1/8 are reserved here and the write pass
        # follows the count pass on the same stream, unseen by the host; finish_march() keeps the result when the count
        # it reads back fits (consecutive batches differ by a few per cent) and repeats the write pass when not
        last = int(getattr(model, "_cold_rows", 0))
        if last > 0:
            spec_rows = min(_budget_rows(last + last // 8), N * max_steps)
            samples = _sample_bufs(spec_rows, dev)
    bufs = model._buffers                            # (nn.Module.__getattr__ is a slow path)
    bitfield = bufs["density_bitfield"]
    box = occupied_box_flag(model)
    if launch_stream is not None:
        if after_signal == "ordered":
            pass        # a stage issued just before on the same launch stream has waited already
        elif after_signal:
            # the current stream's last launch (the MLP backward's reduce) carries a completion signal: waiting for it
            # orders the stage after everything queued so far without an event record in the current stream
            L.check(L.lib().enerf_stream_wait_mlp32_signal(launch_stream.cuda_stream), "stream_wait_mlp32_signal")
        else:
            launch_stream.wait_stream(torch.cuda.current_stream())
    with (torch.cuda.stream(launch_stream) if launch_stream is not None else contextlib.nullcontext()):
        _rb.near_far_from_aabb(rays_o, rays_d, bufs["aabb_train"], N, model.min_near, nears, fars)
        if not budgeted:
            _rb.march_rays_train_count(rays_o, rays_d, bitfield, model.bound, dt_gamma, max_steps, N,
                                       model.cascade, model.grid_size, nears, fars, rays, counter, perturb,
                                       box | (2 if background else 0) | 8)
            total = torch.empty(2, dtype=torch.int32, pin_memory=True)
            total.copy_(counter, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            pre["pending"] = (done, total, rays_o, rays_d, perturb, dt_gamma, max_steps)
            if spec_rows:
                _rb.march_rays_train_write(rays_o, rays_d, bitfield, model.bound, dt_gamma, max_steps, N, model.cascade,
                                           model.grid_size, spec_rows, nears, fars, samples["xyzs"], samples["dirs"],
                                           samples["deltas"], rays, counter, perturb, 1)
                pre["speculative"] = (spec_rows, samples["xyzs"], samples["dirs"], samples["deltas"])
        else:
            _rb.march_rays_train_ex(rays_o, rays_d, bitfield, model.bound, dt_gamma, max_steps, N,
                                    model.cascade, model.grid_size, M, nears, fars, samples["xyzs"], samples["dirs"],
                                    samples["deltas"], rays, counter, perturb, box | (3 if background else 1) | 8)
            pre.update(samples, M=M)
        if launch_stream is not None:
            pre["ready"] = torch.cuda.Event()
            pre["ready"].record(launch_stream)
            model._last_march_event = (pre["ready"], launch_stream)
    if not budgeted and not defer:
        finish_march(model, pre)
    return pre


def finish_march(model, pre):
    """Second half of an unbudgeted march_stage, on the current stream: wait for the count (host side; the pinned
    total is the only thing read), size the sample buffers from it, run the write pass."""
    pending = pre.pop("pending", None)
    if pending is None:
        return pre
    done, total, rays_o, rays_d, perturb, dt_gamma, max_steps = pending
    done.synchronize()
    N = rays_o.shape[0]
    m = int(total[0])
    M = _cold_crop(model, m, N, max_steps)
    spec = pre.pop("speculative", None)
    if spec is not None and M <= spec[0] and m < N * max_steps:
        # the write pass already ran behind the count pass into buffers at least this large: the rows are the same
        # (nothing is dropped below N * max_steps samples, rows past the count are zero-filled either way)
        pre.update(xyzs=spec[1][:M], dirs=spec[2][:M], deltas=spec[3][:M], M=M)
        return pre
    return _write_pass(model, pre, rays_o, rays_d, perturb, dt_gamma, max_steps, M)


class _FusedRenderTrain(Function):
    @staticmethod
    def forward(ctx, rays_o, model, bg_color, pre, embeddings, *weights):
        N = rays_o.shape[0]
        dev = rays_o.device
        nears, fars, xyzs, dirs, deltas, rays, M = (pre[k] for k in ("nears", "fars", "xyzs", "dirs", "deltas", "rays",
                                                                     "M"))

        train = any(p.requires_grad for p in (embeddings,) + weights)
        sigma, rgb, sv = fnet.nerf_forward(xyzs, dirs, fnet.network_cfg(model), train, embeddings, fnet.encoder_offsets(model),
                                           *weights)
        scale = float(model.density_scale)
        sigmas = sigma if scale == 1.0 else sigma * scale
        weights_sum = torch.empty(N, dtype=torch.float32, device=dev)
        depth = torch.empty(N, dtype=torch.float32, device=dev)
        C = rgb.shape[1]
        image = torch.empty(N, C, dtype=torch.float32, device=dev)
        out_image = torch.empty(N, C, dtype=torch.float32, device=dev)
        # composite + `image + (1 - weights_sum).unsqueeze(-1) * bg_color` in one launch
        _rb.composite_rays_train_forward_blend(sigmas, rgb, deltas, rays, M, N, weights_sum, depth, image, bg_color,
                                               out_image)
        out_depth = torch.clamp(depth - nears, min=0) / (fars - nears)
        if train or (isinstance(bg_color, torch.Tensor) and ctx.needs_input_grad[2]):
            ctx.sv = sv
            ctx.rest = (sigmas, rgb, deltas, rays, weights_sum, image, bg_color, M, N, scale)
        ctx.mark_non_differentiable(out_depth)
        return out_depth, out_image

    @staticmethod
    def backward(ctx, _g_depth, g_image):
        sigmas, rgb, deltas, rays, weights_sum, image, bg_color, M, N, scale = ctx.rest
        g_image = g_image.reshape(N, rgb.shape[1]).float().contiguous()
        # ... d/d(bg) = (1 - weights_sum)[:, None] * g: asked for by the background model's per-ray colours only
        g_bg = ((1 - weights_sum).unsqueeze(-1) * g_image).view_as(bg_color) if ctx.needs_input_grad[2] else None
        if ctx.sv is None:                       # (no network parameter takes a gradient)
            return (None, None, g_bg, None) + (None,) * (len(ctx.needs_input_grad) - 4)
        # out_image = image + (1 - weights_sum)[:, None] * bg  ->  d/d(weights_sum) = -(g . bg)
        g_ws = -(g_image * bg_color).sum(-1) if isinstance(bg_color, torch.Tensor) else -(g_image.sum(-1) * bg_color)
        g_ws = g_ws.reshape(N).contiguous()
        g_sigmas = torch.zeros_like(sigmas)
        g_rgbs = torch.zeros_like(rgb)
        _rb.composite_rays_train_backward(g_ws, g_image, sigmas, rgb, deltas, rays, weights_sum, image, M, N, g_sigmas,
                                          g_rgbs)
        g = fnet.nerf_backward(ctx.sv, g_sigmas, g_rgbs, sigma_scale=scale)
        return (None, None, g_bg, None) + g


def _budget(model):
    mean_count = int(model.mean_count)
    quantum = int(getattr(model, "sample_budget_quantum", 0))
    if quantum > 0 and mean_count > 0:
        mean_count = (mean_count + quantum - 1) // quantum * quantum       # fewer distinct shapes (never fewer slots)
    return mean_count


def _next_counter(model):
    """The render's slot of the step-counter ring (raymarching.py:197-199).  Not zeroed here: march_stage tells the
    marcher to start from (0, 0) (flag bit 3) -- a fill launch per step in the middle of the training stream, ~14 us of
    it with the idle queue around it, for eight bytes."""
    # graph replay needs the counter at a fixed address; the harness copies it into the step_counter ring afterwards
    model._last_march_event = None              # (set again by whoever marches on a side stream: see early_mean_count)
    counter = getattr(model, "graph_counter", None)
    if counter is None:
        model.last_counter_slot = model.local_step % 16
        counter = model._buffers["step_counter"][model.last_counter_slot]
        model.local_step += 1
    return counter


def _pinned_ring(model):
    """The pinned host copy of the step-counter ring (made on first use)."""
    host = getattr(model, "_ring_host", None)
    if host is None:
        host = model._ring_host = torch.empty(16, 2, dtype=torch.int32, pin_memory=True)
    return host


def early_mean_count(model):
    """The sample budget update_extra_state is about to compute (mean of the window's step counters,
    nerf/renderer.py:550-552), read BEFORE the update is queued: -> (mean_count or None, total_step), or None when it
    cannot be had without waiting for the training stream.

    update_extra_state's read-back sits behind ~2 ms of sweep kernels, and the host -- which needs the budget to size and
    queue the step that follows -- used to wait for it with an empty queue behind (0.15-0.3 ms of idle device per
    update).  The window's counters are final much earlier: every march of the window has been issued, and when the last
    one ran on the side stream (the normal case: each step marches its successor's rays there) a copy queued behind it
    on that stream completes while the training stream is still a step away from the update.  The copy waits for that
    march only; the value is the same sum of the same ring slots the update kernel forms."""
    total_step = min(16, int(model.local_step))
    if total_step == 0:
        return (None, 0)                           # nothing to average: mean_count keeps its value
    staged = model.__dict__.pop("_ring_copy", None)
    if staged is not None and staged[1] == int(model.local_step) and not getattr(model, "_premarched", None):
        # stage_ring_copy: the ring was copied on the training stream in front of the window's last step (whose march-free
        # call has long been queued behind it); nothing has marched since
        staged[0].synchronize()
        counted = int(model._ring_host[:total_step, 0].to(torch.int64).sum())
        return (int(counted / total_step), total_step)
    last = getattr(model, "_last_march_event", None)
    stash = getattr(model, "_premarched", None)
    if last is None or stash:                      # the last march ran on the training stream / an unconsumed stage
        return None
    _ready, stream = last
    host = _pinned_ring(model)
    with torch.cuda.stream(stream):
        host.copy_(model._buffers["step_counter"], non_blocking=True)
        done = torch.cuda.Event()
        done.record(stream)
    done.synchronize()
    counted = int(host[:total_step, 0].to(torch.int64).sum())
    return (int(counted / total_step), total_step)


def stage_ring_copy(model):
    """The window's step counters to pinned host memory, on the CURRENT stream, now.  Where the marches run on the training
    stream itself (the one-call step carries the next batch's march in its optimizer launch: csrc/train_step.hip), early_mean_count
    has no side stream to read the ring behind: TrainHarness calls this in front of the window's LAST step -- which marches
    nothing, the update that follows voids any stage -- so that the copy is complete a whole step before the update needs it."""
    host = _pinned_ring(model)
    host.copy_(model._buffers["step_counter"], non_blocking=True)
    done = torch.cuda.Event()
    done.record()
    model._ring_copy = (done, int(model.local_step))


def prefetch_march(model, rays_o, rays_d, perturb=True, dt_gamma=0, max_steps=1024, stream=None, background=True,
                   after_signal=False):
    """Run the parameter-independent stage of the NEXT training render now (e.g. under a gradient all-reduce).  The
    result is picked up by the next render_train call on the same ray tensors; anything that changes what the stage
    reads (update_extra_state: bitfield, sample budget) must not happen in between -- the caller's responsibility.

    With `stream` the stage is issued on that HIP stream, ordered after everything queued so far on the current one
    (so it never overlaps a march of the current stream: the marcher's chunk-log workspace is shared), and runs
    concurrently with what the current stream does next (`background`: beside compute kernels, where the count pass
    runs one wavefront per SIMD; False beside collectives, where nothing competes for registers) -- the marcher is
    latency / VALU bound and hides under the
    MFMA- and HBM-bound backward kernels.  The consumer waits on the stage's event."""
    rays_o = rays_o.contiguous().view(-1, 3)
    rays_d = rays_d.contiguous().view(-1, 3)
    stash = _stash_if_free(model)
    if stash is None:
        # an unbudgeted stage is waiting for its write pass, and the marcher's chunk log (count -> write) is one
        # per-process buffer: a second count now would overwrite it.  The second render of an event step marches inline.
        return
    if stream is None:
        pre = march_stage(model, rays_o, rays_d, _next_counter(model), _budget(model), bool(perturb), False,
                          float(dt_gamma), int(max_steps), defer=True)
    else:
        pre = march_stage(model, rays_o, rays_d, _next_counter(model), _budget(model), bool(perturb), False,
                          float(dt_gamma), int(max_steps), background=background, defer=True, launch_stream=stream,
                          after_signal=after_signal)
    pre["slot"] = getattr(model, "last_counter_slot", None)
    stash[_stage_key(rays_o, rays_d, perturb, dt_gamma, max_steps)] = pre      # (an event step stashes both of its renders)


def premarch_count(model, rays_o, rays_d, perturb=True, dt_gamma=0, max_steps=1024):
    """near/far + the marcher's count pass and scan for the coming training render, on the current stream, before the
    sample budget is known on the host: TrainHarness queues it between density_update.update_begin and update_end, so
    the device has work while the host waits for the update's read-back (neither pass reads the budget: rays, counter
    and chunk log do not depend on M).  The render picks the stage up and runs the write pass with the budget it then
    has -- the same launches as march_rays_train_ex, in the same order."""
    rays_o = rays_o.contiguous().view(-1, 3)
    rays_d = rays_d.contiguous().view(-1, 3)
    N = rays_o.shape[0]
    pre = _ray_bufs(N, rays_o.device)
    counter = _next_counter(model)
    bufs = model._buffers
    _rb.near_far_from_aabb(rays_o, rays_d, bufs["aabb_train"], N, model.min_near, pre["nears"], pre["fars"])
    _rb.march_rays_train_count(rays_o, rays_d, bufs["density_bitfield"], model.bound, float(dt_gamma), int(max_steps), N,
                               model.cascade, model.grid_size, pre["nears"], pre["fars"], pre["rays"], counter,
                               bool(perturb), occupied_box_flag(model) | 8)
    pre.update(counter=counter, counted=(rays_o, rays_d, bool(perturb), float(dt_gamma), int(max_steps)),
               slot=getattr(model, "last_counter_slot", None))
    model._premarched = {_stage_key(rays_o, rays_d, perturb, dt_gamma, max_steps): pre}


def _finish_counted(model, pre):
    """Write pass of a premarch_count stage, with the budget the host has by now (march_stage's budgeted branch)."""
    rays_o, rays_d, perturb, dt_gamma, max_steps = pre.pop("counted")
    mean_count = _budget(model)
    if mean_count <= 0:                         # no budget after all (first window): the reference's crop of N * max_steps
        M = _cold_crop(model, int(pre["counter"][0].item()), rays_o.shape[0], max_steps)
    else:
        M = _budget_rows(mean_count)
    return _write_pass(model, pre, rays_o, rays_d, perturb, dt_gamma, max_steps, M)


def render_train(model, rays_o, rays_d, bg_color, perturb, force_all_rays, dt_gamma, max_steps):
    """-> depth [N], image [N,C] (+ the step counter bookkeeping of run_cuda)."""
    pre = _take_or_march(model, rays_o, rays_d, perturb, dt_gamma, max_steps, force_all_rays=force_all_rays)
    return _FusedRenderTrain.apply(rays_o, model, bg_color, pre, *fnet.network_params(model))


def _check_cold_stage(model, pre, rays_o, rays_d, perturb, dt_gamma, max_steps):
    """A stage marched by the one-call step of the cold window into `cap` reserved rows, budgeted-style, is valid iff
    nothing was dropped, i.e. iff the count that came back (behind the march, on its stream) fits.  Waits for that count
    (the only host wait of such a step), records the rows for later reservations, repairs the stage when it does not fit:
    count, scan and ray table do not depend on the rows (same counter slot, nothing marched since), so the write pass
    alone is repeated into buffers of the exact size -- what finish_march does for a speculative write pass that did not
    fit.  -> the stage to use."""
    done, host, cap = pre.pop("cold_check")[:3]
    # the count arrives in pinned memory behind the march (an 8-byte copy on its stream): the host watches the two words
    # it pre-set to -1 instead of sleeping on the event -- the wake-up of an event wait is 10-20 us, in which the device,
    # which has nothing queued yet, idles (the cold window's steps: 11 of the driver's 20)
    # The watch is bounded by a few march times (2 ms; a 4096-ray march is ~0.13 ms) and only tried where the count is
    # stored by the kernel itself (MIRROR_COUNT): a count that arrives by an asynchronous copy is ordered by the event
    # anyway.  A watch that runs out -- pinned memory that is not host-coherent while the kernel runs
    # (HIP_HOST_COHERENT=0) -- is remembered on the model and every later step goes straight to the event.
    hv = host.numpy()
    if hv[0] < 0 or hv[1] < 0:
        if MIRROR_COUNT and not getattr(model, "_cold_watch_failed", False):
            import time as _time
            t_end = _time.perf_counter() + 0.002
            while (hv[0] < 0 or hv[1] < 0) and _time.perf_counter() < t_end:
                pass
            if hv[0] < 0 or hv[1] < 0:
                model._cold_watch_failed = True
        if hv[0] < 0 or hv[1] < 0:
            done.synchronize()
    rows = _cold_crop(model, int(hv[0]), rays_o.shape[0], max_steps)
    if rows <= cap:
        return pre
    return _write_pass(model, dict(pre), rays_o, rays_d, perturb, dt_gamma, max_steps, rows)


def _stage_key(rays_o, rays_d, perturb, dt_gamma, max_steps):
    return (rays_o.data_ptr(), rays_d.data_ptr(), rays_o.shape[0], bool(perturb), float(dt_gamma), int(max_steps))


def _stash_if_free(model):
    """The stash the next stages go into, or None while an unbudgeted stage waits there for its write pass (see
    prefetch_march: nothing else may be marched then)."""
    stash = getattr(model, "_premarched", None)
    if not isinstance(stash, dict):
        stash = model._premarched = {}
    return None if any("pending" in p for p in stash.values()) else stash


def _take_premarched(model, rays_o, rays_d, perturb, dt_gamma, max_steps, defer_cold_check=False):
    stash = getattr(model, "_premarched", None)
    if not stash:
        return None
    pre = stash.pop(_stage_key(rays_o, rays_d, perturb, dt_gamma, max_steps), None)
    if pre is None:
        stash.clear()                                # marched for rays that are not coming: drop, march afresh
        return None
    if "cold_check" in pre:
        ready = pre.pop("ready", None)
        if ready is not None:
            torch.cuda.current_stream().wait_event(ready)
        if defer_cold_check:
            return pre                               # the one-call step checks right before its call (host work first)
        return _check_cold_stage(model, pre, rays_o, rays_d, perturb, dt_gamma, max_steps)
    if "counted" in pre:
        return _finish_counted(model, pre)
    ready = pre.pop("ready", None)
    if ready is not None:                       # marched on a side stream, into buffers of this stream's pool (see
        torch.cuda.current_stream().wait_event(ready)      # march_stage): order this stream after it, nothing else
    return finish_march(model, pre)              # unbudgeted stage: the write pass runs here, sized from the count


def _take_or_march(model, rays_o, rays_d, perturb, dt_gamma, max_steps, defer_cold_check=False, force_all_rays=False):
    """The batch's samples: the stage marched ahead for these rays, or a march now (always, with force_all_rays: a stage
    marched ahead is dropped)."""
    pre = _take_premarched(model, rays_o, rays_d, perturb, dt_gamma, max_steps, defer_cold_check=defer_cold_check)
    if pre is not None and not force_all_rays:
        model.rendered_counter_slot = pre["slot"]
        return pre
    counter = _next_counter(model)
    model.rendered_counter_slot = getattr(model, "last_counter_slot", None)
    return march_stage(model, rays_o, rays_d, counter, _budget(model), bool(perturb), bool(force_all_rays), float(dt_gamma),
                       int(max_steps))


FUSED_COMPOSITE = True        # train_step_mse: compositing forward + MSE backward as one launch
MIRROR_COUNT = True           # cold window: the march's count goes straight to pinned host memory (next_count_host)
import os as _os
SKIP_PADDING_ROWS = _os.environ.get("ENERF_SKIP_PADDING_ROWS", "1") != "0"      # raw renders: the MLP kernels skip the sample budget's unfilled rows (device-side count)


def render_train_raw(model, rays_o, rays_d, bg_color=1, perturb=True, dt_gamma=0, max_steps=1024, composite=True):
    """Forward half of a training render without autograd: -> (image [N,C] blended with bg_color, ctx).  Feed the
    gradient of whatever loss was computed on `image` to backward_raw(ctx, ...).  No depth.  composite=False leaves
    the compositing to backward_raw(target=...), which then runs it fused with its backward (the image is valid once
    that call is queued)."""
    rays_o = rays_o.contiguous().view(-1, 3)
    rays_d = rays_d.contiguous().view(-1, 3)
    N = rays_o.shape[0]
    dev = rays_o.device
    with torch.no_grad():
        pre = _take_or_march(model, rays_o, rays_d, perturb, dt_gamma, max_steps)
        xyzs, dirs, deltas, rays, M = (pre[k] for k in ("xyzs", "dirs", "deltas", "rays", "M"))
        params = fnet.network_params(model)
        sigma, rgb, sv = fnet.nerf_forward(xyzs, dirs, fnet.network_cfg(model), True, params[0],
                                           fnet.encoder_offsets(model), *params[1:],
                                           valid_rows=pre["counter"] if SKIP_PADDING_ROWS else None)
        scale = float(model.density_scale)
        sigmas = sigma if scale == 1.0 else sigma * scale
        weights_sum = torch.empty(N, dtype=torch.float32, device=dev)
        C = rgb.shape[1]
        image = torch.empty(N, C, dtype=torch.float32, device=dev)
        out_image = torch.empty(N, C, dtype=torch.float32, device=dev)
        if isinstance(bg_color, torch.Tensor):
            bg_color = bg_color.detach().to(torch.float32).contiguous()
        if composite:
            _rb.composite_rays_train_forward_blend(sigmas, rgb, deltas, rays, M, N, weights_sum, None, image, bg_color,
                                                   out_image)
    ctx = dict(sv=sv, sigmas=sigmas, rgb=rgb, deltas=deltas, rays=rays, weights_sum=weights_sum, image=image,
               out_image=out_image, bg=bg_color, counter=pre["counter"], M=M, N=N, scale=scale, composited=composite)
    return out_image, ctx


def backward_raw(ctx, g_image=None, target=None, upstream=1.0, loss_out=None, raw=False, defer_table=0,
                 after_mlp=None, frames=None):
    """Backward half.  Either g_image = d loss / d image [N,C], or target [N,C] for loss = mean((image - target)^2) *
    upstream (gradient and, with loss_out, value formed inside the composite backward), or frames = dict(pixels [N, C or
    C + 1], weight, err_out [N] or None, gt_out [N,C] or None) for the frame term (frame_term.frame_term_statement; the
    render came from render_train_raw(composite=False), loss_out is added into).  -> the gradients of
    fused_network.network_params(model) (raw=True: (embedding gradient, flat dW), see fused_network.nerf_backward);
    the embedding gradient is None when it was added into an existing embeddings.grad."""
    N, M = ctx["N"], ctx["M"]
    C = ctx["rgb"].shape[1]
    with torch.no_grad():
        g_sigmas = torch.empty_like(ctx["sigmas"])
        g_rgbs = torch.empty_like(ctx["rgb"])
        if frames is not None:
            assert not ctx["composited"], "backward_raw(frames=...) needs render_train_raw(composite=False)"
            pixels = frames["pixels"]
            _rb.composite_rays_train_fwd_bwd_frames(ctx["sigmas"], ctx["rgb"], ctx["deltas"], ctx["rays"], M, N,
                                                    ctx["weights_sum"], ctx["image"], ctx["bg"], ctx["out_image"],
                                                    pixels.contiguous().view(-1, pixels.shape[-1]),
                                                    float(frames.get("weight", 1.0)), ctx["counter"], g_sigmas, g_rgbs,
                                                    frames.get("gt_out"), frames.get("err_out"), loss_out)
        elif target is not None and not ctx["composited"]:
            _rb.composite_rays_train_fwd_bwd_mse(ctx["sigmas"], ctx["rgb"], ctx["deltas"], ctx["rays"], M, N,
                                                 ctx["weights_sum"], ctx["image"], ctx["bg"], ctx["out_image"],
                                                 target.contiguous().view(-1, C), 2.0 * float(upstream) / (C * N),
                                                 ctx["counter"], g_sigmas, g_rgbs, loss_out)
        elif target is not None:
            _rb.composite_rays_train_backward_mse(ctx["out_image"], target.contiguous().view(-1, C),
                                                  2.0 * float(upstream) / (C * N), ctx["bg"], ctx["counter"],
                                                  ctx["sigmas"], ctx["rgb"], ctx["deltas"], ctx["rays"],
                                                  ctx["weights_sum"], ctx["image"], M, N, g_sigmas, g_rgbs, loss_out)
        else:
            assert ctx["composited"], "render_train_raw(composite=False) needs backward_raw(target=...)"
            _rb.composite_rays_train_backward_mse(g_image.detach().to(torch.float32).contiguous().view(-1, C), None,
                                                  1.0, ctx["bg"], ctx["counter"], ctx["sigmas"], ctx["rgb"],
                                                  ctx["deltas"], ctx["rays"], ctx["weights_sum"], ctx["image"], M, N,
                                                  g_sigmas, g_rgbs, None)
        return fnet.nerf_backward(ctx["sv"], g_sigmas, g_rgbs, sigma_scale=ctx["scale"], raw=raw, owner=True,
                                  defer_table=defer_table, after_mlp=after_mlp)


def train_step_mse(model, rays_o, rays_d, target, bg_color=1, perturb=True, dt_gamma=0, max_steps=1024, upstream=1.0,
                   after_forward=None, loss_out=None, raw=False, defer_table=False, after_mlp_backward=None):
    """Forward AND backward of a training render under loss = mean((image - target)^2) * upstream, without autograd:
    -> (image [N,C], gradients of fused_network.network_params(model) in that order; the first is None when the
    embedding gradient was added straight into the parameter's .grad).

    For loops whose loss is the reference's default (nerf/utils.py:628, MSE): the loss gradient and the blend's
    d/d(weights_sum) are formed inside the composite backward kernel, which also zero-fills what it does not write;
    depth is not computed.  What is skipped relative to render_train + autograd: the engine round trip, its
    AccumulateGrad nodes, ~18 elementwise / fill launches.  `after_forward()` is called once the forward is queued,
    `after_mlp_backward()` once both MLP backward kernels are (the hash table's backward and the optimizer follow);
    `loss_out` (a zeroed device scalar) receives the loss value from the backward kernel itself; raw=True returns the
    gradients as (embedding gradient, flat MLP dW accumulator) -- see fused_network.nerf_backward."""
    out_image, ctx = render_train_raw(model, rays_o, rays_d, bg_color, perturb, dt_gamma, max_steps,
                                      composite=not FUSED_COMPOSITE)
    if after_forward is not None:
        after_forward()                         # e.g. prefetch_march of the next batch on a side stream
    return out_image, backward_raw(ctx, target=target, upstream=upstream, loss_out=loss_out, raw=raw,
                                   defer_table=ctx["M"] if defer_table else 0, after_mlp=after_mlp_backward)


def train_step_frames(model, rays_o, rays_d, pixels, bg_color, weight=1.0, perturb=True, dt_gamma=0, max_steps=1024,
                      after_forward=None, loss_out=None, raw=False, defer_table=False, after_mlp_backward=None,
                      gt_out=None):
    """train_step_mse's twin for the frame term (Trainer.train_step, nerf/utils.py:595-604,634): `pixels` [.., C] or, with
    an alpha, [.., C + 1] -- mixed on `bg_color` inside the compositing launch -- and loss = weight * mean over rays of the
    per-ray squared error.  -> (image [N,C], err [N] the per-ray error, gradients as train_step_mse returns them).
    `loss_out` (a device scalar) has the loss ADDED; `gt_out` [N,C] receives the mixed ground truth."""
    out_image, ctx = render_train_raw(model, rays_o, rays_d, bg_color, perturb, dt_gamma, max_steps, composite=False)
    if after_forward is not None:
        after_forward()
    err = torch.empty(ctx["N"], dtype=torch.float32, device=out_image.device)
    grads = backward_raw(ctx, frames=dict(pixels=pixels, weight=weight, err_out=err, gt_out=gt_out), loss_out=loss_out,
                         raw=raw, defer_table=ctx["M"] if defer_table else 0, after_mlp=after_mlp_backward)
    return out_image, err, grads


# ---------------------------------------------------------------------------------------------------------------------
# The closed-form steps as ONE library call each (csrc/train_step.hip: enerf_train_step_mse, enerf_train_step_events).  The
# same entry points in the same order as train_step_mse above / events.train_step_events_manual + FusedAdam.step_grid_table,
# issued by the library itself: what is left on this side is the bookkeeping (stage hand-over, buffers, optimizer step
# counts), written once for both steps.
import ctypes as _ct

NATIVE_STEP = _os.environ.get("ENERF_NATIVE_STEP", "1") != "0"
_vp, _u32, _f32c = _ct.c_void_p, _ct.c_uint32, _ct.c_float


def _fields(ctype, *names):
    return [(n, ctype) for n in names]


# The blocks of enerf_train_step_args / enerf_step_render / enerf_event_step_args (include/enerf_hip.h), each named once
_MLP_SCRATCH = ("feats", "h32", "fb_s", "fb_c", "sigma", "rgb", "g_sigmas", "g_rgbs", "dx32", "dfeat")
_NEXT_BUFS = ("nears", "fars", "xyzs", "dirs", "deltas", "rays", "counter")
_SMALL = ("small_p", "small_g", "small_m", "small_v", "small_n", "small_lr", "small_step")
_HEAD = [("struct_bytes", _u32), ("mlp_precision", _ct.c_int), ("stream", _vp), ("side_stream", _vp)]
_SAMPLES = _fields(_u32, "N", "M") + _fields(_vp, "xyzs", "dirs", "deltas", "rays", "counter")
_NETS = (_fields(_vp, "embeddings", "offsets") + _fields(_f32c, "level_scale_log2", "bound", "inv_two_bound")
         + _fields(_u32, "base_resolution", "gridtype") + _fields(_vp, "wseg_s", "wseg_c", "dwseg_s", "dwseg_c")
         + _fields(_u32, "nh_s", "nh_c", "w0_cols_c", "out_c"))
_NEXT_RAYS, _NEXT_SIZE = _fields(_vp, "next_rays_o", "next_rays_d"), _fields(_u32, "next_N", "next_M")
_NEXT_OUT = _fields(_vp, *("next_" + n for n in _NEXT_BUFS))
_EVERY_ROW, _MARCH_CARRIED = 4, 1         # ENERF_STEP_EVERY_ROW (flags), ENERF_STEP_MARCH_CARRIED (report)
_MARCH = _fields(_vp, "aabb", "bitfield") + _fields(_f32c, "min_near", "dt_gamma")
_MARCH_U32 = _fields(_u32, "cascade", "grid_size", "max_steps", "perturb", "march_flags")
_OPTIM = (_fields(_vp, "table", "table_grad", "table_m", "table_v") + _fields(_f32c, "lr", "beta1", "beta2", "eps")
          + _fields(_u32, "table_step", "n_small") + _fields(_vp, *_SMALL) + _fields(_u32, "flags", "report"))


def _scratch_fields(*images):             # a render's scratch: the MLP set with the image buffers where the header has them
    return _fields(_vp, *_MLP_SCRATCH[:6], "weights_sum", "image", "out_image", *images, *_MLP_SCRATCH[6:])


class _StepArgs(_ct.Structure):           # enerf_train_step_args
    _fields_ = (_HEAD + _SAMPLES + [("target", _vp), ("bg_scalar", _f32c), ("grad_scale", _f32c), ("loss", _vp)] + _NETS
                + _scratch_fields() + _NEXT_RAYS + _MARCH + _NEXT_SIZE + _MARCH_U32 + _NEXT_OUT + [("next_count_host", _vp)] + _OPTIM)


class _StepRender(_ct.Structure):         # enerf_step_render
    _fields_ = _SAMPLES + _scratch_fields("g_image") + _NEXT_RAYS + _NEXT_SIZE + _NEXT_OUT


class _EventStepArgs(_ct.Structure):      # enerf_event_step_args
    _fields_ = (_HEAD + [("r", _StepRender * 2), ("bg_color", _vp), ("pols", _vp), ("use_luma", _u32), ("linlog", _u32),
                         ("C_thres", _f32c), ("log_thres", _f32c), ("upstream", _f32c), ("delta", _vp), ("loss", _vp)]
                + _NETS + _MARCH + _MARCH_U32 + [("reserved0", _u32)] + _OPTIM + _fields(_vp, *("m_" + n for n in _MLP_SCRATCH)))


COLD_NATIVE = True            # the one-call step also serves the window before the first sample budget (see cold_capacity)
MERGE_EVENT_RENDERS = True    # the one-call event step runs both renders' samples as one batch of 2 M rows (flags bit 1)


def cold_capacity(rows, N, max_steps, floor=0):
    """Rows reserved for a march of the cold window (no sample budget yet: nothing may be dropped), from an earlier
    render's row count: + 1/20, rounded up to 4 Ki rows, and never below what an earlier step of the window reserved
    (`floor`) -- the persistent buffers of the one-call step are keyed by these sizes, so the reservation has to settle
    after a step or two.  A march that turns out to need more gets its write pass repeated at the exact size
    (_repair_cold_stage), which costs one small launch."""
    c = rows + rows // 20
    c = (c + 4095) // 4096 * 4096
    return min(max(c, floor), N * max_steps)


def native_step_supported(model, rays_o, rays_d, opt, data_parallel=False):
    """The one-call step serves the closed-form RGB step with unit density scale and the fused optimizer: in the steady
    state (a sample budget exists) and -- one GPU -- in the cold window from its second step on, where the rows of an
    earlier render size the buffers (cold_capacity) and the count that comes back is checked before the stage is used."""
    ready = _budget(model) > 0 or (COLD_NATIVE and not data_parallel and int(getattr(model, "_cold_rows", 0)) > 0)
    return (NATIVE_STEP and ready and float(model.density_scale) == 1.0
            and hasattr(opt, "grid_table_args") and supported(model, rays_o, rays_d, 1, 0))


def native_events_supported(model, data, loss_opt, opt, normalised=False):
    """What enerf_train_step_events serves: the steady state (a sample budget exists) of the event-only step with the
    fused loss kernel (fp32, one background colour: a batch of one image; the normalised loss, C_thres == -1, only where
    the caller asks for it with `normalised`), unit density scale, the fused optimizer, default march parameters."""
    ro, rd = data["rays_evs_o1"], data["rays_evs_d1"]
    return (NATIVE_STEP and _budget(model) > 0 and float(model.density_scale) == 1.0 and hasattr(opt, "grid_table_plan")
            and loss_opt.event_only and (loss_opt.C_thres != -1 or normalised) and not loss_opt.render_kwargs
            and int(getattr(loss_opt, "out_dim_color", 3)) == channels(model)
            and (not loss_opt.use_luma or channels(model) == 3)              # luma is a three-channel operation
            and data["images"].shape[0] == 1 and data["pols"].dtype == torch.float32 and data["pols"].is_cuda
            and data["rays_evs_o1"].shape == data["rays_evs_o2"].shape
            and data["pols"].numel() * 3 == data["rays_evs_o1"].numel()
            and supported(model, ro.contiguous().view(-1, 3), rd.contiguous().view(-1, 3), 1, 0)
            and supported(model, data["rays_evs_o2"].contiguous().view(-1, 3),
                          data["rays_evs_d2"].contiguous().view(-1, 3), 1, 0))


# ---- what a context holds: everything of a native step that does not change from step to step, built once per (rays,
# sample budget) -- i.e. once per update_extra_state window: the step's scratch buffers, two sets of sample buffers for the
# march that runs ahead (the step reads one set while the next march fills the other), the weight / gradient pointer arrays,
# and the argument struct with its constant fields filled in.  (20 torch.empty calls and ~60 struct fields per step
# otherwise: most of the host's share of a step once the launches themselves come from C.)
def _ctx_for(model, attr, struct, sizes, dev):
    """-> (context, whether it was just built with only the shared parts in it).  Keyed by `sizes` and the networks."""
    params = fnet.network_params(model)
    emb, weights = params[0], params[1:]
    kind = fnet.kind_of(model)
    arch = fnet._ARCH[kind]
    prec = model.__dict__.get("mlp_precision")
    prec = arch["prec"] if prec is None else int(prec)
    out_c = weights[-1].shape[0] if kind == "linear" else 3
    key = sizes + (kind, prec, out_c, emb.data_ptr(), tuple(w.data_ptr() for w in weights), dev)
    ctx = model.__dict__.get(attr)
    if ctx is not None and ctx["key"] == key:
        return ctx, False
    import numpy as _np
    enc = model._modules["encoder"]
    bufs = model._buffers
    seg_s, seg_c = fnet._weight_segments(kind, weights)
    dw, (dseg_s, dseg_c) = fnet._grad_segments(kind, dev, out_c)
    a = struct()
    a.struct_bytes = _ct.sizeof(struct)
    a.mlp_precision = -1 if prec is None else prec
    a.embeddings, a.offsets = emb.data_ptr(), enc._buffers["offsets"].data_ptr()
    a.level_scale_log2 = float(_np.log2(enc.per_level_scale))
    a.bound, a.inv_two_bound = float(model.bound), float(_np.float32(1.0) / _np.float32(2 * model.bound))
    a.base_resolution, a.gridtype = int(enc.base_resolution), int(enc.gridtype_id)
    a.wseg_s, a.wseg_c = _ct.cast(seg_s, _vp), _ct.cast(seg_c, _vp)
    a.dwseg_s, a.dwseg_c = _ct.cast(dseg_s, _vp), _ct.cast(dseg_c, _vp)
    a.nh_s, a.nh_c, a.w0_cols_c, a.out_c = arch["nh_s"], arch["nh_c"], arch["w0c"], out_c
    a.aabb, a.bitfield = bufs["aabb_train"].data_ptr(), bufs["density_bitfield"].data_ptr()
    a.min_near = float(model.min_near)
    a.cascade, a.grid_size = int(model.cascade), int(model.grid_size)
    a.table = emb.data_ptr()
    ctx = dict(key=key, seg=(seg_s, seg_c), dseg=(dseg_s, dseg_c), dw=dw, grads=fnet.unpack_weight_grads(dw, out_c, kind),
               a=a, emb=emb, weights=weights, kind=kind, arch=arch, out_c=out_c)
    model.__dict__[attr] = ctx
    return ctx, True


def _mlp_scratch(rows, arch, out_c, new):
    """The scratch of `rows` rows through the networks (enerf_hip.h: feats .. dfeat); new(name, *shape) -> the tensor."""
    Mp = (rows + 31) // 32 * 32
    shapes = dict(feats=(16, Mp, 2), h32=(rows, 32), fb_s=(arch["nh_s"], Mp, 64), fb_c=(arch["nh_c"], Mp, 64), sigma=(rows,),
                  rgb=(rows, out_c), g_sigmas=(rows,), g_rgbs=(rows, out_c), dx32=(rows, 32), dfeat=(16, Mp, 2))
    return {name: new(name, *shape) for name, shape in shapes.items()}


def _stage_set(Nn, Mn, dev, samples=None):
    """One set of buffers a march of Nn rays into Mn rows fills (`samples`: its xyzs / dirs / deltas, where they exist)."""
    return dict(_ray_bufs(Nn, dev), M=Mn, **(_sample_bufs(Mn, dev) if samples is None else samples))


def _native_ctx(model, N, M, Nn, Mn, dev):
    ctx, new = _ctx_for(model, "_native_ctx", _StepArgs, (N, M, Nn, Mn), dev)
    if not new:
        return ctx
    f32 = dict(dtype=torch.float32, device=dev)
    a = ctx["a"]
    t = _mlp_scratch(M, ctx["arch"], ctx["out_c"], lambda name, *shape: torch.empty(*shape, **f32))
    C = ctx["out_c"]
    t.update(weights_sum=torch.empty(N, **f32), image=torch.empty(N, C, **f32), out_image=torch.empty(N, C, **f32))
    for name, buf in t.items():
        setattr(a, name, buf.data_ptr())
    a.N, a.M = N, M
    a.bg_scalar, a.grad_scale = 1.0, 2.0 / (C * N)
    ctx.update(t=t, stages=[_stage_set(Nn, Mn, dev) for _ in range(2)] if Nn else [], flip=0,
               out_image=t["out_image"])
    return ctx


def _native_events_ctx(model, N, Ms, Nn, Mn, luma, dev):
    ctx, new = _ctx_for(model, "_native_events_ctx", _EventStepArgs, (N, Ms, Nn, Mn, luma), dev)
    if not new:
        return ctx
    f32 = dict(dtype=torch.float32, device=dev)
    a, arch, out_c = ctx["a"], ctx["arch"], ctx["out_c"]
    fresh = lambda name, *shape: torch.empty(*shape, **f32)
    tm = None
    if MERGE_EVENT_RENDERS and Ms[0] == Ms[1]:
        tm = _mlp_scratch(2 * Ms[0], arch, out_c, fresh)     # (2 M is a multiple of 256: no padding of the level-major rows)
        for name, buf in tm.items():
            setattr(a, "m_" + name, buf.data_ptr())
    # the two renders' sample buffers of one stage generation are the halves of ONE allocation: a step that consumes both
    # finds the second render's rows right behind the first's M (merged layout, see train_step_events_native)
    pairs = [_sample_bufs(2 * Mn, dev) for _ in range(2 if Nn else 0)]
    ts, stages = [], []
    for q, M in enumerate(Ms):
        def half(name, *shape):
            # the per-render scratch (steps whose two stages were not marched together: right after an update) is the two
            # halves of the merged allocations, each half in the per-render shape: no second set of buffers
            flat = tm[name].view(-1)
            n = flat.numel() // 2
            return flat[q * n:(q + 1) * n].view(*shape)
        t = _mlp_scratch(M, arch, out_c, fresh if tm is None else half)
        t.update(weights_sum=torch.empty(N, **f32), image=torch.empty(N, out_c, **f32),
                 out_image=torch.empty(N, out_c, **f32), g_image=torch.empty(N, out_c, **f32))
        ts.append(t)
        a.r[q].N, a.r[q].M = N, M
        for name, buf in t.items():
            setattr(a.r[q], name, buf.data_ptr())
        stages.append([_stage_set(Nn, Mn, dev, {k: v[q * Mn:(q + 1) * Mn] for k, v in pb.items()}) for pb in pairs])
    delta = torch.empty(1, N, 1 if luma else out_c, **f32)
    a.delta = delta.data_ptr()
    ctx.update(t=ts, tm=tm, stages=stages, flip=[0, 0], delta=delta)
    return ctx


# ---- the per-step bookkeeping both drivers share
def _fill_step(ctx, a):
    emb = ctx["emb"]
    if emb.grad is None:                    # the dense part of the table's gradient (levels too small to bin)
        emb.grad = torch.zeros_like(emb)
    a.stream = L.stream_handle()
    a.table_grad = emb.grad.data_ptr()


def _fill_samples(r, pre):
    r.xyzs, r.dirs, r.deltas = pre["xyzs"].data_ptr(), pre["dirs"].data_ptr(), pre["deltas"].data_ptr()
    r.rays, r.counter = pre["rays"].data_ptr(), pre["counter"].data_ptr()
    r.next_rays_o = None


def _step_flags(bits):
    """The call's `flags`: with SKIP_PADDING_ROWS off the grid and MLP launches take every row of the budget (the compositing
    needs the counter either way)."""
    return bits if SKIP_PADDING_ROWS else bits | _EVERY_ROW


def _fill_march(a, model, side_stream, perturb, dt_gamma, max_steps, more_flags=0):
    a.side_stream = side_stream.cuda_stream
    a.dt_gamma, a.max_steps, a.perturb = float(dt_gamma), int(max_steps), 1 if perturb else 0
    a.march_flags = occupied_box_flag(model) | 3 | 8 | more_flags


def _next_stage(r, sets, flip, pre, counter, slot, no, nd):
    """The next march of (no, nd) into the buffer set the current batch `pre` is NOT using (sets[flip] is looked at first),
    described in r's next_* fields -> (the stage, its set's index: the next call looks at the other one first)."""
    which = flip ^ 1 if any(pre[k] is sets[flip][k] for k in ("xyzs", "rays")) else flip
    nxt = _Stage(sets[which])
    nxt["counter"], nxt["slot"] = counter, slot
    r.next_rays_o, r.next_rays_d, r.next_N, r.next_M = no.data_ptr(), nd.data_ptr(), no.shape[0], nxt["M"]
    for name in _NEXT_BUFS:
        setattr(r, "next_" + name, nxt[name].data_ptr())
    return nxt, which


def _fill_optimizer(ctx, a, opt):
    """The optimizer block: host arrays (pointers, sizes, learning rates, step counts of the MLP weights) built once per
    context and optimizer, the scalars of this step (which advances the step counts)."""
    plan = ctx.get("plan")
    if plan is None or ctx.get("plan_opt") is not opt:
        plan = ctx["plan"] = opt.grid_table_plan(ctx["emb"], list(ctx["weights"]), list(ctx["grads"]))
        ctx["plan_opt"] = opt
        st = plan.state
        a.table_m, a.table_v = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
        a.n_small = plan.arrays[0]
        for name, arr in zip(_SMALL, plan.arrays[1:]):
            setattr(a, name, _ct.cast(arr, _vp) if arr is not None else None)
    a.lr, a.beta1, a.beta2, a.eps, a.table_step = plan()


def _call(entry, a):
    """The one call -> whether the next marches rode in its own launches, on this stream (no event to wait for then)."""
    L.check(getattr(L.lib(), "enerf_" + entry)(_ct.byref(a)), entry)
    return bool(a.report & _MARCH_CARRIED)


def _count_launches(points):
    """The launch counters bench.py reads: the library issued one grid_encode_forward / backward over `points` rows."""
    from .backends import _gridencoder as _gbk
    _gbk.STATS["fwd_points"] += points
    _gbk.STATS["budget_rows"] += points
    _gbk.STATS["fwd_calls"] += 1
    _gbk.STATS["bwd_points"] += points
    _gbk.STATS["bwd_calls"] += 1
    _gbk.LIFETIME["fwd_points"] += points
    _gbk.LIFETIME["fwd_calls"] += 1


def _hand_over(model, stash, staged, side_stream, carried):
    """The stages just marched go into the stash, with the event their consumer waits for -> that event (None: carried)."""
    ready = None
    if not carried:
        ready = torch.cuda.Event()
        ready.record(side_stream)
    for key, nxt in staged:
        nxt["ready"] = ready
        stash[key] = nxt
    model._last_march_event = None if carried else (ready, side_stream)
    return ready


def _install_grads(ctx):
    """p.grad of the MLP weights: views of the context's flat gradient buffer."""
    views = ctx.get("grad_views")
    if views is None:
        views = ctx["grad_views"] = [g.view_as(p) for p, g in zip(ctx["weights"], ctx["grads"])]
    for p, g in zip(ctx["weights"], views):
        if p.grad is not g:
            p.grad = g


def train_step_native(model, rays_o, rays_d, target, opt, next_rays=None, side_stream=None, loss_out=None, perturb=True,
                      dt_gamma=0, max_steps=1024, raw=False, defer_dp=False):
    """One closed-form RGB step (loss = mean((image - target)^2), white background) through enerf_train_step_mse:
    render of this batch (marched ahead of time when the previous step asked for it) + backward + the optimizer, and the
    march of `next_rays` = (rays_o, rays_d) on `side_stream` behind the MLP backward.  -> blended image [N,C] (a buffer
    that the next step of the same shape overwrites).  Gradients of the MLP weights are left in p.grad (views of one flat
    buffer, likewise reused), the table's dense gradient buffer comes back clean; the optimizer's step counts advance.
    raw=True (data parallel): the table's gradient is summed into the dense buffer `embeddings.grad` and NO optimizer
    runs -- -> (image, flat MLP dW buffer); the caller averages both over the ranks and steps the optimizer."""
    rays_o = rays_o.contiguous().view(-1, 3)
    rays_d = rays_d.contiguous().view(-1, 3)
    N, dev = rays_o.shape[0], rays_o.device
    with torch.no_grad():
        pre = _take_or_march(model, rays_o, rays_d, perturb, dt_gamma, max_steps, defer_cold_check=True)
        stash = no = nd = nxt_counter = nxt_slot = None
        cold_next = False
        Nn = Mn = 0
        if next_rays is not None and side_stream is not None:
            stash = _stash_if_free(model)
        if stash is not None:
            no, nd = next_rays[0].contiguous().view(-1, 3), next_rays[1].contiguous().view(-1, 3)
            Nn = no.shape[0]
            mc = _budget(model)
            cold_next = mc <= 0
            if cold_next:                    # cold window: rows reserved from the last render whose count is known
                Mn = model._cold_cap = cold_capacity(int(model._cold_rows), Nn, int(max_steps),
                                                     int(getattr(model, "_cold_cap", 0)))
            else:
                Mn = _budget_rows(mc)
            nxt_counter = _next_counter(model)
            nxt_slot = getattr(model, "last_counter_slot", None)

        def prepare(pre):
            ctx = _native_ctx(model, N, pre["M"], Nn, Mn, dev)
            a = ctx["a"]
            _fill_step(ctx, a)
            _fill_samples(a, pre)
            a.target = target.contiguous().view(-1, ctx["out_c"]).data_ptr()
            a.loss = None if loss_out is None else loss_out.data_ptr()
            # (bit 1: the sharded tail with an owner range set -- this rank's slice of the table stays as record lists)
            a.flags = _step_flags((3 if defer_dp else 1) if raw else 0)
            nxt, which = None, 0
            if stash is not None:
                # (bit 4: this march stays on the side stream -- the cold window reads its count back behind it there)
                _fill_march(a, model, side_stream, perturb, dt_gamma, max_steps, 16 if cold_next else 0)
                nxt, which = _next_stage(a, ctx["stages"], ctx["flip"], pre, nxt_counter, nxt_slot, no, nd)
            return ctx, a, nxt, which

        ctx, a, nxt, which = prepare(pre)
        if "cold_check" in pre:
            # everything above was host work that did not need the count; only now is it waited for
            fixed = _check_cold_stage(model, pre, rays_o, rays_d, perturb, dt_gamma, max_steps)
            if fixed is not pre:
                pre = fixed
                ctx, a, nxt, which = prepare(pre)
        M = pre["M"]
        if nxt is not None:
            ctx["flip"] = which ^ 1
        if raw:
            a.n_small = 0
            ctx["plan"] = None                  # (a later optimizer-carrying step rebuilds its arrays)
        else:
            _fill_optimizer(ctx, a, opt)
        cold_host = None
        if nxt is not None and cold_next:
            # the count of the cold window's next march travels to pinned memory (one slot per stage set): stored by the
            # march itself (next_count_host) or copied behind it; what _check_cold_stage watches for is both words >= 0
            hosts = ctx.get("cold_hosts")
            if hosts is None:
                hosts = ctx["cold_hosts"] = [torch.empty(2, dtype=torch.int32, pin_memory=True) for _ in range(2)]
            cold_host = hosts[which]
            cold_host.fill_(-1)
        mirrored = cold_host is not None and MIRROR_COUNT
        a.next_count_host = cold_host.data_ptr() if mirrored else None      # (the struct is the last step's: set every time)
        carried = _call("train_step_mse", a)
        _count_launches(M)
        if nxt is not None:
            if cold_next and not mirrored:
                with torch.cuda.stream(side_stream):
                    cold_host.copy_(nxt["counter"], non_blocking=True)
            ready = _hand_over(model, stash, [(_stage_key(no, nd, perturb, dt_gamma, max_steps), nxt)], side_stream, carried)
            if cold_next:
                nxt["cold_check"] = (ready, cold_host, Mn)
        if not raw:
            _install_grads(ctx)
    return (ctx["out_image"], ctx["dw"]) if raw else ctx["out_image"]


def train_step_events_native(model, data, loss_opt, opt, next_data=None, side_stream=None, bg_color=None, perturb=True,
                             dt_gamma=0, max_steps=1024):
    """One event-only training step through enerf_train_step_events: both renders (marched ahead of time when the
    previous step asked for it), the event loss, both backwards, the optimizer, and the two marches of `next_data` on
    `side_stream`.  -> (loss, delta).  Gradients of the MLP weights are left in p.grad, the table's dense gradient buffer
    comes back clean, the optimizer's step counts advance.  Values: those of events.train_step_events_manual +
    FusedAdam.step_grid_table (the same library calls, in the same order)."""
    flat = lambda d: [(d["rays_evs_o" + k].contiguous().view(-1, 3), d["rays_evs_d" + k].contiguous().view(-1, 3)) for k in "12"]
    pairs = flat(data)
    N, dev = pairs[0][0].shape[0], pairs[0][0].device
    with torch.no_grad():
        C = channels(model)
        bg = torch.rand((1, 1, C), device=dev) if bg_color is None else bg_color.detach().to(torch.float32).contiguous()
        if bg.numel() != C:
            raise ValueError(f"train_step_events_native: one background colour of {C} values, got {bg.numel()}")
        pres, slots = [], []
        for ro, rd in pairs:
            pres.append(_take_or_march(model, ro, rd, perturb, dt_gamma, max_steps))
            slots.append(model.rendered_counter_slot)
        stash = _stash_if_free(model) if next_data is not None and side_stream is not None else None
        Nn = Mn = 0
        if stash is not None:
            nxt_pairs = flat(next_data)
            Nn = nxt_pairs[0][0].shape[0]
            Mn = _budget_rows(_budget(model))
        ctx = _native_events_ctx(model, N, (pres[0]["M"], pres[1]["M"]), Nn, Mn, bool(loss_opt.use_luma), dev)
        a = ctx["a"]
        _fill_step(ctx, a)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        a.bg_color = bg.data_ptr()
        a.pols = data["pols"].contiguous().data_ptr()
        a.use_luma, a.linlog = int(bool(loss_opt.use_luma)), int(bool(loss_opt.linlog))
        # (the normalised loss carries the reference's weight of 20: event_only is a condition of this step)
        a.C_thres, a.log_thres = float(loss_opt.C_thres), float(loss_opt.log_thres)
        a.upstream = 20.0 if loss_opt.C_thres == -1 else 1.0
        a.loss = loss.data_ptr()
        for q, pre in enumerate(pres):
            _fill_samples(a.r[q], pre)
        # merged layout: the second render's samples lie right behind the first's M rows (stages of one generation do)
        M0 = pres[0]["M"]
        merged = (ctx["tm"] is not None and pres[1]["M"] == M0
                  and pres[1]["xyzs"].data_ptr() == pres[0]["xyzs"].data_ptr() + 12 * M0
                  and pres[1]["dirs"].data_ptr() == pres[0]["dirs"].data_ptr() + 12 * M0
                  and pres[1]["deltas"].data_ptr() == pres[0]["deltas"].data_ptr() + 8 * M0)
        a.flags = _step_flags(2 if merged else 0)
        staged = []
        if stash is not None:
            _fill_march(a, model, side_stream, perturb, dt_gamma, max_steps)
            for q, (no, nd) in enumerate(nxt_pairs):
                counter = _next_counter(model)
                nxt, which = _next_stage(a.r[q], ctx["stages"][q], ctx["flip"][q], pres[q], counter,
                                         getattr(model, "last_counter_slot", None), no, nd)
                ctx["flip"][q] = which ^ 1
                staged.append((_stage_key(no, nd, perturb, dt_gamma, max_steps), nxt))
        _fill_optimizer(ctx, a, opt)
        carried = _call("train_step_events", a)
        # (merged, the library issued ONE grid_encode_forward / backward over 2 M points)
        for points in ([pres[0]["M"] + pres[1]["M"]] if merged else [pre["M"] for pre in pres]):
            _count_launches(points)
        if staged:
            _hand_over(model, stash, staged, side_stream, carried)
        _install_grads(ctx)
        model.rendered_counter_slot = slots[-1]
    return loss, ctx["delta"]
