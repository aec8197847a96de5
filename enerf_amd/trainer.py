"""Minimal train / render harness around the hot path (the bench's "step"), re-stating what main_nerf.py +
Trainer.train_one_epoch do per iteration in the reference (main_nerf.py:211-214, nerf/utils.py:943-997):

    every 16 steps: model.update_extra_state()          (density-grid EMA + packbits + mean_count)
    render -> loss -> backward -> [all-reduce grads] -> Adam(betas=(0.9, 0.99), eps=1e-15) step

`occupancy="synthetic"` keeps marching against the analytic scene's bitfield: update_extra_state() still runs (its cost
is part of the step) but the synthetic grid is restored afterwards, so sample counts stay reproducible with
random-init weights.

`use_graphs=True` (fused fp32 HIP path only): once the sample budget is known (after the first 16 steps) the
render -> loss -> backward part of an RGB step is captured into a HIP graph per (ray count, sample budget) and replayed;
update_extra_state, the gradient all-reduce and the optimizer stay outside.  The sample budget is rounded up to a
multiple of 8192 samples so that the 16-step windows share graphs (a larger budget never drops a ray the reference's
budget would keep).  A 4096-ray step is otherwise bounded by the host's launch rate, not by the kernels.
"""
import torch

from . import dp_tail, scene
from .optim import FusedAdam
from .parallel import GradAverager


_UNSET = object()


class TrainHarness:
    def __init__(self, model, lr=1e-2, occupancy="synthetic", world=1, update_interval=16, use_graphs=False,
                 optimizer=None, fp16=False, amp=None, prime_pool=None, ema_decay=None):
        self.model = model
        # the parameters' exponential moving average (nerf/utils.py:370-373; main_nerf.py:214 trains with 0.95): what
        # evaluate() renders with, what the "best" checkpoint holds, 'ema' in a full checkpoint; moved by train_one_epoch
        self.ema = None
        if ema_decay is not None:
            from .ema import ParamEMA
            self.ema = ParamEMA(model.parameters(), ema_decay)
        adam = optimizer or (FusedAdam if next(model.parameters()).is_cuda else torch.optim.Adam)
        self.opt = adam(model.get_params(lr), betas=(0.9, 0.99), eps=1e-15)
        self.occupancy = occupancy
        self.update_interval = update_interval
        self.global_step = 0
        self.avg = GradAverager(list(model.parameters())) if world > 1 else None
        self._syn = None
        if model.cuda_ray and occupancy == "synthetic":
            self._syn = scene.install_occupancy(model)
        self.early_budget = True      # update_extra_state: the sample budget is read before the update is queued (no stall)
        self.prefetch = True          # data parallel: march the next batch underneath the gradient all-reduce
        self.perturb = True           # training renders jitter their rays (nerf/utils.py:605 `perturb=True`); tests of
        #                               shard-vs-whole-batch equality switch it off: the jitter is seeded by the ray's
        #                               index in ITS batch (raymarching.cu:349-350)
        self.manual_mse = True        # RGB step: closed-form MSE gradient into the fused render node, no autograd engine
        self.fuse_table_adam = True   # one GPU: the table gradient's tile sums feed Adam straight from LDS
        self.overlap_update = True    # update steps: the render's count pass is queued before the update's read-back
        self.native_step = True       # steady-state RGB steps on one GPU as ONE library call (enerf_train_step_mse)
        self.native_normalised = False  # the one-call event step also at C_thres = -1 (the normalised loss): opt-in
        # the frame term in closed form (fused_render.train_step_frames): step_frames, and step_events with
        # event_only = 0, leave autograd where _closed_frames_regime() and the routes' own checks hold: opt-in
        self.closed_frames = False
        self._native_route_sig, self._native_route_dp, self._pending_sig = None, False, None
        self._params = [p for g in self.opt.param_groups for p in g["params"]]
        enc = getattr(model, "encoder", None)
        table = getattr(enc, "embeddings", None)
        self._small_params = [p for p in self._params if p is not table]
        self._opt_step = getattr(self.opt, "step_now", self.opt.step)
        self._side = None             # HIP stream of the next batch's march (created on first use)
        self.comm_chunks = 4          # data parallel: pieces of the hash-table gradient all-reduce (0: one bucket + Adam)
        self.comm_mode = "allreduce"  # or "sharded": reduce-scatter -> Adam on this rank's slice -> all-gather
        self.comm_dtype = None        # torch.bfloat16: halve the table gradient's bytes on the wire (changes rounding)
        # sharded tail: this rank's slice of the table keeps its own record lists for the optimizer pass (the one-GPU
        # flush, csrc/gridencoder.hip OwnerRange) and only the rest of the gradient is made dense for the reduce-scatter
        self.fused_sharded = True
        # where the next batch's march is released on the side stream: once the "forward" is queued (runs beside the
        # MLP backward), once the MLP backward is ("mlp_backward": runs beside the hash table's backward and the
        # optimizer -- the MFMA kernels, one register-filling wavefront per SIMD, then have the CUs to themselves:
        # steady step 0.470 -> 0.434 ms on one MI355X), or, data parallel, once the "collectives" are
        self.prefetch_at = "mlp_backward"
        self._raw_grads = None
        self._cleared_grad = None     # the embeddings' gradient buffer as the last Adam pass left it (all zeros)
        dev0 = next(model.parameters()).device
        self._prime_pool(dev0, prime_pool)
        self._loss_ring = torch.zeros(64, device=dev0)
        self._loss_cursor = 0
        # Mixed precision, two separate switches:
        #   fp16=True: the shipped configs' `fp16 = True` (nerf/utils.py:350,964-975: autocast(float16) + GradScaler).  Two
        #     routes to the same regime, chosen here:
        #       * the closed-form step on fp16 operands (`amp_f16`; one GPU, a model the fused path serves, FusedAdam): the
        #         nn.Linear nets on v_mfma_f32_32x32x16_f16 with every layer's activations and activation gradients rounded
        #         to fp16 (enerf_mlp32_precision(3)), fp32 accumulation, fp32 marching / compositing / trunc_exp as under
        #         the reference's autocast, and the GradScaler's protocol on the device (csrc/optim.hip enerf_amp_*: the
        #         loss gradient is multiplied by the scale, a step whose weight gradients are not finite is not applied
        #         and halves the scale, 2000 clean steps double it) on the scaler's own tensors -- so its state_dict() is
        #         what a checkpoint stores and restores.  What is NOT reproduced: the half copy of the hash table
        #         (gridencoder/grid.py:38-39: the gather reads the fp32 table, features are fp32 until the first layer
        #         rounds them).
        #       * the stratified sampler's fp16 regime (`strat_f16`; one GPU, a `cuda_ray = False` model of network.py
        #         nets): the same mlp32 precision 3, set for the step by _amp_scope, on the native route of
        #         stratified.py with its colour rows / rgb in fp16, and the GradScaler's host
        #         protocol as the reference runs it (scale(loss).backward(), unscale_, step, update) -- no autocast.
        #         A step that route does not serve (background model, upsample_steps, FFMLP nets, an attached
        #         averager) takes the autocast route with the same scaler.
        #       * fp16="autocast" (and whatever the closed-form step does not serve): torch.autocast + GradScaler around
        #         the op-by-op route, half hash table + half table gradient (gridencoder/grid.py:38-39,72), half SH.
        #   amp="bf16": NOT the reference's regime, named apart for that reason -- the closed-form step with the networks
        #     on bf16 operands (mlp32 precision 2), fp32 hash table, fp32 master weights.  bf16 has fp32's exponent range,
        #     so there is no loss scaling: the GradScaler is kept disabled.  The model's own `mlp_precision` is only
        #     overridden for the duration of this harness's steps.
        if fp16 == "bf16":                      # (the spelling of earlier rounds)
            fp16, amp = False, "bf16"
        if amp not in (None, "bf16"):
            raise ValueError(f"amp={amp!r}: None or 'bf16'")
        self.fp16 = bool(fp16)                  # the autocast route (all of it, or the steps the closed form cannot take)
        self.amp_bf16 = self.amp_f16 = self.strat_f16 = False
        self._f16_autocast = True               # the autocast route's autocast (off for a strat_f16 step)
        cuda_fused = False
        if (fp16 or amp) and next(model.parameters()).is_cuda:
            from . import fused_network
            cuda_fused = fused_network.kind_of(model) is not None
        if fp16 is True and cuda_fused and world == 1 and hasattr(self.opt, "step_grid_table") \
                and getattr(model, "cuda_ray", False):
            self.fp16, self.amp_f16 = False, True
        elif fp16 is True and cuda_fused and world == 1 and not getattr(model, "cuda_ray", False):
            self.fp16, self.strat_f16 = False, True
        if amp == "bf16" and not fp16:
            if cuda_fused:
                self.amp_bf16 = True            # (scoped to this harness's own steps: _amp_scope)
            else:
                raise ValueError("amp='bf16' needs a CUDA model the fused path serves (network.py / network_ff.py nets)")
        self.scaler = (torch.amp.GradScaler("cuda", enabled=self.fp16 or self.amp_f16 or self.strat_f16)
                       if (self.fp16 or self.amp_bf16 or self.amp_f16 or self.strat_f16) else None)
        self._amp_words = None
        if self.amp_f16:
            self.scaler._lazy_init_scale_growth_tracker(dev0)
            self._amp_words = torch.zeros(2, dtype=torch.int32, device=dev0)       # [found_inf, skipped steps]
        # what Trainer keeps beside the model and lands in its checkpoints (nerf/utils.py:381-389,1300-1304)
        self.epoch = 1
        self.stats = {"loss": [], "valid_loss": [], "results": [], "checkpoints": [], "best_result": None}
        self.lr_scheduler = None      # set_lr_scheduler(): stepped after every optimizer step (main_nerf.py:212,214)
        self._log = None              # the TrainLog of the epoch under way (train_one_epoch(log=...)), else None
        self.use_graphs = bool(use_graphs)
        self._graphs = {}
        self._graph_generation = 0
        if self.use_graphs:
            model.sample_budget_quantum = 8192

    @staticmethod
    def _prime_pool(dev, want):
        """Once per process: leave one large free block in torch's caching pool.  The first 16 steps size their sample
        buffers from each render's own count (a different size every step), and every size the pool cannot serve is a
        hipMalloc in the middle of a step -- milliseconds on a fresh process, in a loop whose step is 0.4 ms.
        `want`: None = on unless ENERF_PRIME_POOL=0, False = off, True = on, an int = that many bytes.  Sized from what
        is actually free (at most a quarter of it, 2 GiB at most, nothing under 1 GiB free): several ranks on one device
        or a nearly full GPU must not lose a harness to it, and a failed priming is a no-op."""
        import os
        if dev.type != "cuda" or getattr(TrainHarness, "_pool_primed", False) or want is False:
            return
        if want is None and os.environ.get("ENERF_PRIME_POOL", "1") == "0":
            return
        try:
            free, _total = torch.cuda.mem_get_info(dev)
            size = int(want) if (want is not True and want is not None) else min(2 << 30, free // 4)
            if free < (1 << 30) or size <= 0 or size > free // 2:
                return
            torch.empty(size, dtype=torch.uint8, device=dev)
            TrainHarness._pool_primed = True
        except Exception:                       # noqa: BLE001 -- out of memory or no device API: train without it
            pass

    def _amp_scope(self):
        """amp='bf16' / the fp16 closed form: the fused kernels read `model.mlp_precision` at launch -- set for this
        harness's step, restored after it (the model keeps its own arithmetic for inference and for other harnesses)."""
        m = self.model
        prev = m.__dict__.get("mlp_precision", _UNSET)
        m.mlp_precision = 3 if (self.amp_f16 or self.strat_f16) else 2
        return prev

    def _strat_f16_step(self, fn, native, *args):
        """strat_f16: one step on the host GradScaler protocol under mlp32 precision 3 -- without autocast when the
        stratified route serves it (`native`), under autocast (the statement) otherwise."""
        prev = self._amp_scope()
        self.fp16, self._f16_autocast = True, not native
        try:
            return fn(*args)
        finally:
            self.fp16, self._f16_autocast = False, True
            self._amp_restore(prev)

    def _strat_f16_ok(self, rays_o, rays_d, render_kw=None, bg_color=None):
        """The stratified route takes this step's renders in the fp16 regime (decided per step: an averager may be
        attached after __init__, and render keywords may ask for upsampling -- NeRFRenderer.run's default does)."""
        from . import stratified
        kw = render_kw or {}
        return self.avg is None and stratified.supported(self.model, rays_o, rays_d, kw.get("upsample_steps", 128),
                                                         bg_color, kw.get("out_dim_color"))

    def amp_skipped_steps(self):
        """fp16 closed form: optimizer steps the loss scaling has skipped so far (their gradients were not finite) -- the
        optimizer's own `step` counts them, its bias corrections do not.  One 4-byte read-back."""
        return int(self._amp_words[1]) if self._amp_words is not None else 0

    def _amp_closed_form_ok(self):
        """Decided per step (graph replay, an attached averager and `fuse_table_adam` can all change after __init__): what
        the device-side GradScaler protocol cannot serve takes the autocast route with the same scaler instead of raising."""
        return not self.use_graphs and self.avg is None and bool(self.fuse_table_adam)

    def _amp_step(self, fn, *args, **kw):
        """One step under the device-side GradScaler protocol (include/enerf_hip.h: enerf_amp_begin / enerf_amp_end)."""
        from . import _lib as L
        lib = L.lib()
        sc = self.scaler
        if self.use_graphs or self.avg is not None or not self.fuse_table_adam:
            raise RuntimeError("the fp16 closed-form step needs one GPU, the fused table optimizer and no graph replay "
                               "(use fp16='autocast')")
        L.check(lib.enerf_amp_begin(sc._scale.data_ptr(), sc._growth_tracker.data_ptr(), self._amp_words.data_ptr(),
                                    self._amp_words.data_ptr() + 4), "amp_begin")
        try:
            out = fn(*args, **kw)
        except BaseException:
            lib.enerf_amp_cancel()
            raise
        L.check(lib.enerf_amp_end(float(sc.get_growth_factor()), float(sc.get_backoff_factor()),
                                  int(sc.get_growth_interval()), L.stream_handle()), "amp_end")
        return out

    def _amp_restore(self, prev):
        if prev is _UNSET:
            self.model.__dict__.pop("mlp_precision", None)
        else:
            self.model.mlp_precision = prev

    def set_lr_scheduler(self, factory):
        """`factory(optimizer) -> scheduler`, as the reference's Trainer takes it (main_nerf.py:212: LambdaLR with
        0.1 ** min(iter / iters, 1)); stepped once after every optimizer step (`scheduler_update_every_step=True`).
        Every optimizer route of the harness reads `param_groups[...]['lr']` at launch time, the fused table pass
        (FusedAdam.step_grid_table) included, so the schedule reaches all of them."""
        self.lr_scheduler = factory(self.opt)
        self.opt._opt_called = True       # the harness calls step_now / step_grid_table, not the wrapped step()
        return self.lr_scheduler

    def save_checkpoint(self, path, full=False, best=False):
        """The reference's checkpoint dict (nerf/utils.py:1295-1351) -> `path`; a full one carries 'ema' when the harness
        keeps an average.  `best` (:1333-1351): written only when stats["results"][-1] is below stats["best_result"] (or
        there is none yet), which it then becomes, with the AVERAGE's weights under 'model' when there is one; -> None
        when nothing was written (a warning when nothing has been evaluated yet)."""
        from .checkpoint import save_checkpoint
        return save_checkpoint(self, path, full=full, best=best)

    def save_mesh(self, save_path, resolution=256, threshold=10):
        """The reference's Trainer.save_mesh (nerf/utils.py:712-732): sigma on a resolution^3 lattice over aabb_infer,
        marching cubes at `threshold`, a binary PLY at `save_path` (rank 0 writes).  The query runs in this harness's
        regime, as the reference's autocast(enabled=fp16) does.  -> (vertices [V, 3] fp64 world, triangles [F, 3] int32)."""
        from .mesh import harness_save_mesh
        return harness_save_mesh(self, save_path, resolution, threshold)

    def evaluate(self, views, opt, name="eval", save_dir=None, ema=None):
        """The reference's Trainer.evaluate / evaluate_one_epoch (nerf/utils.py:763-766, 1028-1293) over `views` (the
        val split's collate dicts): the renders of eval_step / eval_step_tumvie under model.eval() in this harness's
        regime, PSNR and SSIM, or for `opt.event_only` the log-affine correction and its metrics; `ema` (store / copy_to /
        restore; None: the harness's own average, if it keeps one) brackets the renders as there; rank 0 writes the
        validation/ tree under `save_dir`.  -> dict of floats and lists (enerf_amd/evaluate.py)."""
        from .evaluate import harness_evaluate
        return harness_evaluate(self, views, opt, name=name, save_dir=save_dir, ema=self.ema if ema is None else ema)

    def test(self, views, opt, save_path, name=None, write_depth=None, write_behind=True):
        """The reference's Trainer.test (nerf/utils.py:768-804) over `views` (dicts with rays_o, rays_d, H, W: a
        FrameSampler(num_rays=-1) batch; images are not needed): test_step per view (bg_color None, perturb off, staged)
        under model.eval() in this harness's regime, WITHOUT the average, as there; one enerf_view_finish launch makes the
        bytes (linear_to_srgb for color_space = "linear") and `{save_path}/{name}_{i:04d}.png` -- grey for C = 1, RGB for
        C = 3 -- is written behind the next view's render, `depth/{name}_{i:04d}_depth.png` with `write_depth` (default:
        the reference's epoch % 100 == 0).  `name` defaults to ngp_ep{epoch:04d}.  Returns once every file is written
        (`write_behind=False`: view by view, synchronously) -> the list of image paths (enerf_amd/view.py)."""
        from .view import harness_test
        return harness_test(self, views, opt, save_path, name=name, write_depth=write_depth, write_behind=write_behind)

    def render_path(self, poses, intrinsics, H, W, opt, outdir, normalize=False, write_behind=True):
        """The path loop of the reference's scripts/render.py:489-509 over cam2world `poses` [n, 3 or 4, 4] (see
        enerf_amd/render_path.py): full-frame rays on the device, render with bg_color 1, `rgb/{i}.png`,
        `depth/{i}_depth.png`, `raws/{i}.npy` under `outdir`; `normalize` is that script's per-frame min-max scaling
        (enerf_view_minmax into enerf_view_finish; the raw frame is then the scaled one, as there).  -> the rgb paths."""
        from .view import harness_render_path
        return harness_render_path(self, poses, intrinsics, H, W, opt, outdir, normalize=normalize,
                                   write_behind=write_behind)

    def train_one_epoch(self, sampler, opt, order=None, log=None):
        """The reference's Trainer.train_one_epoch (nerf/utils.py:920-1015); its logging with `log`: one step per batch of
        `sampler` (a FrameSampler or an EventSampler) in `order` (default: torch.randperm(len(sampler)) from torch's
        global CPU generator, the DataLoader(shuffle=True) of the reference) -- step_events for a batch with
        "rays_evs_o1", step_frames otherwise; the next batch is drawn before the current step is taken, so that the event
        route can march it underneath.  The losses are summed on the device in fp64, in step order (the reference's
        Python-float sum of fp32 losses), and read back once.  After the last step the average, if there is one, is
        updated; -> the epoch's mean loss, also appended to stats["loss"].  `self.epoch` is train()'s to move.
        `log` (a train_log.TrainLog; None, the default: no step does anything it would not do otherwise): every step writes
        one row of the log's device ring -- the loss, an event step's terms and the implicit contrast threshold of its
        delta and polarities (event_diag.estimate_C_thres), by launches on the step's stream and no read-back -- and the
        ring is read back once, by log.flush() when the epoch ends.  A logged event step does not take the captured-graph
        route (`use_graphs`), which hands out nothing but the loss: it takes the next route that serves it.  Rank 0 logs
        its own batch; on other ranks the log is ignored."""
        if log is not None and not log.active:
            log = None
        if order is None:
            order = torch.randperm(len(sampler))
        order = [int(i) for i in (order.tolist() if torch.is_tensor(order) else order)]
        if not order:
            raise ValueError("train_one_epoch: an empty epoch")
        total = None
        data = sampler.batch([order[0]])
        if log is not None:
            log.begin(len(order), next(self.model.parameters()).device)
        self._log = log
        try:
            for k in range(len(order)):
                nxt = sampler.batch([order[k + 1]]) if k + 1 < len(order) else None
                if "rays_evs_o1" in data:
                    loss = self.step_events(data, opt, nxt if nxt is not None and "rays_evs_o1" in nxt else None)
                else:
                    loss = self.step_frames(data, opt, sampler)
                    if log is not None:
                        log.frame_step(loss)
                if log is not None:                     # (the lr after this step's scheduler step, as the reference logs it)
                    log.end_step(self.global_step, self.epoch, self.opt.param_groups[0]["lr"])
                loss = loss.detach().double()
                total = loss.clone() if total is None else total.add_(loss)
                data = nxt
        finally:
            self._log = None
        if log is not None:
            log.flush()
        if self.ema is not None:
            self.ema.update()
        mean = float(total) / len(order)
        self.stats["loss"].append(mean)
        return mean

    def train(self, sampler, opt, max_epochs, valid_views=None, eval_interval=10, workspace=None, name="ngp",
              max_keep_ckpt=2, log=None):
        """The reference's Trainer.train (nerf/utils.py:734-761): for every epoch from `self.epoch` to `max_epochs`,
        train_one_epoch; with a `workspace`, on rank 0, a full checkpoint {workspace}/checkpoints/{name}_ep{epoch:04d}.pth,
        recorded in stats["checkpoints"], the oldest beyond `max_keep_ckpt` deleted (:1323-1329); every `eval_interval`
        epochs, with `valid_views`, evaluate() -- its valid_loss appended to stats["valid_loss"] and stats["results"] (the
        reference's default use_loss_as_metric=True) -- and the "best" checkpoint {workspace}/checkpoints/{name}.pth.
        Marking the cells no training camera sees (model.mark_untrained_grid, which the reference calls here) stays the
        caller's job, as for every other entry point of the harness.  `log`: every epoch's train_one_epoch(log=log); the
        log is not part of a checkpoint.  -> stats."""
        import os
        import torch.distributed as dist
        rank0 = not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0
        ckpt_dir = None
        if workspace is not None:
            ckpt_dir = os.path.join(workspace, "checkpoints")
            if rank0:
                os.makedirs(ckpt_dir, exist_ok=True)
        for epoch in range(self.epoch, max_epochs + 1):
            self.epoch = epoch
            self.train_one_epoch(sampler, opt, log=log)
            if ckpt_dir is not None and rank0:
                path = os.path.join(ckpt_dir, f"{name}_ep{epoch:04d}.pth")
                kept = self.stats["checkpoints"]
                kept.append(path)
                if len(kept) > max_keep_ckpt:
                    old = kept.pop(0)
                    if os.path.exists(old):
                        os.remove(old)
                self.save_checkpoint(path, full=True)
            if valid_views is not None and epoch % eval_interval == 0:
                r = self.evaluate(valid_views, opt, name=f"{name}_ep{epoch:04d}")
                self.stats["valid_loss"].append(r["valid_loss"])
                self.stats["results"].append(r["valid_loss"])
                if ckpt_dir is not None and rank0:
                    self.save_checkpoint(os.path.join(ckpt_dir, f"{name}.pth"), best=True)
        return self.stats

    def load_checkpoint(self, checkpoint, model_only=False):
        """Resume from a checkpoint in the reference's format (nerf/utils.py:1353-1415), whoever wrote it."""
        from .checkpoint import load_checkpoint
        self._graphs.clear()
        return load_checkpoint(self, checkpoint, model_only=model_only)

    def maybe_update_extra_state(self, coming_render=None):
        """`coming_render` = (rays_o, rays_d) of the render this step starts with, when it will take the fused path with
        default march settings: its near/far + count pass are queued before the update's read-back is waited for
        (fused_render.premarch_count), so the device works while the host waits."""
        m = self.model
        if m.cuda_ray and self.global_step % self.update_interval == 0:
            begin = getattr(m, "update_extra_state_begin", None)
            early = None
            if begin is None or coming_render is None or not self.overlap_update or self.use_graphs:
                m.update_extra_state()
                handle = None
            else:
                if self.early_budget:
                    # the window's step counters, read behind the last march on the side stream: the budget is known
                    # before the update is even queued, and the host never waits behind the sweep
                    from . import fused_render as _fr
                    early = _fr.early_mean_count(m)
                handle = begin()
            if self._syn is not None:
                m.density_grid.copy_(self._syn[0])
                m.density_bitfield.copy_(self._syn[1])
            if handle is not None:
                from . import fused_render
                m._premarched = None                    # (anything marched against the old bitfield is void)
                fused_render.premarch_count(m, *coming_render, perturb=self.perturb)
                if early is not None:
                    m.update_extra_state_end(handle, early)
                else:
                    m.update_extra_state_end(handle)
            self._agree_on_budget()

    def _agree_on_budget(self):
        """Data parallel: every rank must take the same route through the step (the routes differ in the collectives
        they issue), and the routes are chosen from static properties of the model plus -- for graph replay -- the
        sample budget.  The budget comes from each rank's own step counters ("all-reduce-MAX it every 16
        steps so M is uniform"): one 8-byte MAX all-reduce per update_extra_state window makes it the same everywhere
        (a larger budget never drops a ray the local budget would keep)."""
        if self.avg is None:
            return
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        m = self.model
        dev = next(m.parameters()).device
        t = torch.tensor([int(m.mean_count)], dtype=torch.int64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        m.mean_count = int(t.item())

    # ------------------------------------------------------------------ HIP-graph replay of render + loss + backward
    def _graph_key(self, tag, rays_o):
        m = self.model
        q = m.sample_budget_quantum
        return (tag, tuple(rays_o.shape), (int(m.mean_count) + q - 1) // q * q)

    def _capture(self, inputs, loss_fn, fwd_bwd_fn=None):
        """Capture loss_fn(static inputs) + backward -- or fwd_bwd_fn(static inputs), which leaves the gradients in
        p.grad itself and returns the loss; returns the replay state."""
        from . import _lib
        m = self.model
        _lib.prof.enable(False)                       # hipEvent timing hooks cannot live inside a captured graph
        if getattr(m, "graph_counter", None) is None:
            m.graph_counter = torch.zeros(2, dtype=torch.int32, device=inputs[0].device)
        st = {"in": [t.clone() for t in inputs]}
        params = [p for p in m.parameters() if p.requires_grad]

        def fwd_bwd():
            if fwd_bwd_fn is not None:
                return fwd_bwd_fn(*st["in"])
            loss = loss_fn(*st["in"])
            loss.backward()
            return loss

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):                        # warm-up on the capture stream: workspaces reach their size
                self.opt.zero_grad(set_to_none=True)
                fwd_bwd()
        torch.cuda.current_stream().wait_stream(side)
        gen = _lib.lib().enerf_workspace_generation()
        if gen != self._graph_generation:             # the warm-up grew a scratch buffer: older captures point at
            self._graphs.clear()                      # freed memory (see _graph_for)
            self._graph_generation = gen
        self.opt.zero_grad(set_to_none=True)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st["loss"] = fwd_bwd().detach()
        st["graph"] = g
        st["grads"] = [(p, p.grad) for p in params]
        assert _lib.lib().enerf_workspace_generation() == gen, "a scratch buffer grew inside a graph capture"
        return st

    def _graph_for(self, key):
        """The captured state for `key`, or None.  The library's scratch buffers are grow-only: a launch that needed
        more (a larger budget or ray count) re-allocated one since the captures were made, and every captured graph
        holds the old pointers -- all of them are dropped and re-captured on demand."""
        if self._graphs:
            from . import _lib
            if _lib.lib().enerf_workspace_generation() != self._graph_generation:
                self._graphs.clear()
        return self._graphs.get(key)

    def _replay(self, st, inputs, renders):
        m = self.model
        for dst, src in zip(st["in"], inputs):
            dst.copy_(src)
        # the captured count pass clips rays against the library's occupied-cell box, which only host code refreshes
        # (fused_render.occupied_box_flag): update_extra_state may have rewritten the bitfield since the capture
        from . import fused_render
        fused_render.occupied_box_flag(m)
        st["graph"].replay()
        for p, g in st["grads"]:
            p.grad = g
        # every render of the step used the same fixed-address counter; the ring gets the last render's counts
        for _ in range(renders):
            m.step_counter[m.local_step % 16].copy_(m.graph_counter)
            m.local_step += 1
        if self.avg is not None:
            self.avg()
        self._opt_step()
        return st["loss"].detach()

    def _graphable(self, rays_o, rays_d):
        from . import fused_render
        return (self.use_graphs and not self.fp16 and self.model.mean_count > 0
                and fused_render.supported(self.model, rays_o.contiguous().view(-1, 3), rays_d.contiguous().view(-1, 3),
                                           1, 0))

    def _reduce_grads(self, next_rays=None):
        """Average gradients across ranks.  With `next_rays` = (rays_o, rays_d) of the following step, the part of that
        step's render that does not read the parameters (near_far + march_rays_train, ~20 % of a step) is issued right
        after the collectives and runs underneath them; skipped whenever the next step starts with
        update_extra_state (new bitfield / sample budget) or the sample budget is not known yet."""
        if self.avg is None:
            return
        self.avg.start()
        m = self.model
        if (next_rays is not None and self.prefetch and m.cuda_ray
                and self.global_step % self.update_interval != 0):
            from . import fused_render
            ro, rd = next_rays
            if fused_render.supported(m, ro.contiguous().view(-1, 3), rd.contiguous().view(-1, 3), 1, 0):
                fused_render.prefetch_march(m, ro, rd, perturb=self.perturb)
        self.avg.finish()

    def _manual_ok(self, rays_o, rays_d, target, render_kw):
        from . import fused_render
        m = self.model
        return (self.manual_mse and m.cuda_ray and target.dtype == torch.float32
                and not set(render_kw) - {"dt_gamma", "max_steps"}
                and fused_render.supported(m, rays_o.contiguous().view(-1, 3), rays_d.contiguous().view(-1, 3), 1,
                                           render_kw.get("dt_gamma", 0)))

    def _side_prefetch(self, *next_rays):
        """-> a callable that marches the next step's ray sets (one (rays_o, rays_d) pair per render) on the side
        stream (see fused_render.prefetch_march), or None when the next step starts with update_extra_state (new
        bitfield / budget) or nothing is known about it."""
        m = self.model
        if (not next_rays or any(r is None for r in next_rays) or not self.prefetch
                or getattr(m, "graph_counter", None) is not None or self.global_step % self.update_interval == 0):
            return None
        from . import fused_render
        for ro, rd in next_rays:
            if not fused_render.supported(m, ro.contiguous().view(-1, 3), rd.contiguous().view(-1, 3), 1, 0):
                return None
        if self._side is None:
            self._side = torch.cuda.Stream()

        def issue(background=True, signalled=False):
            # signalled: called right after the MLP backward's reduce launch, which carries a completion signal
            # (fused_network.nerf_backward) -- the side stream waits for that instead of an event record here.
            # (the second march of an event step is ordered behind the first on the side stream: no wait of its own)
            for k, (ro, rd) in enumerate(next_rays):
                fused_render.prefetch_march(m, ro, rd, perturb=self.perturb, stream=self._side, background=background,
                                            after_signal=(True if k == 0 else "ordered") if signalled else False)
        return issue

    def _manual_fwd_bwd(self, rays_o, rays_d, target, dt_gamma=0, max_steps=1024, after_forward=None, raw=False,
                        defer_table=False, after_mlp_backward=None):
        """Render + MSE + backward with the loss gradient in closed form (fused_render.train_step_mse): same kernels
        for the render and its backward, no autograd graph, no loss-backward / blend / depth / fill launches.
        Leaves the gradients in p.grad, returns the loss."""
        from . import fused_network, fused_render
        m = self.model
        # nothing accumulates across steps (zero_grad(set_to_none=True)) -- except that the hash table's gradient
        # buffer is kept when the previous step's Adam pass cleared it (step_now(zero_grads=True)): the grid backward
        # then adds straight into it, with no 52 MB allocation and fill
        emb = m._modules["encoder"]._parameters["embeddings"]
        keep = self._reuse_cleared_grad(emb)
        for p in self._params:
            p.grad = None
        if keep is not None and not self.use_graphs:
            emb.grad = keep
        loss = None
        if not self.use_graphs:                     # (a captured graph would always accumulate into the same slot)
            # loss values land in a ring of device scalars, cleared once per lap: no loss kernels, no per-step fill
            # (laps are counted on the ring's own cursor: steps of other kinds in between do not use slots)
            loss = self._loss_slot()
        if defer_table and emb.grad is None:        # the dense part of the gradient (levels too small to bin) needs a home
            emb.grad = torch.zeros_like(emb)
        image, grads = fused_render.train_step_mse(m, rays_o, rays_d, target, 1, self.perturb, dt_gamma, max_steps,
                                                   after_forward=after_forward, loss_out=loss, raw=raw,
                                                   defer_table=defer_table, after_mlp_backward=after_mlp_backward)
        if raw:
            self._raw_grads = grads                 # (embedding gradient, flat dW): dp_tail.finish takes over
        else:
            for p, g in zip(fused_network.network_params(m), grads):
                if g is not None:
                    p.grad = g.view_as(p)
        if loss is not None:
            return loss             # a view into the ring: overwritten one lap (64 steps) later -- clone to keep it
        with torch.no_grad():
            return torch.nn.functional.mse_loss(image, target.view(image.shape))

    def _reuse_cleared_grad(self, emb):
        """Only a buffer the last flush left clean may be added into: -> emb.grad when it is the buffer the last
        optimizer pass cleared (`_cleared_grad`), else None (the caller drops whatever is there).  The claim is spent
        either way: whoever clears the buffer next sets `_cleared_grad` again."""
        keep = emb.grad if (self._cleared_grad is not None and emb.grad is self._cleared_grad) else None
        self._cleared_grad = None
        return keep

    @staticmethod
    def _discard_pending_records():
        """A step that left the table gradient as record lists died before its optimizer pass: empty the lists so that
        the next backward is not refused."""
        from . import _lib
        _lib.lib().enerf_grid_records_discard(_lib.stream_handle())

    def _step_then_tail(self, data_parallel, step, issue_prefetch):
        """The handoff of both RGB step routes: `step(own)` renders and runs the backward; with `data_parallel`,
        dp_tail.finish then averages the gradients and takes the optimizer step (`issue_prefetch`: the next batch's
        march, where the tail is to place it).  `own`: this rank's slice of the table where the fused sharded tail
        applies, set in the library for both and cleared however they end.  A step that raises leaves no record lists."""
        own = dp_tail.owner_range(self) if data_parallel else None
        if own is not None:
            from . import _lib as L
            L.check(L.lib().enerf_grid_owner_range(own[0], own[1], 1.0 / own[2]), "grid_owner_range")
        try:
            try:
                out = step(own)
            except BaseException:
                self._discard_pending_records()
                raise
            if data_parallel:
                dp_tail.finish(self, own, issue_prefetch)
        finally:
            if own is not None:
                L.lib().enerf_grid_owner_range(0, 0, 1.0)
        return out

    def gather_sharded_optimizer_state(self):
        """Data parallel, after steps with a sharded tail: the table's Adam moments, whole on every rank again."""
        dp_tail.gather_sharded_optimizer_state(self)

    def tune_comm(self, step_fn, candidates=(1, 2, 4, 8), window=None):
        """Data parallel: pick `comm_chunks`, `comm_mode` and `prefetch_at` by measurement -> {chunks: ms_per_step}."""
        return dp_tail.tune_comm(self, step_fn, candidates, window)

    def probe_comm_dtype(self, step_fn, dtype=torch.bfloat16, window=None, first_step=0):
        """Data parallel: ms per step over one window with the table gradient on the wire in `dtype`; None on one rank."""
        return dp_tail.probe_comm_dtype(self, step_fn, dtype, window, first_step)

    def _loss_slot(self):
        """Loss values land in a ring of device scalars, cleared once per lap: no loss kernels, no per-step fill (laps are
        counted on the ring's own cursor: steps of other kinds in between do not use slots)."""
        slot = self._loss_cursor % self._loss_ring.numel()
        self._loss_cursor += 1
        if slot == 0:
            self._loss_ring.zero_()
        return self._loss_ring[slot]

    def _route_signature(self, rays_o, rays_d, target, next_rays):
        from . import fused_network, fused_render, raymarching
        m = self.model

        def of(t):
            return (t.shape, t.dtype, t.device, t.is_contiguous(), t.requires_grad)
        nxt = None if next_rays is None or any(r is None for r in next_rays) else (of(next_rays[0]), of(next_rays[1]))
        return (of(rays_o), of(rays_d), of(target), nxt, m.training, m.cuda_ray, m.bg_radius, float(m.density_scale),
                torch.is_grad_enabled(), torch.is_autocast_enabled(), fused_render.ENABLED, fused_render.NATIVE_STEP,
                fused_network.ENABLED, raymarching._DEVICE, self.use_graphs, self.fp16, self.manual_mse, self.prefetch,
                self.prefetch_at, self.avg is None, self.fuse_table_adam, self.comm_chunks, self.comm_mode,
                self.comm_dtype, getattr(m, "graph_counter", None) is None, getattr(m, "disable_view_direction", None),
                id(self.opt))

    def _step_rgb_native(self, rays_o, rays_d, target, next_rays, data_parallel=False, checked=False):
        """The steady-state step as one library call (fused_render.train_step_native -> enerf_train_step_mse): the same
        launches in the same order as _step_rgb_manual's one-GPU route, issued from C.  data_parallel: the call stops
        after the table's backward (dense gradient, no optimizer) and one of the data-parallel tails takes over
        (dp_tail.finish)."""
        from . import fused_render
        m = self.model
        emb = m._modules["encoder"]._parameters["embeddings"]
        if self._reuse_cleared_grad(emb) is None:
            emb.grad = None
        if not checked:                         # (decided by the full checks: later steps of the same signature skip them)
            self._native_route_sig, self._native_route_dp = self._pending_sig, data_parallel
        nxt = None
        if (next_rays is not None and all(r is not None for r in next_rays) and self.prefetch
                and self.global_step % self.update_interval != 0
                and (checked or fused_render.supported(m, next_rays[0].contiguous().view(-1, 3),
                                                       next_rays[1].contiguous().view(-1, 3), 1, 0))):
            if self._side is None:
                self._side = torch.cuda.Stream()
            nxt = next_rays
        if (nxt is None and self.early_budget and self.prefetch and self.global_step % self.update_interval == 0
                and getattr(m, "_last_march_event", None) is None and not data_parallel):
            # the window's last step (the next call starts with update_extra_state): where the marches ride on this
            # stream, the ring of step counters is copied out here, a whole step before the update wants the budget
            fused_render.stage_ring_copy(m)
        loss = self._loss_slot()

        def step(own):                          # (no march for the tail to place: it is queued behind the MLP backward)
            out = fused_render.train_step_native(m, rays_o, rays_d, target, self.opt, next_rays=nxt,
                                                 side_stream=self._side, loss_out=loss, perturb=self.perturb,
                                                 raw=data_parallel, defer_dp=own is not None)
            if data_parallel:
                self._raw_grads = (None, out[1])        # (the table's gradient sits in embeddings.grad)
        self._step_then_tail(data_parallel, step, None)
        if not data_parallel:
            self._cleared_grad = emb.grad
        return loss

    def _step_rgb_manual(self, rays_o, rays_d, target, next_rays, **render_kw):
        chunked = (self.avg is not None and isinstance(self.avg, GradAverager) and hasattr(self.opt, "step_now")
                   and self.comm_chunks > 0)
        if (self.native_step and not render_kw and not self.use_graphs and self.prefetch_at == "mlp_backward"
                and getattr(self.model, "graph_counter", None) is None
                and ((self.avg is None and self.fuse_table_adam) or chunked)):
            from . import fused_render
            if fused_render.native_step_supported(self.model, rays_o.contiguous().view(-1, 3),
                                                  rays_d.contiguous().view(-1, 3), self.opt, data_parallel=chunked):
                return self._step_rgb_native(rays_o, rays_d, target, next_rays, data_parallel=chunked)
        side = self._side_prefetch(next_rays) if not render_kw else None
        late = chunked and side is not None and self.prefetch_at == "collectives"
        # one GPU: nobody but Adam reads the table's gradient, so the backward leaves it as record lists and the
        # optimizer's pass over the table sums them tile by tile in LDS (FusedAdam.step_grid_table)
        fuse_table = (self.fuse_table_adam and self.avg is None and hasattr(self.opt, "step_grid_table")
                      and not self.use_graphs)
        tail_side = side if (not late and self.prefetch_at == "mlp_backward") else None

        def step(own):
            return self._manual_fwd_bwd(rays_o, rays_d, target,
                                        after_forward=None if (late or tail_side is not None) else side, raw=chunked,
                                        defer_table=fuse_table or own is not None, after_mlp_backward=tail_side,
                                        **render_kw)
        loss = self._step_then_tail(chunked, step, side if late else None)
        if chunked:
            return loss
        self._reduce_grads(None if side is not None else next_rays)
        self._optimizer_tail(fuse_table)
        return loss

    def _optimizer_tail(self, fuse_table):
        """The optimizer step of the closed-form routes: the table's record lists straight into Adam where the backward
        left them as lists (`fuse_table`), else Adam over the dense gradients."""
        if fuse_table:
            enc = self.model._modules["encoder"]
            emb = enc._parameters["embeddings"]
            self.opt.step_grid_table(emb, enc._buffers["offsets"], enc.level_dim, extra=self._small_params)
            self._cleared_grad = emb.grad
        elif self.avg is None and hasattr(self.opt, "step_now") and not self.use_graphs:
            self.opt.step_now(zero_grads=True)          # Adam clears what it has read: the next step needs no fill
            self._cleared_grad = self.model.encoder.embeddings.grad
        else:
            self._opt_step()

    def step_rgb(self, rays_o, rays_d, target, next_rays=None, **render_kw):
        """One RGB training step (nerf/utils.py:575-640 train_step + the optimizer part of train_one_epoch)."""
        if self.strat_f16:
            loss = self._strat_f16_step(lambda: self._step_rgb(rays_o, rays_d, target, next_rays, **render_kw),
                                        self._strat_f16_ok(rays_o, rays_d, render_kw))
        elif self.amp_bf16 or self.amp_f16:
            prev = self._amp_scope()
            try:
                if self.amp_f16 and self._amp_closed_form_ok() and self._manual_ok(rays_o, rays_d, target, render_kw):
                    loss = self._amp_step(self._step_rgb, rays_o, rays_d, target, next_rays, **render_kw)
                elif self.amp_f16:              # a step the closed form does not serve: the autocast route, same scaler
                    self.fp16 = True
                    try:
                        loss = self._step_rgb(rays_o, rays_d, target, next_rays, **render_kw)
                    finally:
                        self.fp16 = False
                else:
                    loss = self._step_rgb(rays_o, rays_d, target, next_rays, **render_kw)
            finally:
                self._amp_restore(prev)
        else:
            loss = self._step_rgb(rays_o, rays_d, target, next_rays, **render_kw)
        if self.lr_scheduler is not None:
            self.lr_scheduler.step()
        return loss

    def _step_rgb(self, rays_o, rays_d, target, next_rays=None, **render_kw):
        if not self.model.training:                 # Module.train() walks every submodule: 40 us of a 900 us step
            self.model.train()
        coming = None
        if (self.global_step % self.update_interval == 0 and self.overlap_update and not render_kw and not self.fp16
                and self._manual_ok(rays_o, rays_d, target, render_kw)):
            coming = (rays_o, rays_d)
        self.maybe_update_extra_state(coming)
        self.global_step += 1
        if self._graphable(rays_o, rays_d):
            m = self.model
            key = self._graph_key("rgb", rays_o)
            if self._graph_for(key) is None:
                manual = self._manual_ok(rays_o, rays_d, target, render_kw)
                self._graphs[key] = self._capture(
                    (rays_o, rays_d, target),
                    lambda ro, rd, tg: torch.nn.functional.mse_loss(
                        m.render(ro, rd, staged=False, bg_color=None, perturb=self.perturb, **render_kw)["image"], tg),
                    (lambda ro, rd, tg: self._manual_fwd_bwd(ro, rd, tg, **render_kw)) if manual else None)
            return self._replay(self._graphs[key], (rays_o, rays_d, target), 1)
        if self.fp16:
            self.opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.float16, enabled=self._f16_autocast):
                out = self.model.render(rays_o, rays_d, staged=False, bg_color=None, perturb=self.perturb, **render_kw)
                loss = torch.nn.functional.mse_loss(out["image"], target)
            self.scaler.scale(loss).backward()
            self.scaler.unscale_(self.opt)
            self._reduce_grads(next_rays)
            self.scaler.step(self.opt)
            self.scaler.update()
            return loss.detach()
        # everything the route decision below reads, as one tuple: a step whose tuple equals that of the last step that
        # went the one-call route skips the checks (five `supported` walks, ~60 us of a 0.3 ms host budget)
        sig = None
        if self.native_step and not render_kw and (self.model.mean_count > 0 or getattr(self.model, "_cold_rows", 0) > 0):
            sig = self._route_signature(rays_o, rays_d, target, next_rays)
            if sig == self._native_route_sig:
                return self._step_rgb_native(rays_o, rays_d, target, next_rays, data_parallel=self._native_route_dp,
                                             checked=True)
        self._pending_sig = sig
        if self._manual_ok(rays_o, rays_d, target, render_kw):
            return self._step_rgb_manual(rays_o, rays_d, target, next_rays, **render_kw)
        self.opt.zero_grad(set_to_none=True)
        out = self.model.render(rays_o, rays_d, staged=False, bg_color=None, perturb=self.perturb, **render_kw)
        loss = torch.nn.functional.mse_loss(out["image"], target)
        loss.backward()
        self._reduce_grads(next_rays)
        self.opt.step()
        return loss.detach()

    def step_frames(self, batch, opt=None, sampler=None):
        """One frame training step: the reference's Trainer.train_step (nerf/utils.py:575-636) + the optimizer part of
        train_one_epoch, on a FrameSampler batch ("rays_o", "rays_d" [B,N,3], "images" [B,N,C or C+1]).  A per-pixel
        random background (white with a background model), alpha images mixed onto it, `opt.color_space == "linear"`
        converted, per-ray squared error; with `sampler` and the batch's "index" / "inds_coarse" the per-ray error is
        written back into the sampler's error map.  `opt` (EventOptions-like, optional) gives out_dim_color, color_space
        and render_kwargs.  Autograd through model.render in every regime, with that regime's optimizer and scaler
        protocol; under strat_f16 the stratified route's fp16 regime when it serves the render.  With `closed_frames`
        the plain fp32 one-GPU step goes without autograd (_frames_closed_ok, _step_frames_closed)."""
        m = self.model
        C = int(getattr(opt, "out_dim_color", None) or getattr(m, "out_dim_color", 3))
        kw = dict(getattr(opt, "render_kwargs", None) or {})
        kw.setdefault("out_dim_color", C)
        rays_o, rays_d, images = batch["rays_o"], batch["rays_d"], batch["images"]
        if getattr(opt, "color_space", "srgb") == "linear":
            from .evaluate import srgb_to_linear
            images = torch.cat([srgb_to_linear(images[..., :C]), images[..., C:]], dim=-1)
        bg = 1 if m.bg_radius > 0 else torch.rand_like(images[..., :C])     # (pixel-wise random, nerf/utils.py:593)
        closed = self._frames_closed_ok(rays_o, rays_d, images, bg, kw)
        if closed:
            gt = None       # (the alpha mix, the per-ray error and the loss gradient come out of the compositing launch)
        elif images.shape[-1] == C + 1:
            gt = images[..., :C] * images[..., C:] + bg * (1 - images[..., C:])
        else:
            gt = images
        if closed:
            per_ray = self._step_frames_closed(rays_o, rays_d, images, bg, kw)
        elif self.strat_f16:
            per_ray = self._strat_f16_step(lambda: self._step_frames(rays_o, rays_d, gt, bg, kw),
                                           self._strat_f16_ok(rays_o, rays_d, kw, bg))
        elif self.amp_bf16 or self.amp_f16:
            prev = self._amp_scope()
            self.fp16 = self.amp_f16                # (fp16: the autocast route with the same scaler, as step_rgb's)
            try:
                per_ray = self._step_frames(rays_o, rays_d, gt, bg, kw)
            finally:
                self.fp16 = False
                self._amp_restore(prev)
        else:
            per_ray = self._step_frames(rays_o, rays_d, gt, bg, kw)
        if sampler is not None and "inds_coarse" in batch and "index" in batch:
            sampler.update_error(batch["index"], batch["inds_coarse"], per_ray)
        if self.lr_scheduler is not None:
            self.lr_scheduler.step()
        return per_ray.mean()

    def _closed_frames_regime(self):
        """Where the closed frame term may run at all: switched on, the plain fp32 regime, one GPU, no captured graphs."""
        return (self.closed_frames and not (self.fp16 or self.amp_bf16 or self.amp_f16 or self.strat_f16)
                and self.avg is None and not self.use_graphs and getattr(self.model, "graph_counter", None) is None)

    def _frames_closed_ok(self, rays_o, rays_d, images, bg, kw):
        """step_frames takes fused_render.train_step_frames: the regime above, fp32 pixels of C or C + 1 channels, render
        keywords the raw render knows, a render the fused route serves (no background model: `supported` refuses)."""
        if not (self._closed_frames_regime() and self.manual_mse and self.model.cuda_ray):
            return False
        from . import fused_render
        C = fused_render.channels(self.model)
        return (images.dtype == torch.float32 and images.device == rays_o.device and images.shape[-1] in (C, C + 1)
                and images.shape[:-1] == rays_o.shape[:-1] and kw.get("out_dim_color", C) == C
                and not set(kw) - {"dt_gamma", "max_steps", "out_dim_color"}
                and fused_render.supported(self.model, rays_o.contiguous().view(-1, 3), rays_d.contiguous().view(-1, 3), bg,
                                           kw.get("dt_gamma", 0)))

    def _fresh_grads(self, defer_table):
        """No gradient accumulates across steps -- except that the table's buffer is kept where the last Adam pass left it
        clean (see _manual_fwd_bwd); with `defer_table` the dense part of the table's gradient gets a home."""
        emb = self.model._modules["encoder"]._parameters["embeddings"]
        keep = self._reuse_cleared_grad(emb)
        for p in self._params:
            p.grad = None
        if keep is not None:
            emb.grad = keep
        elif defer_table:
            emb.grad = torch.zeros_like(emb)

    def _step_frames_closed(self, rays_o, rays_d, images, bg, kw):
        """_step_frames without autograd (one GPU, fp32): -> the per-ray loss [B,N]; the step is taken."""
        from . import fused_network, fused_render
        m = self.model
        if not m.training:
            m.train()
        self.maybe_update_extra_state()
        self.global_step += 1
        fuse_table = self.fuse_table_adam and hasattr(self.opt, "step_grid_table")
        march = {k: kw[k] for k in ("dt_gamma", "max_steps") if k in kw}

        def step(_own):
            self._fresh_grads(fuse_table)
            _, err, grads = fused_render.train_step_frames(m, rays_o, rays_d, images, bg, 1.0, self.perturb,
                                                           defer_table=fuse_table, **march)
            for p, g in zip(fused_network.network_params(m), grads):
                if g is not None:
                    p.grad = g.view_as(p)
            return err
        err = self._step_then_tail(False, step, None)
        self._optimizer_tail(fuse_table)
        return err.view(rays_o.shape[:-1])

    def _step_frames(self, rays_o, rays_d, gt, bg, kw):
        """-> the per-ray loss [B,N] fp32, detached; the step is taken."""
        if not self.model.training:
            self.model.train()
        self.maybe_update_extra_state()
        self.global_step += 1
        self.opt.zero_grad(set_to_none=True)

        def forward():
            out = self.model.render(rays_o, rays_d, staged=False, bg_color=bg, perturb=self.perturb, **kw)
            per_ray = ((out["image"] - gt) ** 2).mean(-1)
            return per_ray, per_ray.mean()
        if self.fp16:
            with torch.autocast("cuda", dtype=torch.float16, enabled=self._f16_autocast):
                per_ray, loss = forward()
            self.scaler.scale(loss).backward()
            self.scaler.unscale_(self.opt)
            self._reduce_grads()
            self.scaler.step(self.opt)
            self.scaler.update()
        else:
            per_ray, loss = forward()
            loss.backward()
            self._reduce_grads()
            self.opt.step()
        return per_ray.detach().float()

    def step_events(self, data, opt, next_data=None):
        """One event training step: two renders sharing one backward (nerf/utils.py:482-573)."""
        if self.strat_f16:
            # (events.train_step_events: both renders take a [B,1,C] background drawn on the device)
            bg = torch.empty((data["images"].shape[0], 1, opt.out_dim_color), device=data["rays_evs_o1"].device)
            kw = dict(opt.render_kwargs, out_dim_color=opt.render_kwargs.get("out_dim_color", opt.out_dim_color))
            native = (self._strat_f16_ok(data["rays_evs_o1"], data["rays_evs_d1"], kw, bg)
                      and self._strat_f16_ok(data["rays_evs_o2"], data["rays_evs_d2"], kw, bg))
            if native and not opt.event_only:
                # the frame term's render (events.train_step_events): no background, or for alpha images (C + 1 = 4
                # channels) a per-pixel one drawn like the frames' first out_dim_color channels
                images = data["images"]
                bg_frames = torch.empty_like(images[..., :opt.out_dim_color]) if images.shape[-1] == 4 else None
                native = self._strat_f16_ok(data["rays_o"], data["rays_d"], kw, bg_frames)
            loss = self._strat_f16_step(lambda: self._step_events(data, opt, next_data), native)
        elif self.amp_bf16 or self.amp_f16:
            prev = self._amp_scope()
            try:
                if self.amp_f16 and self._amp_closed_form_ok() and opt.event_only and self._events_manual_ok(data, opt):
                    loss = self._amp_step(self._step_events, data, opt, next_data)
                elif self.amp_f16:
                    self.fp16 = True
                    try:
                        loss = self._step_events(data, opt, next_data)
                    finally:
                        self.fp16 = False
                else:
                    loss = self._step_events(data, opt, next_data)
            finally:
                self._amp_restore(prev)
        else:
            loss = self._step_events(data, opt, next_data)
        if self.lr_scheduler is not None:
            self.lr_scheduler.step()
        return loss

    def _step_events(self, data, opt, next_data=None):
        from .events import train_step_events
        if not self.model.training:
            self.model.train()
        coming = None
        if (self.global_step % self.update_interval == 0 and self.overlap_update and not self.fp16 and opt.event_only
                and not opt.render_kwargs and self._events_manual_ok(data, opt)):
            # (the first render's count pass only: the marcher's chunk log holds ONE outstanding count pass, the second
            # render is marched whole once the first's write pass has run)
            coming = (data["rays_evs_o1"], data["rays_evs_d1"])
        self.maybe_update_extra_state(coming)
        self.global_step += 1
        from .events import wants_no_event_term
        no_ev = wants_no_event_term(opt)                 # two more renders per step: neither graphs nor the one-call step
        log = self._log                                  # (a logged step wants the terms and delta: not a graph's to give)
        if (log is None and opt.event_only and not no_ev
                and self._graphable(data["rays_evs_o1"], data["rays_evs_d1"])):
            names = ("images", "rays_evs_o1", "rays_evs_d1", "rays_evs_o2", "rays_evs_d2", "pols")
            key = self._graph_key("events", data["rays_evs_o1"])
            inputs = tuple(data[n] for n in names)
            if self._graph_for(key) is None:
                self._graphs[key] = self._capture(
                    inputs, lambda *ts: train_step_events(self.model, dict(zip(names, ts)), opt)[0])
            return self._replay(self._graphs[key], inputs, 2)
        if self.fp16:
            # the shipped configs' fp16 = True around the event step (nerf/utils.py:964-975): autocast + GradScaler
            self.opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.float16, enabled=self._f16_autocast):
                loss, *rest = train_step_events(self.model, data, opt, return_terms=log is not None)
            if log is not None:
                log.event_step(loss, rest[0], data["pols"], rest[1])
            self.scaler.scale(loss).backward()
            self.scaler.unscale_(self.opt)
            if self.avg is not None:
                self.avg()
            self.scaler.step(self.opt)
            self.scaler.update()
            return loss.detach()
        if self._events_manual_ok(data, opt):
            from .events import train_step_events_manual
            if (self.native_step and self.fuse_table_adam and self.avg is None and not self.use_graphs and not no_ev
                    and self.prefetch_at == "mlp_backward" and hasattr(self.opt, "grid_table_plan")
                    and getattr(self.model, "graph_counter", None) is None):
                from . import fused_render
                if fused_render.native_events_supported(self.model, data, opt, self.opt,
                                                        normalised=self.native_normalised):
                    return self._step_events_native(data, opt, next_data)
            side = None
            if next_data is not None and not opt.render_kwargs:
                side = self._side_prefetch((next_data["rays_evs_o1"], next_data["rays_evs_d1"]),
                                           (next_data["rays_evs_o2"], next_data["rays_evs_d2"]))
            fuse_table = (self.fuse_table_adam and self.avg is None and hasattr(self.opt, "step_grid_table")
                          and not self.use_graphs)
            emb = self.model.encoder.embeddings
            if self._reuse_cleared_grad(emb) is None:
                emb.grad = None
            try:
                tail = self.prefetch_at == "mlp_backward"
                loss, *rest = train_step_events_manual(self.model, data, opt, after_forward=None if tail else side,
                                                       after_mlp_backward=side if tail else None,
                                                       defer_table=fuse_table, return_terms=log is not None)
                if log is not None:
                    log.event_step(loss, rest[0], data["pols"], rest[1])
            except BaseException:
                self._discard_pending_records()
                raise
            self._reduce_grads()
            if fuse_table:
                enc = self.model.encoder
                self.opt.step_grid_table(enc.embeddings, enc.offsets, enc.level_dim, extra=self._small_params)
                self._cleared_grad = enc.embeddings.grad
            else:
                self._opt_step()
            return loss
        self.opt.zero_grad(set_to_none=True)
        loss, *rest = train_step_events(self.model, data, opt, return_terms=log is not None)
        if log is not None:
            log.event_step(loss, rest[0], data["pols"], rest[1])
        loss.backward()
        if self.avg is not None:
            self.avg()
        self.opt.step()
        return loss.detach()

    def _step_events_native(self, data, opt, next_data):
        """The steady-state event-only step as one library call (fused_render.train_step_events_native ->
        enerf_train_step_events): the launches of the manual route below, in its order, issued from C."""
        from . import fused_render
        m = self.model
        emb = m._modules["encoder"]._parameters["embeddings"]
        if self._reuse_cleared_grad(emb) is None:
            emb.grad = None
        nxt = None
        if (next_data is not None and self.prefetch and self.global_step % self.update_interval != 0
                and all(fused_render.supported(m, next_data[o].contiguous().view(-1, 3),
                                               next_data[d].contiguous().view(-1, 3), 1, 0)
                        for o, d in (("rays_evs_o1", "rays_evs_d1"), ("rays_evs_o2", "rays_evs_d2")))):
            if self._side is None:
                self._side = torch.cuda.Stream()
            nxt = next_data
        if (nxt is None and self.early_budget and self.prefetch and self.global_step % self.update_interval == 0
                and getattr(m, "_last_march_event", None) is None):
            fused_render.stage_ring_copy(m)     # (the window's last step, marches on this stream: see _step_rgb_native)
        try:
            loss, delta = fused_render.train_step_events_native(m, data, opt, self.opt, next_data=nxt, side_stream=self._side)
        except BaseException:
            self._discard_pending_records()
            raise
        if self._log is not None:
            # on the one-call step loss_evs IS the loss; `delta` is the step context's buffer, which the next step of this
            # shape overwrites: the estimate is queued now, on the step's stream
            self._log.event_step(loss, delta, data["pols"], dict(loss_evs=loss))
        self._cleared_grad = emb.grad
        return loss

    def _events_manual_ok(self, data, opt):
        from . import fused_render
        m = self.model
        ro, rd = data["rays_evs_o1"], data["rays_evs_d1"]
        if not opt.event_only and not self._event_frames_closed_ok(data, opt):
            return False
        return (self.manual_mse and m.cuda_ray
                and not set(opt.render_kwargs) - {"dt_gamma", "max_steps", "out_dim_color"}
                and fused_render.supported(m, ro.contiguous().view(-1, 3), rd.contiguous().view(-1, 3), 1,
                                           opt.render_kwargs.get("dt_gamma", 0)))

    def _event_frames_closed_ok(self, data, opt):
        """event_only = 0: the frame term of the step (the default MSE criterion -- the harness passes no other) goes the
        closed route too: the regime of _closed_frames_regime, fp32 frames without alpha or, at three channels, with one
        (train_step_events tells alpha images by their four channels, as the reference does), frame rays the fused
        render serves with the background they will get."""
        if not self._closed_frames_regime():
            return False
        from . import fused_render
        images, C = data["images"], int(opt.out_dim_color)
        if not (images.dtype == torch.float32 and images.device == data["rays_o"].device
                and C == fused_render.channels(self.model)
                and opt.render_kwargs.get("out_dim_color", C) == C
                and (images.shape[-1] == C or (C == 3 and images.shape[-1] == 4))
                and images.shape[:-1] == data["rays_o"].shape[:-1]):
            return False
        bg = torch.empty_like(images[..., :C]) if images.shape[-1] == C + 1 else 1
        return fused_render.supported(self.model, data["rays_o"].contiguous().view(-1, 3),
                                      data["rays_d"].contiguous().view(-1, 3), bg, opt.render_kwargs.get("dt_gamma", 0))
