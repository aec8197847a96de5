"""TrainHarness.train_one_epoch(log=TrainLog()) on the three routes a harness takes an event step through today -- the
stratified fp16 route of the shipped configs (cuda_ray off, fp16 = True), the Python-driven marching route and the
one-call native step -- on a small model and 256 event pairs; one configuration with C = 1 without luma per route, and C = 3
with luma (and the no-event term) on the marching route.

  (a) training is undisturbed: three steps with a log against three without, from the same seed -- the losses and every
      parameter bit-equal;
  (b) the logged medians are the statement's (event_diag.estimate_C_thres_statement on the CPU) on that step's delta and
      polarities, the logged terms sum to the logged loss with the step's weights, absent terms are absent;
  (c) what a logged step adds -- the row's writes and the estimate -- runs under torch.cuda.set_sync_debug_mode("error");
  (d) the epoch: one row per step, the mean of train/loss equal to stats["loss"][-1].
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAIRS = 256


def _rays(n_batches, seed=11):
    from enerf_amd import scene
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [scene.training_batch(b, PAIRS, DEV, generator=g)[0] for b in range(n_batches)]


def _event_batches(C, n, no_events=False):
    rays = _rays(n + 2)
    g = torch.Generator(device=DEV).manual_seed(5)
    out = []
    for i in range(n):
        (o1, d1), (o2, d2), (o3, d3) = rays[i], rays[i + 1], rays[i + 2]
        pols = torch.randint(-2, 3, (1, PAIRS), device=DEV, generator=g).float()       # (zeros among them)
        data = {"images": torch.zeros(1, PAIRS, C, device=DEV), "pols": pols,
                "rays_evs_o1": o1.view(1, -1, 3), "rays_evs_d1": d1.view(1, -1, 3),
                "rays_evs_o2": o2.view(1, -1, 3), "rays_evs_d2": d2.view(1, -1, 3)}
        if no_events:
            data.update(rays_no_evs_o1=o2.view(1, -1, 3), rays_no_evs_d1=d2.view(1, -1, 3),
                        rays_no_evs_o2=o3.view(1, -1, 3), rays_no_evs_d2=d3.view(1, -1, 3))
        out.append(data)
    return out


class _Sampler:
    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def batch(self, idx):
        return self.batches[idx[0]]


ROUTES = {
    # name: (cuda_ray, C, harness keywords, harness switches, option keywords, a sample budget given up front, no-event term)
    # (the one-call step serves the steady state, where a sample budget exists: it is handed one, and the epoch starts
    #  past the update step that would re-derive it from step counters that are still empty)
    "stratified_fp16": (False, 1, dict(fp16=True), {}, dict(render_kwargs={"num_steps": 64, "upsample_steps": 0}), 0, False),
    "marching_manual": (True, 1, {}, dict(native_step=False), {}, 0, False),
    "marching_manual_luma_no_events": (True, 3, {}, dict(native_step=False),
                                       dict(use_luma=True, negative_event_sampling=True, w_no_ev=0.5), 0, True),
    "native_one_call": (True, 1, {}, {}, {}, 40000, False),
}


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32),
                                                                     b.contiguous().view(torch.int32))


def _pin_table_backward(monkeypatch, tape, replay):
    """The stratified route's table backward (backends._gridencoder.grid_encode_backward, flushed at once) does not
    repeat its own bits: measured on an MI355X, the same call on the same inputs into the same zeroed buffer differs in
    1000 - 2700 of the table gradient's elements (by <= 3e-8 of the scaled gradient), whatever the binning settings,
    while every other gradient of the step repeats exactly.  Two free runs of this route therefore never agree in their
    parameters -- without any log: 3977 table elements after three steps, by at most 5.4e-8 -- and say nothing about
    the log.  So the first run records, per call, that kernel's inputs and what it left in the gradient buffer; the
    second run still makes the call, is held to bit-equal INPUTS at every call (nothing upstream was disturbed), and
    goes on from the recorded output (so that everything downstream, the optimizer and the next steps, can be held to
    bit-equal results).  -> the number of calls seen so far, as a one-element list."""
    from enerf_amd import stratified
    gb = stratified._gb
    orig, n = gb.grid_encode_backward, [0]

    def call(dfeat, xyz, emb, offsets, g_emb, *a, **k):
        out = orig(dfeat, xyz, emb, offsets, g_emb, *a, **k)
        if not replay:
            tape.append((dfeat.clone(), xyz.clone(), emb.detach().clone(), g_emb.clone()))
        else:
            r_dfeat, r_xyz, r_emb, r_out = tape[n[0]]
            assert _bits_equal(dfeat, r_dfeat) and _bits_equal(xyz, r_xyz) and _bits_equal(emb.detach(), r_emb), n[0]
            g_emb.copy_(r_out)
        n[0] += 1
        return out
    monkeypatch.setattr(gb, "grid_encode_backward", call)
    return n


def _run(route, logged, monkeypatch, table_tape=None, replay=False):
    """One epoch of three steps: -> (harness, losses of the epoch's steps, log or None, the (pols, delta) each estimate
    saw, calls of the routes' step functions).  `table_tape`: see _pin_table_backward."""
    from enerf_amd import event_diag, events, fused_render, stratified
    from enerf_amd.events import EventOptions
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.train_log import TrainLog
    from enerf_amd.trainer import TrainHarness
    cuda_ray, C, hkw, switches, okw, budget, no_events = ROUTES[route]
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=cuda_ray, out_dim_color=C).to(DEV)
    h = TrainHarness(model, lr=1e-2, **dict(dict(occupancy="synthetic") if cuda_ray else {}, **hkw))
    for k, v in switches.items():
        setattr(h, k, v)
    opt = EventOptions(**dict(dict(out_dim_color=C, use_luma=False, linlog=True, C_thres=0.2, event_only=True), **okw))
    batches = _event_batches(C, 4, no_events)
    seen, calls, losses = [], {"native": 0, "manual": 0, "strat": stratified.stats["calls"]}, []
    orig_est = event_diag.estimate_C_thres
    monkeypatch.setattr(event_diag, "estimate_C_thres",
                        lambda p, d, out=None: (seen.append((p.clone(), d.clone())), orig_est(p, d, out=out))[1])
    orig_native, orig_manual = fused_render.train_step_events_native, events.train_step_events_manual
    monkeypatch.setattr(fused_render, "train_step_events_native",
                        lambda *a, **k: (calls.__setitem__("native", calls["native"] + 1), orig_native(*a, **k))[1])
    monkeypatch.setattr(events, "train_step_events_manual",
                        lambda *a, **k: (calls.__setitem__("manual", calls["manual"] + 1), orig_manual(*a, **k))[1])
    orig_step = h.step_events
    h.step_events = lambda *a, **k: (lambda loss: (losses.append(loss.detach().clone()), loss)[1])(orig_step(*a, **k))
    pinned = _pin_table_backward(monkeypatch, table_tape, replay) if table_tape is not None else None
    torch.manual_seed(3)                                 # the steps draw random background colours
    if budget:
        model.mean_count, h.global_step = budget, 1
    log = TrainLog() if logged else None
    h.train_one_epoch(_Sampler(batches), opt, order=[0, 1, 2], log=log)
    torch.cuda.synchronize()
    calls["strat"] = stratified.stats["calls"] - calls["strat"]
    calls["table_backward"] = pinned[0] if pinned is not None else None
    monkeypatch.undo()
    return h, torch.stack(losses).cpu(), log, seen, calls


def _took_its_route(route, h, calls):
    """The route the configuration is named for was the one taken."""
    if route == "native_one_call":
        return calls["native"] == 3 and calls["manual"] == 0
    if ROUTES[route][0]:
        return calls["manual"] == 3 and calls["native"] == 0
    return h.strat_f16 and calls["strat"] == 6 and calls["manual"] == calls["native"] == 0


@pytest.mark.parametrize("route", list(ROUTES))
def test_training_is_undisturbed_by_the_log(route, monkeypatch):
    """(a) Three steps with a log against three without, from the same seed: the losses and every parameter bit-equal.
    On the marching routes two free runs are compared: their sums have a fixed order.  On the stratified route the one
    kernel that does not repeat its own bits is pinned (_pin_table_backward): its inputs are held bit-equal at each of
    the six calls, and both runs go on from the same output."""
    tape = [] if route == "stratified_fp16" else None
    h0, l0, _, seen0, calls0 = _run(route, False, monkeypatch, tape)
    h1, l1, log, seen, calls = _run(route, True, monkeypatch, tape, replay=True)
    if tape is not None:
        assert len(tape) == 6 and calls0["table_backward"] == calls["table_backward"] == 6
    assert _took_its_route(route, h0, calls0) and _took_its_route(route, h1, calls)
    assert not seen0 and len(seen) == 3 and len(log.rows()) == 3
    assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)), (l0, l1)
    differ = {n: (int((p0 != p1).sum()), float((p0 - p1).abs().max()))
              for (n, p0), (_, p1) in zip(h0.model.named_parameters(), h1.model.named_parameters())
              if not torch.equal(p0.detach(), p1.detach())}
    print(route, "parameters that differ (elements, max abs):", differ)
    assert not differ, differ


@pytest.mark.parametrize("route", list(ROUTES))
def test_logged_epoch_holds_the_statements_values(route, monkeypatch):
    from enerf_amd.event_diag import NAMES, estimate_C_thres_statement
    from enerf_amd.train_log import C_TAGS, N_TAGS
    no_events = ROUTES[route][6]
    h1, l1, log, seen, calls = _run(route, True, monkeypatch)
    assert _took_its_route(route, h1, calls) and len(seen) == 3
    # (d) one row per step; the epoch's mean loss
    rows = log.rows()
    assert len(rows) == 3 and [r["step"] for r in rows] == [h1.global_step - 2, h1.global_step - 1, h1.global_step]
    assert [r["train/loss"] for r in rows] == [float(x) for x in l1]
    mean = float(np.mean(np.array([r["train/loss"] for r in rows], np.float64)))
    assert abs(mean - h1.stats["loss"][-1]) <= 3 * 2.0 ** -24 * abs(mean), (mean, h1.stats["loss"][-1])
    assert all(r["train/epoch"] == 1 and r["train/lr"] == h1.opt.param_groups[0]["lr"] for r in rows)
    # (b) the medians and counts of the step's own delta and polarities; the terms
    for rec, (pols, delta) in zip(rows, seen):
        assert pols.shape == (1, PAIRS) and delta.shape == (1, PAIRS, 1)
        est, counts = estimate_C_thres_statement(pols[0][:, None].cpu(), delta[0].cpu(), with_counts=True)
        want = np.array([float(est[k]) for k in NAMES], np.float32)
        got = np.array([rec[t] for t in C_TAGS], np.float32)
        print(route, rec["step"], "medians", got, "statement", want, "counts", counts)
        assert bool(np.all((got == want) | (np.isnan(got) & np.isnan(want)))), (got, want)
        assert [rec[t] for t in N_TAGS] == counts and sum(counts[:2]) < PAIRS
        assert "train/loss_frames" not in rec and ("train/loss_no_evs" in rec) == no_events
        total = np.float32(rec["train/loss_evs"])
        if no_events:
            assert rec["train/loss_no_evs"] >= 0.0
            total = total + np.float32(rec["train/loss_no_evs"])         # (w_no_ev is inside the term, as the reference's)
        assert abs(float(total) - rec["train/loss"]) <= 2.0 ** -23 * abs(rec["train/loss"]), (total, rec["train/loss"])


def test_a_logged_step_adds_no_host_synchronisation(monkeypatch):
    """The one-call native step with a log: everything the log does per step (TrainLog.event_step, end_step) runs with
    synchronisation made an error; flush() is the one read-back."""
    from enerf_amd.train_log import TrainLog
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=DEV).item()
            polices = False
        except RuntimeError:
            polices = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not polices:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this torch build")
    entered = []
    for name in ("event_step", "end_step"):
        orig = getattr(TrainLog, name)

        def guarded(self, *a, _orig=orig, _name=name, **k):
            torch.cuda.set_sync_debug_mode("error")
            try:
                entered.append(_name)
                return _orig(self, *a, **k)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        monkeypatch.setattr(TrainLog, name, guarded)
    _, _, log, _, calls = _run("native_one_call", True, monkeypatch)
    assert calls["native"] == 3 and entered == ["event_step", "end_step"] * 3 and len(log.rows()) == 3


def test_graph_replay_is_not_taken_by_a_logged_step_and_frame_steps_log_their_loss(monkeypatch):
    """use_graphs hands out nothing but the loss: a logged event step takes the next route.  A frame step logs loss,
    epoch and lr only."""
    from enerf_amd.events import EventOptions
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.train_log import TrainLog
    from enerf_amd.trainer import TrainHarness
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=1).to(DEV)
    h = TrainHarness(model, lr=1e-2, occupancy="synthetic", use_graphs=True)
    opt = EventOptions(out_dim_color=1, use_luma=False, linlog=True, C_thres=0.2, event_only=True)
    model.mean_count = 8192                              # (a sample budget: the condition of graph replay)
    captured = []
    monkeypatch.setattr(h, "_capture", lambda *a, **k: captured.append(1))
    batches = _event_batches(1, 2)
    (ro, rd) = _rays(1)[0]
    frames = {"rays_o": ro.view(1, -1, 3), "rays_d": rd.view(1, -1, 3), "images": torch.rand(1, PAIRS, 1, device=DEV)}
    log = TrainLog()
    h.global_step = 1                                    # (not an update step: mean_count stays)
    h.train_one_epoch(_Sampler([batches[0], frames, batches[1]]), opt, order=[0, 1, 2], log=log)
    rows = log.rows()
    assert not captured and len(rows) == 3
    assert set(rows[1]) == {"step", "train/loss", "train/epoch", "train/lr"}
    assert "train/est_C_med_on" in rows[0] and "train/loss_evs" in rows[2]
    assert rows[1]["train/loss"] > 0 and np.isfinite([r["train/loss"] for r in rows]).all()
