"""The implicit contrast threshold on the host: enerf_amd/event_diag.py's statement against the reference's own
`estimate_C_thres_from_pol_dL` (tests/golden/ref_c_estimate.npz, minted by tests/refcheck/mint_c_estimate_golden.py with
the documented (N,1) / (N,C) shapes), and enerf_amd/train_log.py's TrainLog driven by stub steps on the CPU: the tags per
step kind, the row count, the JSON-lines round trip, the writer's call order."""
import math
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_c_estimate.npz")


def _cases():
    z = np.load(GOLDEN)
    names = sorted(k[:-len("_out")] for k in z.files if k.endswith("_out"))
    return z, names


def _same(got, want):
    """== with NaNs in the same places."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))


def test_fixture_covers_what_it_is_meant_to():
    z, names = _cases()
    assert os.path.getsize(GOLDEN) < 200 * 1024
    ns = {z[n + "_pols"].shape[0] for n in names}
    assert {1, 2, 3, 4} <= ns and max(ns) <= 4097
    assert {z[n + "_delta"].shape[1] for n in names} == {1, 3}
    assert any(np.isnan(z[n + "_out"]).any() for n in names)
    assert any((z[n + "_pols"] == 0).any() for n in names) and any((np.abs(z[n + "_pols"]) > 1).any() for n in names)
    assert any((z[n + "_pols"] > 0).all() for n in names) and any((z[n + "_pols"] < 0).all() for n in names)


@pytest.mark.parametrize("name", _cases()[1])
def test_statement_equals_the_reference(name):
    from enerf_amd.event_diag import NAMES, estimate_C_thres_statement
    z, _ = _cases()
    pols, delta = torch.from_numpy(z[name + "_pols"]), torch.from_numpy(z[name + "_delta"])
    est = estimate_C_thres_statement(pols, delta)
    assert tuple(est) == NAMES
    assert _same([float(est[k]) for k in NAMES], z[name + "_out"]), (name, est, z[name + "_out"])


@pytest.mark.parametrize("name", ["typical_c3", "accumulated_c1", "all_positive_c3", "one_nan_c1", "n3_c3"])
def test_estimate_on_the_cpu_is_the_statement_in_every_accepted_layout(name):
    from enerf_amd.event_diag import estimate_C_thres
    z, _ = _cases()
    pols, delta = torch.from_numpy(z[name + "_pols"]), torch.from_numpy(z[name + "_delta"])
    n, C = delta.shape
    want = z[name + "_out"]
    # the counts: n_class * C quotients (after the luma of the N == 3 branch: one per event)
    p, d0 = z[name + "_pols"][:, 0], z[name + "_delta"][:, 0]
    per = 1 if n == 3 else C
    if n == 3:
        d0 = (z[name + "_delta"] * np.array([0.299, 0.587, 0.114], np.float32)).sum(-1)
    counts = [int((p > 0).sum()) * per, int((p < 0).sum()) * per, int(((p > 0) & (d0 >= 0)).sum()) * per,
              int(((p < 0) & (d0 <= 0)).sum()) * per]
    for pp, dd in ((pols, delta), (pols[:, 0], delta), (pols[:, 0][None], delta[None]), (pols[None], delta[None])):
        med, cnt = estimate_C_thres(pp, dd)
        assert med.dtype == torch.float32 and cnt.dtype == torch.int32 and med.shape == cnt.shape == (4,)
        assert _same(med.numpy(), want) and cnt.tolist() == counts
    out = torch.full((8,), 7.0)
    med, cnt = estimate_C_thres(pols, delta, out=out)
    assert med.data_ptr() == out.data_ptr() and _same(out[:4].numpy(), want)
    assert out[4:].view(torch.int32).tolist() == counts


def test_estimate_refuses_a_batch_of_more_than_one_entry():
    from enerf_amd.event_diag import estimate_C_thres
    with pytest.raises(ValueError):
        estimate_C_thres(torch.ones(2, 5), torch.ones(2, 5, 1))
    with pytest.raises(ValueError):
        estimate_C_thres(torch.ones(4), torch.ones(5, 1))


def test_train_step_events_default_return_is_unchanged():
    import inspect
    from enerf_amd.events import train_step_events, train_step_events_manual
    for fn in (train_step_events, train_step_events_manual):
        assert inspect.signature(fn).parameters["return_terms"].default is False


# ---------------------------------------------------------------------------------------------------------- TrainLog
class _Writer:
    def __init__(self):
        self.calls = []

    def add_scalar(self, tag, value, step):
        self.calls.append((tag, value, step))


def _drive(log, kinds):
    """What TrainHarness does per step, with made-up numbers: -> the (pols, delta) of the event steps."""
    g = torch.Generator().manual_seed(5)
    fed = []
    log.begin(len(kinds), "cpu")
    for i, kind in enumerate(kinds):
        loss = torch.tensor(0.5 + i)
        if kind == "frames":
            log.frame_step(loss)
        else:
            pols = torch.where(torch.rand(1, 40, generator=g) < 0.5, 1.0, -1.0)
            delta = torch.randn(1, 40, 1, generator=g)
            terms = dict(loss_evs=torch.tensor(0.25 + i), loss_no_evs=None, loss_frames=None)
            if kind in ("events+no", "events+both"):
                terms["loss_no_evs"] = torch.tensor(0.125)
            if kind in ("events+frames", "events+both"):
                terms["loss_frames"] = torch.tensor(0.0625)
            log.event_step(loss, delta, pols, terms)
            fed.append((pols, delta))
        log.end_step(i + 1, 3, 0.01 * 0.5 ** i)
    return fed


KINDS = ["events", "frames", "events+no", "events+frames", "events+both", "frames"]
BASE = {"step", "train/loss", "train/epoch", "train/lr"}


def test_train_log_tags_per_step_kind_and_values(tmp_path):
    from enerf_amd.event_diag import NAMES, estimate_C_thres_statement
    from enerf_amd.train_log import C_TAGS, N_TAGS, TrainLog, read_jsonl
    path, writer = str(tmp_path / "log.jsonl"), _Writer()
    log = TrainLog(path=path, writer=writer)
    fed = _drive(log, KINDS)
    assert log.rows() == []                                  # nothing is formed before flush()
    new = log.flush()
    rows = log.rows()
    assert new == rows and len(rows) == len(KINDS)
    est_tags = set(C_TAGS) | set(N_TAGS)
    want_tags = {"events": BASE | {"train/loss_evs"} | est_tags, "frames": BASE,
                 "events+no": BASE | {"train/loss_evs", "train/loss_no_evs"} | est_tags,
                 "events+frames": BASE | {"train/loss_evs", "train/loss_frames"} | est_tags,
                 "events+both": BASE | {"train/loss_evs", "train/loss_no_evs", "train/loss_frames"} | est_tags}
    k = 0
    for i, (kind, rec) in enumerate(zip(KINDS, rows)):
        assert set(rec) == want_tags[kind], (kind, sorted(rec))
        assert rec["step"] == i + 1 and rec["train/epoch"] == 3 and rec["train/loss"] == 0.5 + i
        assert rec["train/lr"] == 0.01 * 0.5 ** i
        if kind != "frames":
            assert rec["train/loss_evs"] == 0.25 + i
            pols, delta = fed[k]
            k += 1
            est, counts = estimate_C_thres_statement(pols[0][:, None], delta[0], with_counts=True)
            assert [rec[t] for t in C_TAGS] == [float(est[n]) for n in NAMES]
            assert [rec[t] for t in N_TAGS] == counts
    # the JSON-lines file round-trips the records
    assert read_jsonl(path) == rows
    # the writer: step order, and within a step the record's own order, which is the reference's add_scalar order
    assert [c[2] for c in writer.calls] == sorted(c[2] for c in writer.calls)
    assert [(t, v, s) for t, v, s in writer.calls] == [(t, v, r["step"]) for r in rows for t, v in r.items() if t != "step"]
    first = [t for t, _, s in writer.calls if s == 5]
    assert first[:6] == ["train/loss", "train/epoch", "train/loss_evs", "train/loss_no_evs", "train/loss_frames", "train/lr"]
    assert first[6:10] == list(C_TAGS)


def test_train_log_without_implicit_C_and_across_flushes(tmp_path):
    from enerf_amd.train_log import TrainLog, read_jsonl
    path = str(tmp_path / "log.jsonl")
    log = TrainLog(implicit_C=False, path=path)
    _drive(log, ["events", "frames"])
    log.flush()
    _drive(log, ["events+no"])
    log.flush()
    assert log.flush() == []
    rows = log.rows()
    assert [set(r) for r in rows] == [BASE | {"train/loss_evs"}, BASE, BASE | {"train/loss_evs", "train/loss_no_evs"}]
    assert read_jsonl(path) == rows


def test_train_log_nan_median_survives_the_file(tmp_path):
    from enerf_amd.train_log import TrainLog, read_jsonl
    path = str(tmp_path / "log.jsonl")
    log = TrainLog(path=path)
    log.begin(1, "cpu")
    delta = torch.tensor([[[1.0], [float("nan")], [-1.0], [2.0]]])
    log.event_step(torch.tensor(1.0), delta, torch.tensor([[1.0, 1.0, -1.0, -1.0]]), dict(loss_evs=torch.tensor(1.0)))
    log.end_step(1, 1, 0.01)
    log.flush()
    rec = read_jsonl(path)[0]
    assert math.isnan(rec["train/est_C_med_on"]) and rec["train/est_C_med_off"] == -2.0
    assert rec["train/est_C_n_on"] == 2 and rec["train/est_C_n_on_sign"] == 1


def test_train_one_epoch_with_a_log_on_stub_steps(tmp_path):
    """TrainHarness.train_one_epoch(log=...) around stubbed steps: one row per step, frames and events told apart, the lr
    read after the step, the mean of train/loss equal to the epoch's mean loss, nothing kept on the harness afterwards."""
    from enerf_amd.train_log import TrainLog
    from enerf_amd.trainer import TrainHarness

    class Sampler:
        def __len__(self):
            return 4

        def batch(self, idx):
            i = idx[0]
            if i % 2:
                return {"rays_o": None, "i": i}
            return {"rays_evs_o1": None, "i": i, "pols": torch.tensor([[1.0, -1.0, 1.0, 1.0, -1.0]]),
                    "delta": torch.tensor([[[0.2], [-0.1], [0.4], [-0.3], [0.5]]]) * (i + 1)}

    h = TrainHarness.__new__(TrainHarness)
    h.model = torch.nn.Linear(1, 1)
    h.opt = torch.optim.SGD(h.model.parameters(), lr=0.5)
    h.ema, h.epoch, h.global_step, h.stats, h._log = None, 7, 0, {"loss": []}, None
    seen = []

    def step_events(data, opt, nxt):
        h.global_step += 1
        seen.append(h._log)
        loss = torch.tensor(0.1 * (data["i"] + 1))
        h._log.event_step(loss, data["delta"], data["pols"], dict(loss_evs=loss))
        h.opt.param_groups[0]["lr"] *= 0.5
        return loss

    def step_frames(data, opt, sampler):
        h.global_step += 1
        h.opt.param_groups[0]["lr"] *= 0.5
        return torch.tensor(0.1 * (data["i"] + 1))

    h.step_events, h.step_frames = step_events, step_frames
    log = TrainLog()
    mean = h.train_one_epoch(Sampler(), None, order=[0, 1, 2, 3], log=log)
    rows = log.rows()
    assert len(rows) == 4 and all(s is log for s in seen) and h._log is None
    assert [r["step"] for r in rows] == [1, 2, 3, 4] and all(r["train/epoch"] == 7 for r in rows)
    assert [r["train/lr"] for r in rows] == [0.25, 0.125, 0.0625, 0.03125]
    assert ["train/loss_evs" in r for r in rows] == [True, False, True, False]
    assert rows[0]["train/est_C_med_on"] == pytest.approx(0.2) and rows[0]["train/est_C_n_off"] == 2
    assert abs(sum(r["train/loss"] for r in rows) / 4 - mean) <= 1e-7 and h.stats["loss"] == [mean]
