"""The logging of the reference's Trainer.train_one_epoch (nerf/utils.py:975-989): per step the loss, its individual
terms and -- `--log_implicit_C_thres 1`, the reference's default -- the implicit contrast threshold's four medians
(enerf_amd/event_diag.py), under the reference's tags and conditions.

The reference reads every scalar back as it is made (`.item()`, and four torch.where inside the estimate): a stall of
the host after every step.  Here a step fills one fp32 row of a ring on the device -- the terms by one stack launch, the
medians and their counts by the one launch of enerf_event_c_estimate -- and the ring is read back ONCE, by flush(), which
TrainHarness.train_one_epoch calls at the end of the epoch.  The host-side scalars (step, epoch, lr) are noted as the
step is taken.  DESIGN.md 4.19.
"""
import json

import torch

from . import event_diag

# a row of the ring: the loss, the three terms, the four medians, the four counts (int32 bits)
_COLS = 12
_TERMS = ("loss_evs", "loss_no_evs", "loss_frames")
C_TAGS = ("train/est_C_med_on", "train/est_C_med_off", "train/est_C_med_on_sign", "train/est_C_med_off_sign")
N_TAGS = ("train/est_C_n_on", "train/est_C_n_off", "train/est_C_n_on_sign", "train/est_C_n_off_sign")


def _rank0():
    import torch.distributed as dist
    return not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0


class TrainLog:
    """TrainLog(implicit_C=True, path=None, writer=None) -> hand it to TrainHarness.train_one_epoch / train as `log`.

    Per step, keyed as the reference's writer.add_scalar calls are (nerf/utils.py:976-989):
      train/loss, train/epoch, train/lr      every step; lr is the value after the step's scheduler step
      train/loss_evs                         event steps
      train/loss_no_evs                      event steps while the no-event term is active
      train/loss_frames                      event steps with event_only = 0 (unweighted, as the reference logs it)
      train/est_C_med_{on,off,on_sign,off_sign}   event steps, with `implicit_C`
      train/est_C_n_{...}                    the numbers of quotients behind those medians (an addition)
    rows() -> the records flushed so far, one dict per step with "step" and the tags; `path`: each flush appends them to
    a JSON-lines file; `writer` (anything with add_scalar(tag, value, step): tensorboardX's SummaryWriter): each flush
    writes the scalars in step order.  Rank 0 logs its own batch, other ranks do nothing.  Not part of a checkpoint."""

    def __init__(self, implicit_C=True, path=None, writer=None):
        self.implicit_C = bool(implicit_C)
        self.path, self.writer = path, writer
        self.active = _rank0()
        self._ring = None
        self._zero = None
        self._cursor = 0
        self._pending = []            # the host's part of the rows not yet flushed
        self._rows = []

    # ---- the harness's side -------------------------------------------------------------------------------------------
    def begin(self, steps, device):
        """Room for `steps` more rows on `device` (what is pending is flushed first when the ring has to grow)."""
        need = self._cursor + int(steps)
        if self._ring is None or self._ring.device != torch.device(device) or self._ring.shape[0] < need:
            self.flush()
            self._ring = torch.zeros((max(int(steps), 1), _COLS), dtype=torch.float32, device=device)
            self._zero = torch.zeros((), dtype=torch.float32, device=device)

    def _row(self, device):
        if self._ring is None or self._cursor == self._ring.shape[0]:
            self.begin(max(64, self._cursor), device)     # (a step outside begin()'s count: flushes, i.e. one read-back)
        self._open = dict(kind="frames", terms=(), implicit=False)
        return self._ring[self._cursor]

    def event_step(self, loss, delta, pols, terms):
        """An event step's device part, on the current stream: the loss and the terms (`terms`: the dict of
        events.train_step_events(return_terms=True)) into the step's row by one launch, the medians of `delta` / `pols`
        by one more.  Nothing is read back."""
        row = self._row(loss.device)
        vals = [loss] + [terms.get(k) for k in _TERMS]
        present = tuple(k for k in _TERMS if terms.get(k) is not None)
        vals = [self._zero if v is None else v.detach().reshape(()).to(torch.float32) for v in vals]
        torch.stack(vals, out=row[:4])
        if self.implicit_C:
            event_diag.estimate_C_thres(pols.detach().to(torch.float32), delta.detach().to(torch.float32), out=row[4:])
        self._open = dict(kind="events", terms=present, implicit=self.implicit_C)

    def frame_step(self, loss):
        """A frame step's device part: its loss into the step's row."""
        row = self._row(loss.device)
        row[:1].copy_(loss.detach().reshape(1))

    def end_step(self, step, epoch, lr):
        """The host's part of the row just filled."""
        self._pending.append(dict(self._open, step=int(step), epoch=int(epoch), lr=float(lr)))
        self._cursor += 1

    # ---- the user's side ----------------------------------------------------------------------------------------------
    def flush(self):
        """Read the ring back (one copy), form the records, append them to `path`, hand them to `writer`."""
        if not self._pending:
            self._cursor = 0
            return []
        host = self._ring[:self._cursor].cpu()
        counts = host[:, 8:].contiguous().view(torch.int32)
        new = []
        for i, meta in enumerate(self._pending):
            # (in the reference's add_scalar order)
            rec = {"step": meta["step"], "train/loss": float(host[i, 0]), "train/epoch": meta["epoch"]}
            for j, k in enumerate(_TERMS):
                if k in meta["terms"]:
                    rec["train/" + k] = float(host[i, 1 + j])
            rec["train/lr"] = meta["lr"]
            if meta["implicit"]:
                for j in range(4):
                    rec[C_TAGS[j]] = float(host[i, 4 + j])
                for j in range(4):
                    rec[N_TAGS[j]] = int(counts[i, j])
            new.append(rec)
        self._pending, self._cursor = [], 0
        self._rows += new
        if self.path is not None:
            with open(self.path, "a") as f:
                for rec in new:
                    f.write(json.dumps(rec) + "\n")
        if self.writer is not None:
            for rec in new:
                for tag, value in rec.items():
                    if tag != "step":
                        self.writer.add_scalar(tag, value, rec["step"])
        return new

    def rows(self):
        return list(self._rows)


def read_jsonl(path):
    """The records of a TrainLog(path=...) file."""
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]
