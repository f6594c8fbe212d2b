"""x2gnn.fit's epoch loop on a scripted stand-in trainer (CPU): when the test split is evaluated and the best
checkpoint written, the log lines, the per-epoch checkpoint, resume."""
import os
import re

import numpy as np
import pytest
import torch

# trainer.py:68, restated
FORMAT = ("{time_str}[lr]:{lr:.7f}\t[epoch]:{epoch:03d}\t[Loss]:{loss:.7f}\t[ValMAE]:{val_error:.7f}\t"
          "[TestMAE]:{test_error:.7f}\n")


class Opt:
    lr = 1e-3


class Loader:
    def __init__(self, indices, **kw):
        self.indices, self.kw = list(indices), kw


class Dataset:
    def __init__(self):
        self.calls = []

    def loader(self, batch_size, shuffle=True, seed=0, drop_last=False, indices=None):
        ld = Loader(indices, batch_size=batch_size, shuffle=shuffle, seed=seed)
        self.calls.append(ld)
        return ld


class ScriptedTrainer:
    """Validation errors from a script; the test error of epoch e is 100 + e, the loss 10 + e."""

    def __init__(self, vals, split):
        self.vals, self.split = list(vals), [list(s) for s in split]
        self.opt = Opt()
        self.epoch = 0
        self.events = []

    def run_epoch(self, loader):
        assert loader.indices == self.split[2]
        self.events.append(("train", self.epoch, loader.kw["shuffle"], loader.kw["seed"]))
        return 10.0 + self.epoch

    def evaluate(self, loader, std=1.0):
        assert loader.kw["shuffle"] is False
        if loader.indices == self.split[1]:
            self.events.append(("val", self.epoch))
            v = self.vals[self.epoch]
            self.epoch += 1
            return std * v
        assert loader.indices == self.split[0]
        self.events.append(("test", self.epoch - 1))
        return std * (100.0 + self.epoch - 1)

    def state_dict(self):
        return {"format": 1, "epochs_done": self.epoch}

    def load_state_dict(self, sd):
        assert sd["format"] == 1
        self.epoch = sd["epochs_done"]


class Schedule:
    def __init__(self):
        self.seen = []

    def step(self, metric):
        self.seen.append(metric)

    def state_dict(self):
        return {"n": len(self.seen)}

    def load_state_dict(self, sd):
        self.seen = [None] * sd["n"]


SPLIT = (np.array([7, 8]), np.array([4, 5, 6]), np.array([0, 1, 2, 3]))
#        e: 0    1    2    3    4    5    6    7
VALS = [5.0, 4.0, 4.5, 3.0, 3.0, 3.5, 2.0, 2.0]
# best so far (ties count): e = 0, 1, 3, 4, 6, 7; past save_after = 2: 3, 4, 6, 7
SAVED = [3, 4, 6, 7]


def run(tmp_path, **kw):
    import x2gnn

    tr, ds, sched = ScriptedTrainer(VALS, SPLIT), Dataset(), Schedule()
    paths = {k: str(tmp_path / f"{k}.pt") for k in ("best", "last")}
    log = str(tmp_path / "run.log")
    hist = x2gnn.fit(tr, ds, SPLIT, epochs=len(VALS), batch_size=2, schedule=sched, save_after=2,
                     best_path=paths["best"], last_path=paths["last"], log_path=log, **kw)
    return tr, ds, sched, paths, log, hist


def test_when_the_test_split_is_evaluated_and_the_best_checkpoint_written(tmp_path, monkeypatch):
    import importlib

    fit_mod = importlib.import_module("x2gnn.fit")
    writes, inner = [], fit_mod._save

    def save(obj, path):
        writes.append((os.path.basename(path), obj["epoch"]))
        inner(obj, path)

    monkeypatch.setattr(fit_mod, "_save", save)
    tr, ds, sched, paths, log, hist = run(tmp_path)
    assert [e for kind, e, *_ in tr.events if kind == "test"] == SAVED  # a tie saves; nothing at e <= save_after
    assert [e for name, e in writes if name == "best.pt"] == SAVED
    assert [e for name, e in writes if name == "last.pt"] == list(range(len(VALS)))  # every epoch
    # the order inside an epoch: train, validate, then the test split
    assert tr.events[:2] == [("train", 0, False, 0), ("val", 0)]
    i = tr.events.index(("test", 3))
    assert tr.events[i - 2:i] == [("train", 3, False, 3), ("val", 3)]  # (seed + e; unshuffled by default)
    assert sched.seen == VALS
    bests = [5.0, 4.0, 4.0, 3.0, 3.0, 3.0, 2.0, 2.0]
    for e, h in enumerate(hist):
        assert h == {"epoch": e, "lr": 1e-3, "loss": 10.0 + e, "val": VALS[e], "best": bests[e], "skipped": 0,
                     "test": 100.0 + e if e in SAVED else None}
    best = torch.load(paths["best"], weights_only=True)
    assert best == {"format": 1, "epochs_done": 8, "epoch": 7, "best": 2.0, "schedule": {"n": 8}, "seed": 0}
    last = torch.load(paths["last"], weights_only=True)
    assert last == best
    assert sorted(os.listdir(tmp_path)) == ["best.pt", "last.pt", "run.log"]  # no temporary file remains


def test_the_log_lines_are_the_references(tmp_path):
    tr, ds, sched, paths, log, hist = run(tmp_path, std=2.0)
    lines = open(log).readlines()
    assert len(lines) == len(VALS)
    for e, line in enumerate(lines):
        stamp = line[:14]
        assert re.fullmatch(r"\d\d_\d\d_\d\d_\d\d_\d\d", stamp), line
        assert line == FORMAT.format(time_str=stamp, lr=1e-3, epoch=e + 1, loss=10.0 + e, val_error=2.0 * VALS[e],
                                     test_error=2.0 * (100.0 + e) if e in SAVED else -1.0)
    assert "[TestMAE]:-1.0000000\n" in lines[0]


def test_resume_continues_at_the_next_epoch_with_the_saved_best(tmp_path):
    import x2gnn

    full = run(tmp_path)[5]
    first = tmp_path / "first"
    first.mkdir()
    tr, ds, sched = ScriptedTrainer(VALS, SPLIT), Dataset(), Schedule()
    last = str(first / "last.pt")
    head = x2gnn.fit(tr, ds, SPLIT, epochs=5, batch_size=2, schedule=sched, save_after=2, last_path=last)
    assert head == full[:5]
    tr2, sched2 = ScriptedTrainer(VALS, SPLIT), Schedule()
    tail = x2gnn.fit(tr2, Dataset(), SPLIT, epochs=len(VALS), batch_size=2, schedule=sched2, save_after=2, resume=last)
    assert tail == full[5:]
    assert len(sched2.seen) == len(VALS) and sched2.seen[5:] == VALS[5:]
    assert not [e for kind, e, *_ in tr2.events if kind == "test" and e < 5]


def test_k_targets_follow_the_mean_of_the_unscaled_errors(tmp_path):
    import x2gnn

    class Multi(ScriptedTrainer):
        def evaluate(self, loader, std=1.0):
            v = super().evaluate(loader, 1.0)
            return [s * v for s in std]  # the same error on both targets, in the targets' units

    tr, sched = Multi([3.0, 1.0, 2.0], SPLIT), Schedule()
    log = str(tmp_path / "k.log")
    hist = x2gnn.fit(tr, Dataset(), SPLIT, epochs=3, std=(2.0, 10.0), schedule=sched, save_after=0, log_path=log)
    assert sched.seen == [3.0, 1.0, 2.0]
    assert [h["best"] for h in hist] == [3.0, 1.0, 1.0]
    assert hist[1]["val"] == [2.0, 10.0] and hist[1]["test"] == [202.0, 1010.0]
    lines = open(log).readlines()
    assert lines[1][14:] == FORMAT.format(time_str="", lr=1e-3, epoch=2, loss=11.0, val_error=1.0, test_error=606.0)
    with pytest.raises(ValueError):
        x2gnn.fit(Multi([1.0], SPLIT), Dataset(), SPLIT, epochs=1, std=(1.0, 0.0))  # no unscaled error
