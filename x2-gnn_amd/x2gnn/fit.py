"""The reference's training run around the step (trainer.py:89-116, ``Train_EMA.train``): ``fit``.

Per epoch: train on the train split, validate on the averaged weights, step the plateau schedule, evaluate the test
split and save when the validation error is the best so far (and the epoch is past ``save_after``), write one log
line.  The reference has no resume; ``Trainer.load_state_dict`` resumes bit for bit, so ``fit`` adds one.

``fit`` steps eagerly on fresh batches (``DeviceDataset.loader``).  It captures no graph per batch and pads no
batch: both routes ended in unexplained GPU faults and are out of the tree.  A trainer captured on
one resident batch is not what ``fit`` drives; single-rank only (``Trainer.counts`` is fixed at construction).
"""
from __future__ import annotations

import os
import time

import torch

# trainer.py:68
LOG_FORMAT = ("{time_str}[lr]:{lr:.7f}\t[epoch]:{epoch:03d}\t[Loss]:{loss:.7f}\t[ValMAE]:{val_error:.7f}\t"
              "[TestMAE]:{test_error:.7f}\n")


def _mean(v):
    """A K-target result (a list of per-target MAEs) as one number; a single-target one as it is."""
    return sum(v) / len(v) if isinstance(v, (list, tuple)) else v


def _criterion(val, std):
    """What ``best`` and the schedule follow: the validation MAE; for K targets the mean over targets of the
    UNSCALED (std = 1) MAEs, so that no target's unit dominates."""
    if not isinstance(val, (list, tuple)):
        return val
    try:
        stds = [float(s) for s in std]
    except TypeError:
        stds = [float(std)] * len(val)
    if len(stds) != len(val) or any(s == 0 for s in stds):
        raise ValueError(f"std {std!r} does not scale {len(val)} targets")
    return sum(v / s for v, s in zip(val, stds)) / len(val)


def _save(obj, path):
    """Written to a temporary file next to ``path`` and moved over it: a killed run leaves the old file whole."""
    tmp = f"{path}.tmp"
    torch.save(obj, tmp)
    os.replace(tmp, path)


def fit(trainer, dataset, split, epochs, batch_size=128, std=1.0, schedule=None, shuffle=False, seed=0,
        save_after=100, best_path=None, last_path=None, log_path=None, resume=None):
    """Train for ``epochs`` epochs as ``Train_EMA.train`` does; returns one dict per epoch run by this call.

    ``trainer``: a ``Trainer`` (anything with its ``run_epoch``, ``evaluate``, ``state_dict``, ``load_state_dict``
    and ``opt``); ``dataset``: a ``DeviceDataset``; ``split``: ``(test, val, train)`` index arrays
    (``datasets.split_indices``); ``schedule``: a ``schedule.Plateau`` or None.

    Epoch ``e`` (0-based), in the reference's order:

    * train: ``trainer.run_epoch(dataset.loader(batch_size, shuffle=shuffle, seed=seed + e, indices=train))``
      (``shuffle=False`` is the reference's regime, trainer.py:27: the same batches every epoch); one sync;
    * validate: ``trainer.evaluate(dataset.loader(batch_size, shuffle=False, indices=val), std)`` on the averaged
      weights; one sync.  A K-target model: ``std`` a number or K numbers, the result the K per-target MAEs, and
      the criterion the mean over targets of the unscaled MAEs (otherwise the criterion is the result);
    * ``schedule.step(criterion)``;
    * best: ``criterion <= best`` (a tie counts, as in the reference) updates ``best``; if also ``e > save_after``
      (the reference's ``epoch > 100``) the test split is evaluated and the checkpoint goes to ``best_path``:
      ``trainer.state_dict()`` plus ``{"epoch": e, "best": best, "schedule": schedule.state_dict() or None,
      "seed": seed}``, written to a temporary file and moved into place;
    * last: with ``last_path`` the same dict of this epoch, every epoch;
    * log: with ``log_path`` one line in the reference's format (``LOG_FORMAT``, trainer.py:68), ``epoch`` = e + 1,
      the test error -1.0 when it was not evaluated; for K targets the criterion and the mean test MAE.  ``lr`` is
      ``float(trainer.opt.lr)`` read AFTER the epoch, the rate of the epoch's last update, where the reference
      prints the rate at the epoch's start (one less device read per epoch; under a per-step schedule the two
      differ by one epoch of decay, under a plateau schedule by nothing: a reduction takes effect at the next
      update either way);
    * history: ``{"epoch", "lr", "loss", "val", "test" (None when not evaluated), "best", "skipped"}``, ``skipped``
      the non-finite guard's count so far (0 without the guard).

    ``resume``: the path of such a dict (``last_path``'s, usually).  It is loaded into the trainer and the schedule,
    and the run continues at its ``epoch + 1`` with its ``best``; the remaining epochs are the uninterrupted run's
    bit for bit (the epoch's batches depend on ``seed + e`` alone)."""
    test_idx, val_idx, train_idx = split
    best, start = None, 0
    if resume is not None:
        ckpt = torch.load(resume, weights_only=True)
        trainer.load_state_dict(ckpt)
        if schedule is not None and ckpt.get("schedule") is not None:
            schedule.load_state_dict(ckpt["schedule"])
        best, start = ckpt["best"], int(ckpt["epoch"]) + 1
    opt = trainer.opt
    history = []
    for e in range(start, epochs):
        loss = trainer.run_epoch(dataset.loader(batch_size, shuffle=shuffle, seed=seed + e, indices=train_idx))
        val = trainer.evaluate(dataset.loader(batch_size, shuffle=False, indices=val_idx), std)
        criterion = _criterion(val, std)
        if schedule is not None:
            schedule.step(criterion)
        test, improved = None, best is None or criterion <= best
        if improved:
            best = criterion
        saves = improved and e > save_after
        if saves:
            test = trainer.evaluate(dataset.loader(batch_size, shuffle=False, indices=test_idx), std)
        if (saves and best_path is not None) or last_path is not None:
            # taken after the epoch's last evaluation: the state the next epoch starts from
            ckpt = dict(trainer.state_dict())
            ckpt.update(epoch=e, best=best, schedule=None if schedule is None else schedule.state_dict(), seed=seed)
            if saves and best_path is not None:
                _save(ckpt, best_path)
            if last_path is not None:
                _save(ckpt, last_path)
        lr = float(opt.lr)
        if log_path is not None:
            with open(log_path, "a") as f:
                f.write(LOG_FORMAT.format(time_str=time.strftime("%m_%d_%H_%M_%S"), lr=lr, epoch=e + 1, loss=loss,
                                          val_error=criterion, test_error=-1.0 if test is None else _mean(test)))
        history.append({"epoch": e, "lr": lr, "loss": loss, "val": val, "test": test, "best": best,
                        "skipped": int(opt.skipped) if getattr(opt, "skip_nonfinite", False) else 0})
    return history
