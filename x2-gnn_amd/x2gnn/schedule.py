"""Host-side learning-rate schedules for a ``FlatAdam``: ``Plateau``, the reference's ReduceLROnPlateau
(train_ema.py:52-53).

``Plateau`` is ``torch.optim.lr_scheduler.ReduceLROnPlateau(mode='min', threshold_mode='rel')`` restated for an
optimizer whose learning rate is one device scalar: a reduction calls ``opt.set_lr(new_lr)``, a write into the
scalar block the update kernels read, so a captured update graph follows it at its next replay.

Why it steps once per epoch on the validation MAE: the reference calls ``scheduler.step()`` after every batch with
no metric (trainer.py:47).  For ReduceLROnPlateau that call raises TypeError (``step()`` needs ``metrics``), so the
reference's plateau branch never ran as written; stepping per epoch on the validation error, the quantity its
``best`` logic already tracks, is the only reading that runs, and it is how ReduceLROnPlateau is meant to be used.

``FlatAdam.set_lr`` clears a device-side warmup / decay schedule (``set_schedule``): the first reduction of a
``Plateau`` ends such a schedule.  The reference uses one or the other (train_ema.py:50-53), never both.
"""
from __future__ import annotations

import math


class Plateau:
    """``step(metric)`` once per epoch.  The current rate is kept as a host float (``lr``); ``step`` never reads
    the device.  ``lr``: the optimizer's current rate; None reads it from the optimizer once, here, at
    construction (the one device read of this class)."""

    def __init__(self, opt, factor, patience, min_lr, threshold=1e-4, cooldown=0, eps=1e-8, lr=None):
        if factor >= 1.0:
            raise ValueError("Factor should be < 1.0.")
        self.opt = opt
        self.factor, self.patience, self.min_lr = float(factor), int(patience), float(min_lr)
        self.threshold, self.cooldown, self.eps = float(threshold), int(cooldown), float(eps)
        self.lr = float(opt.lr) if lr is None else float(lr)
        self.best = math.inf
        self.num_bad_epochs = 0
        self.cooldown_counter = 0
        self.last_epoch = 0

    def step(self, metric):
        """ReduceLROnPlateau.step: returns the learning rate after it."""
        current = float(metric)
        self.last_epoch += 1
        if current < self.best * (1.0 - self.threshold):  # mode 'min', threshold_mode 'rel'
            self.best = current
            self.num_bad_epochs = 0
        else:
            self.num_bad_epochs += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0  # bad epochs in the cooldown do not count
        if self.num_bad_epochs > self.patience:
            new_lr = max(self.lr * self.factor, self.min_lr)
            if self.lr - new_lr > self.eps:
                self.lr = new_lr
                self.opt.set_lr(new_lr)
            self.cooldown_counter = self.cooldown
            self.num_bad_epochs = 0
        return self.lr

    _STATE = ("lr", "best", "num_bad_epochs", "cooldown_counter", "last_epoch")

    def state_dict(self):
        """What a resumed run continues from (host numbers only)."""
        return {k: getattr(self, k) for k in self._STATE}

    def load_state_dict(self, sd):
        """The state of a saved schedule.  The optimizer's own rate is part of the trainer's state (its scalar
        block), so nothing is written to the device here."""
        missing = [k for k in self._STATE if k not in sd]
        if missing:
            raise KeyError(f"plateau state: missing {missing}")
        for k in self._STATE:
            setattr(self, k, type(getattr(self, k))(sd[k]))
