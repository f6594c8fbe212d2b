"""The reference trainer's parameter update on flat buffers (trainer.py:39-48, train_ema.py:45-48).

``FlatAdam`` re-homes every parameter as a view of ONE flat fp32 buffer (the gradient side is
``dist.GradBucket``'s flat buffer), so clip_grad_norm_ + Adam + the EMA of AveragedModel are
two launches of ``x2g_clip_adam_ema`` over contiguous memory instead of torch's per-tensor
foreach/capturable kernels.  Step count, norm and bias corrections live on the device, so the
update can sit inside a captured HIP graph.
"""
from __future__ import annotations

import contextlib

import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from .dist import GradBucket, flat_layout

# slots of the float[16] device scalar block (X2G_OPT_* of include/x2g.h)
_LR, _B1, _B2, _EPS, _MAXN, _EMAD, _STEP, _NORM, _CLIP, _WARMUP, _DECAY_STEPS, _DECAY_RATE, _BASE_LR, _STAIRCASE = (
    _lib.CONSTS["OPT_" + n] for n in ("LR", "BETA1", "BETA2", "EPS", "MAX_NORM", "EMA_DECAY", "STEP", "NORM", "CLIP",
                                      "WARMUP", "DECAY_STEPS", "DECAY_RATE", "BASE_LR", "STAIRCASE"))


class FlatAdam:
    """Adam(lr, betas, eps, amsgrad=False) + clip_grad_norm_(max_norm) + EMA(decay) over flat buffers.

    ``params`` must all be fp32 CUDA tensors; they become views of ``self.flat`` (values kept).
    ``ema`` (a flat buffer, same layout) holds the AveragedModel parameters; ``ema_params()``
    returns them shaped like the model's parameters.

    ``skip_nonfinite=True``: every ``step`` is the guarded update (``x2g_clip_adam_ema_guard``,
    include/x2g_train.h).  A step whose gradient norm is inf or NaN (an inf / NaN gradient, or finite gradients
    whose sum of squares overflows fp32, a norm above about 1.8e19) is skipped on the device: parameters, both
    moments, the average, the step count and the learning-rate schedule stay as they were, the gradients are
    still zeroed when asked, and ``skipped`` / ``last_skipped`` (device int64 scalars, allocated here) count it.
    A step with a finite norm writes bit for bit what the unguarded one writes.  The decision needs no host read,
    so it holds inside a captured graph.  Under data parallelism every rank holds the same reduced bucket, forms
    the same norm and reaches the same verdict: no collective is added.  With the default ``False``, ``step``
    makes the one call it always made and nothing is allocated."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=100.0, ema_decay=0.95,
                 bucket: GradBucket | None = None, skip_nonfinite=False):
        self.params = [p for p in params if p.requires_grad]
        dev = self.params[0].device
        self.offsets, n = flat_layout(self.params)  # same layout as GradBucket: 16-byte aligned views
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        for p, off in zip(self.params, self.offsets):
            k = p.numel()
            self.flat[off:off + k].copy_(p.detach().reshape(-1))
            p.data = self.flat[off:off + k].view_as(p)
        self.bucket = bucket if bucket is not None else GradBucket(self.params)
        if self.bucket.offsets != self.offsets:
            raise ValueError("gradient bucket does not cover the same parameters")
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        self.ema = self.flat.clone() if ema_decay is not None else None
        sc = torch.zeros(16, dtype=torch.float32)
        sc[[_LR, _B1, _B2, _EPS, _MAXN, _EMAD]] = torch.tensor(
            [lr, betas[0], betas[1], eps, max_norm if max_norm else 0.0, ema_decay or 0.0], dtype=torch.float32)
        self.scalars = sc.to(dev)
        self.skip_nonfinite = bool(skip_nonfinite)
        # [skipped steps, whether the last step was skipped]: written by the guarded update only
        self.guard = torch.zeros(2, dtype=torch.int64, device=dev) if self.skip_nonfinite else None
        lib = _lib.load()
        self.ws_bytes = int((lib.x2g_optimizer_guard_workspace if self.skip_nonfinite
                             else lib.x2g_optimizer_workspace)(n))
        self.ws = torch.empty(max(self.ws_bytes, 4), dtype=torch.uint8, device=dev)

    def step(self, zero_grads=False):
        """One update; ``zero_grads``: also zero the gradient bucket as it is read (zero_grad()
        folded into the step's last kernel, so the next backward needs no fill)."""
        if self.skip_nonfinite:
            call("x2g_clip_adam_ema_guard", ptr(self.flat), ptr(self.bucket.flat), ptr(self.exp_avg),
                 ptr(self.exp_avg_sq), ptr(self.ema), self.flat.numel(), ptr(self.scalars),
                 _lib.CONSTS["OPT_ZERO_GRADS"] if zero_grads else 0, ptr(self.guard), ptr(self.ws), self.ws_bytes,
                 stream_ptr())
            return
        call("x2g_clip_adam_ema_ex", ptr(self.flat), ptr(self.bucket.flat), ptr(self.exp_avg), ptr(self.exp_avg_sq),
             ptr(self.ema), self.flat.numel(), ptr(self.scalars),
             _lib.CONSTS["OPT_ZERO_GRADS"] if zero_grads else 0, ptr(self.ws), self.ws_bytes, stream_ptr())

    def set_lr(self, lr):
        """A fixed learning rate from the next step on (clears a schedule; e.g. for a host-side
        ReduceLROnPlateau, train_ema.py:52-53)."""
        self.scalars[_WARMUP] = 0.0
        self.scalars[_LR] = lr

    def set_schedule(self, warmup_steps, decay_steps, decay_rate, staircase=False, base_lr=None):
        """LinearWarmupExponentialDecay (scheduler.py:4-31; train_ema.py:50-51) evaluated on the device
        from the step count at every update, so captured HIP graphs follow it: update t (0-based)
        uses base_lr * min(1/W + t/W, 1) * decay_rate^(t / decay_steps), as the reference's
        LambdaLR gives optimizer.step() when scheduler.step() follows every batch (trainer.py:47)."""
        if decay_rate > 1:
            raise ValueError("decay_rate must be <= 1 (scheduler.py:16)")
        base = float(self.scalars[_LR]) if base_lr is None and float(self.scalars[_WARMUP]) <= 0 else base_lr
        base = float(self.scalars[_BASE_LR]) if base is None else float(base)
        vals = torch.tensor([max(int(warmup_steps), 1), float(decay_steps), float(decay_rate), base,
                             1.0 if staircase else 0.0], dtype=torch.float32)
        self.scalars[_WARMUP:_STAIRCASE + 1] = vals.to(self.scalars.device)

    @property
    def lr(self):
        """The learning rate the last update used (device scalar)."""
        return self.scalars[_LR]

    @property
    def grad_norm(self):
        return self.scalars[_NORM]

    @property
    def steps(self):
        return self.scalars[_STEP]

    @property
    def skipped(self):
        """The steps the guard has skipped (device int64 scalar; a per-run diagnostic, not part of any saved
        state).  Without ``skip_nonfinite`` there is no guard: ValueError."""
        return self._guard_word(0)

    @property
    def last_skipped(self):
        """Whether the last step was skipped (device int64 scalar, 0 or 1)."""
        return self._guard_word(1)

    def _guard_word(self, i):
        if self.guard is None:
            raise ValueError("this optimizer has no guard (skip_nonfinite=False)")
        return self.guard[i]

    def ema_params(self):
        return [self.ema[off:off + p.numel()].view_as(p) for p, off in zip(self.params, self.offsets)]

    def averaged(self, model=None):
        """Context manager: inside it the optimizer's parameters read the average in place (``ParamSwap``
        onto ``ema_params()``); on leaving it, after an exception too, they are the training views of ``flat``
        again, and ``model``'s train / eval mode (when a model is given) is what it was."""
        return self.average_swap().active(model)

    def average_swap(self):
        """The ``ParamSwap`` of the parameters onto the average's views, restoring the views of ``flat``
        this optimizer gave them (kept, so a swap reads no ``.data`` back)."""
        if self.ema is None:
            raise ValueError("this optimizer keeps no average (ema_decay=None)")
        home = [self.flat[off:off + p.numel()].view_as(p) for p, off in zip(self.params, self.offsets)]
        return ParamSwap(self.params, self.ema_params(), restore=home)


class ParamSwap:
    """Parameters that can read another set of tensors in place: ``enter()`` makes ``values[i]`` the ``.data`` of
    ``params[i]`` (same shape, dtype and device, checked once here: a pointer rebinding, no bytes are copied),
    ``leave()`` gives each its former storage back (``restore[i]`` when given, else what ``enter`` found), and
    ``active(model)`` is the two as a context manager that also restores ``model.training``.

    Every ops call takes its weight pointers at call time and nothing caches them, so a forward between the
    two reads ``values`` in place — and writes them where a forward writes its weights: the embedding's
    max_norm renormalisation (ops.embedding_table) then acts on ``values``, as the reference's
    ``ema_model(data)`` renormalises the averaged table (atom_embedding.py:14).  The Parameter objects stay,
    so their ``.grad`` views into the GradBucket and the ``_x2g_grad_sink`` marks are untouched, and so are the
    flat buffers that captured training graphs replay on (those hold addresses, not Parameter objects).

    The cost is host time only: two ``.data`` assignments per parameter and evaluation."""

    def __init__(self, params, values, restore=None):
        self.params, values = list(params), list(values)
        for name, ts in (("values", values), ("restore", restore)):
            if ts is None:
                continue
            if len(self.params) != len(ts):
                raise ValueError(f"{len(ts)} {name} for {len(self.params)} parameters")
            for p, v in zip(self.params, ts):
                if p.shape != v.shape or p.dtype != v.dtype or p.device != v.device or not v.is_contiguous():
                    raise ValueError(f"cannot stand in for a parameter of shape {tuple(p.shape)}: "
                                     f"{tuple(v.shape)} {v.dtype} on {v.device}")
        self.values = [v.detach() for v in values]
        self.restore = None if restore is None else [v.detach() for v in restore]
        self.held = None

    def enter(self):
        if self.held is not None:
            raise RuntimeError("these parameters are swapped already")
        self.held = self.restore if self.restore is not None else [p.data for p in self.params]
        for p, v in zip(self.params, self.values):
            p.data = v

    def leave(self):
        held, self.held = self.held, None
        for p, h in zip(self.params, held):
            p.data = h

    @contextlib.contextmanager
    def active(self, model=None):
        was = None if model is None else model.training
        self.enter()
        try:
            yield
        finally:
            self.leave()
            if model is not None:
                model.train(was)


def swap_params(params, values, model=None):
    """``ParamSwap(params, values).active(model)``: inside the context every parameter has the matching tensor
    of ``values`` as its ``.data``; on leaving it, after an exception too, its former storage is back."""
    return ParamSwap(params, values).active(model)
