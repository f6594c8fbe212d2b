"""The reference trainer's per-batch step (trainer.py:37-48) on the device path, single- or
multi-rank (molecule-sharded data parallelism, x2gnn.dist).

``Trainer.step(batch)`` = forward (xgnn_poly.forward) + smooth-L1 loss (trainer.py:41) +
backward (trainer.py:42) into one flat gradient bucket + the gradient / loss all-reduce
(N > 1; §8(e) of SURVEY.md) + clip_grad_norm_(100) + Adam + EMA (trainer.py:44-48), with the
reference's per-batch LinearWarmupExponentialDecay (scheduler.py, trainer.py:47) when
``lr_schedule`` is given (evaluated on the device, so captured replays follow it).
``capture()`` records the step as two HIP graphs — forward+loss+backward, and the update — with
the all-reduce eager between them, so a replay enqueues the same kernels as an eager step
without the ~500 Python-side launches (the eager step is launch-bound).

Under data parallelism every rank owns a shard of the global batch (``dist.shard_by_triplets``:
balanced by triplet count, so shards hold unequal molecule counts).  The reference's loss is the
mean over the whole batch, so each rank's gradient of its own shard mean is weighted by
``local_count / global_count`` before the SUM all-reduce (``GradBucket.allreduce_mean``); the
shard's loss rides in the bucket's trailing slot, so the global mean loss comes out of the same
collective.

The rest of the reference's epoch: ``Trainer.run_epoch`` (the epoch loss, trainer.py:45,50),
``Trainer.evaluate`` / ``Evaluator`` (the validation MAE on the averaged weights, trainer.py:52-58)
and ``Trainer.state_dict`` / ``load_state_dict`` (trainer.py:99-105) — sums kept on the device, one
host sync per epoch or split.
"""
from __future__ import annotations

import math

import torch
import torch.distributed as dist

from . import ops
from .dist import GradBucket
from .optim import FlatAdam, ParamSwap


def _world(group=None):
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group)
    return 1


class Trainer:
    """One training step over a resident batch with a flat gradient bucket.

    ``local_count`` / ``global_count``: molecules in this rank's shard / in the global batch
    (host ints from the sharding); None = every rank holds the same count (plain mean)."""

    def __init__(self, model, lr=1e-3, max_norm=100.0, ema_decay=0.95, local_count=None, global_count=None,
                 group=None, lr_schedule=None, exchange_chunks=1, skip_nonfinite=False):
        """``lr_schedule``: None (constant ``lr``) or a dict of LinearWarmupExponentialDecay's
        arguments — warmup_steps, decay_steps, decay_rate[, staircase] (config.json: 3000, 3e6,
        0.01) — applied per step from base ``lr`` (FlatAdam.set_schedule).  ``exchange_chunks``: the
        gradient all-reduce as that many asynchronous collectives over contiguous bucket ranges
        (GradBucket.allreduce_mean(chunks=...)), joined before the optimizer.  ``skip_nonfinite``: the update
        skips, on the device, a step whose gradient norm is not finite (FlatAdam; ``opt.skipped`` counts them;
        the count is a per-run diagnostic and is not part of ``state_dict``)."""
        self.model = model
        self.group = group
        self.multi = _world(group) > 1
        # one trailing float: the shard's loss, all-reduced together with the gradients
        self.bucket = GradBucket(model.parameters(), extra=1 if self.multi else 0)
        # clip_grad_norm_(100) + Adam(1e-3) + EMA(0.95) (config.json) in three launches over the
        # flat parameter / gradient buffers (x2gnn.optim.FlatAdam, csrc/optim.hip)
        self.opt = FlatAdam(model.parameters(), lr=lr, max_norm=max_norm, ema_decay=ema_decay, bucket=self.bucket,
                            skip_nonfinite=skip_nonfinite)
        if lr_schedule is not None:
            self.opt.set_schedule(base_lr=lr, **lr_schedule)
        self.flat_launches = []  # [(rows, cols) per job] of the last backward's flat weight-gradient launches
        self.counts = (local_count, global_count)
        self.exchange_chunks = int(exchange_chunks)
        self.graphs = None
        self.loss = None
        self.grads_zeroed = False  # the bucket starts zeroed too; the first step zeroes it anyway
        # d loss / d loss, kept: autograd's per-step ones_like fill is skipped
        self.seed = torch.ones((), device=self.bucket.flat.device)
        # run_epoch's (sum of loss * molecules, molecules), allocated here like every buffer a step touches
        self.epoch_acc = torch.zeros(2, dtype=torch.float64, device=self.bucket.flat.device)
        self._evaluators = {}  # evaluate()'s, by weights

    def forward_backward(self, batch):
        """Forward + loss + backward into the bucket (no exchange, no update); returns the loss."""
        if not self.grads_zeroed:  # otherwise the previous update zeroed them (FlatAdam.step(zero_grads=True))
            self.bucket.zero()
        self.grads_zeroed = False
        self.model.train()  # trainer.py:30 (an Inference sharing the model may have left it in eval)
        res = self.model(batch)
        # trainer.py:41; the loss launch also writes d loss / d res for the seed (no backward launch)
        loss = ops.smooth_l1_loss(res, batch.y, unit_seed=self.seed)
        with ops.deferred_wgrad() as d:  # all layers' weight-gradient slab sums in one launch
            torch.autograd.backward(loss, self.seed)
        self.flat_launches = d.flat_launches
        if self.multi:
            self.bucket.extra_view.copy_(loss.detach().reshape(1))
        return loss

    def reduce(self):
        """The step's only exchange (N > 1): gradients + loss, count-weighted SUM all-reduce."""
        if not self.multi:
            return
        local, total = self.counts
        if local is None:
            self.bucket.allreduce_mean(group=self.group, chunks=self.exchange_chunks)
        else:
            self.bucket.allreduce_mean(group=self.group, local_count=local, global_count=total,
                                       chunks=self.exchange_chunks)

    def global_loss(self, local_loss):
        """The global-batch mean loss after ``reduce()`` (the shard's loss when single-rank)."""
        return self.bucket.extra_view[0] if self.multi else local_loss

    def update(self):
        self.opt.step(zero_grads=True)
        self.grads_zeroed = True

    def step(self, batch):
        """One step; returns the (global) loss as a device scalar.  After ``capture()`` it is the
        graph's own loss buffer — valid until the next step overwrites it (the CUDA / HIP graph output
        contract): read it (``float(loss)``) or ``clone()`` it to keep it.  (Copying it out on every step
        was a 4.6 µs launch of its own.)"""
        if self.graphs is None:
            loss = self.forward_backward(batch)
            self.reduce()
            self.update()
            return self.global_loss(loss)
        self.replay_forward_backward()
        self.reduce()
        self.graphs[1].replay()
        self.grads_zeroed = True
        return self.global_loss(self.loss)

    def replay_forward_backward(self):
        """Replay the captured forward+loss+backward (accumulates into the bucket: zeroed by the
        previous update, or by the caller); returns the captured loss tensor."""
        self.graphs[0].replay()
        self.grads_zeroed = False
        return self.loss

    def capture(self, batch, warm=3):
        """Record forward+backward and the update as two HIP graphs (warm-up passes on a side
        stream first: forward+backward+exchange only, the parameters are not updated)."""
        drop = self._dropout_state()
        held = None if drop is None else drop.clone()  # (the warm-up passes draw masks: not steps of the run)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warm):
                self.forward_backward(batch)
                self.reduce()
        torch.cuda.current_stream().wait_stream(side)
        if held is not None:
            drop.copy_(held)
        # the forward+backward graph accumulates into a zeroed bucket and does not zero it itself:
        # the update graph's last kernel does (FlatAdam.step(zero_grads=True)), so a replayed step
        # has no fill launch; a caller replaying g_fb alone zeroes the bucket first
        self.bucket.zero()
        self.grads_zeroed = True
        g_fb, g_up = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_fb):
            self.loss = self.forward_backward(batch)
        with torch.cuda.graph(g_up):
            self.update()
        self.graphs = (g_fb, g_up)
        self.grads_zeroed = True  # (nothing ran during capture: the bucket is still the zeroed one)

    # ------------------------------------------------------------------ the rest of the reference's epoch
    def averaged(self):
        """Context manager: inside it the model's parameters are the average's views (FlatAdam.averaged)."""
        return self.opt.averaged(self.model)

    def evaluator(self, weights="ema"):
        """A new ``Evaluator`` on the averaged weights ("ema": ``opt.ema`` read in place) or the live ones
        ("model")."""
        if weights not in ("ema", "model"):
            raise ValueError(f"weights must be 'ema' or 'model', not {weights!r}")
        if weights == "model":
            return Evaluator(self.model)
        return Evaluator(self.model, swap=self.opt.average_swap())

    def evaluate(self, batches, std=1.0, weights="ema"):
        """Train_EMA.test (trainer.py:52-58): ``std`` * the mean absolute error over every molecule of
        ``batches`` (anything ``model()`` takes, e.g. a ``DeviceDataset.loader(..., shuffle=False,
        indices=val)``), on the averaged weights by default.  One host sync, at the end.  This rank's
        batches only (see Evaluator)."""
        ev = self._evaluators.get(weights)
        if ev is None:
            ev = self._evaluators[weights] = self.evaluator(weights)
        return ev.run(batches, std=std)["mae"]

    def run_epoch(self, batches):
        """Train_EMA.epoch (trainer.py:33-50): ``step(batch)`` per batch, each followed by one eager launch that
        adds ``loss * num_graphs`` and ``num_graphs`` to a device accumulator (``loss.item() * num_graphs``
        without the per-batch sync; outside the captured graphs, which are replayed as they are); one sync at
        the end; returns the epoch's mean loss per molecule.  Under data parallelism the loss is the global
        one and the weight the global batch's molecule count."""
        acc = self.epoch_acc
        acc.zero_()
        for batch in batches:
            loss = self.step(batch)
            ops.weighted_accum(loss, self._global_count(batch), acc)
        a = acc.cpu()  # the epoch's one sync
        return float(a[0]) / float(a[1])

    def _global_count(self, batch):
        if not self.multi:
            return batch.num_graphs
        total = self.counts[1]
        return total if total is not None else batch.num_graphs * _world(self.group)

    def _dropout_state(self):
        """The trunk's attention-dropout (seed, step) buffer when the model trains with dropout, else None."""
        trunk = getattr(self.model, "fin_model", self.model)
        if getattr(trunk, "attn_dropout", 0.0) > 0:
            return trunk.attn_dropout_state
        return None

    def _names(self):
        """The optimizer's parameters by their names in the model, and the model's full state (detached
        aliases of the live tensors: parameters and buffers)."""
        named = [(n, p) for n, p in self.model.named_parameters() if p.requires_grad]
        if len(named) != len(self.opt.params) or any(p is not q for (_, p), q in zip(named, self.opt.params)):
            raise RuntimeError("the optimizer does not hold this model's parameters")
        return [n for n, _ in named], self.model.state_dict()

    def state_dict(self):
        """Everything a run resumes from (the reference saves model, optimizer, scheduler and epoch,
        trainer.py:99-105), keyed by parameter NAME, so it does not depend on the flat layout::

            {"format": 1, "model": {name: tensor}, "ema": {name: tensor},
             "optimizer": {"exp_avg": {name: tensor}, "exp_avg_sq": {name: tensor}, "scalars": float32[16]}}

        plus ``"attn_dropout_state"``: int64 [2] (seed, step) when the model has attention dropout, so a resumed
        run draws the masks the uninterrupted one would.
        ``scalars`` carries the step count and the learning-rate schedule.  Every tensor is a clone
        (``torch.save`` takes the dict as it is).  "model" and "ema" have the model's own ``state_dict()`` keys
        — entries the optimizer does not average (buffers, frozen parameters) are the model's in both — so
        ``xgnn_poly(...).load_state_dict(sd["ema"])`` is the averaged model."""
        names, live = self._names()
        opt = self.opt

        def by_name(flat):
            return {n: flat[off:off + p.numel()].view_as(p).clone() for n, p, off in zip(names, opt.params,
                                                                                         opt.offsets)}

        model = {k: v.clone() for k, v in live.items()}
        ema = dict(model)
        if opt.ema is not None:
            ema.update(by_name(opt.ema))
        sd = {"format": 1, "model": model, "ema": ema,
              "optimizer": {"exp_avg": by_name(opt.exp_avg), "exp_avg_sq": by_name(opt.exp_avg_sq),
                            "scalars": opt.scalars.clone()}}
        drop = self._dropout_state()
        if drop is not None:
            sd["attn_dropout_state"] = drop.clone()
        return sd

    def load_state_dict(self, sd):
        """Copy a ``state_dict()`` INTO the existing flat buffers (``copy_``; nothing is rebound, so graphs
        captured before the call keep replaying on the same addresses, now on the loaded state).  Raises
        KeyError on a missing or unexpected name and ValueError on a shape mismatch, before anything is
        copied."""
        if sd.get("format") != 1:
            raise ValueError(f"unknown trainer state format {sd.get('format')!r}")
        names, live = self._names()
        opt = self.opt
        o = sd["optimizer"]
        views = {
            "model": live,
            "ema": dict(live) if opt.ema is None else {**live, **dict(zip(names, opt.ema_params()))},
            "exp_avg": {n: opt.exp_avg[off:off + p.numel()].view_as(p) for n, p, off in zip(names, opt.params,
                                                                                            opt.offsets)},
            "exp_avg_sq": {n: opt.exp_avg_sq[off:off + p.numel()].view_as(p) for n, p, off in zip(names, opt.params,
                                                                                                  opt.offsets)},
        }
        given = {"model": sd["model"], "ema": sd["ema"], "exp_avg": o["exp_avg"], "exp_avg_sq": o["exp_avg_sq"]}
        for part, dst in views.items():
            src = given[part]
            missing, extra = sorted(set(dst) - set(src)), sorted(set(src) - set(dst))
            if missing or extra:
                raise KeyError(f"trainer state '{part}': missing {missing}, unexpected {extra}")
            for n, d in dst.items():
                if tuple(src[n].shape) != tuple(d.shape):
                    raise ValueError(f"trainer state '{part}': {n} has shape {tuple(src[n].shape)}, "
                                     f"expected {tuple(d.shape)}")
        if tuple(o["scalars"].shape) != tuple(opt.scalars.shape):
            raise ValueError(f"trainer state 'scalars' has shape {tuple(o['scalars'].shape)}")
        drop = self._dropout_state()
        if drop is not None and "attn_dropout_state" not in sd:
            raise KeyError("trainer state: missing 'attn_dropout_state' (the model has attention dropout)")
        if drop is not None and tuple(sd["attn_dropout_state"].shape) != (2,):
            raise ValueError(f"trainer state 'attn_dropout_state' has shape {tuple(sd['attn_dropout_state'].shape)}")
        with torch.no_grad():
            if drop is not None:
                drop.copy_(sd["attn_dropout_state"])
            for part, dst in views.items():
                if part == "ema" and opt.ema is None:
                    continue
                for n, d in dst.items():
                    if part == "ema" and n not in views["exp_avg"]:
                        continue  # (not averaged: the model's own entry, loaded with "model")
                    d.copy_(given[part][n])
            opt.scalars.copy_(o["scalars"])


class Inference:
    """Config 5's step: the model forward on a resident batch (trainer.test's path without the
    MAE, trainer.py:52-58), captured in one HIP graph; ``step`` returns the energies' sum."""

    def __init__(self, model):
        self.model = model
        self.graph = None
        self.out = None

    def _fwd(self, batch):
        was = self.model.training  # eval for the forward (trainer.py:54), the caller's mode restored
        self.model.eval()
        try:
            with torch.no_grad():
                return self.model(batch).sum()
        finally:
            self.model.train(was)

    def step(self, batch):
        if self.graph is None:
            return self._fwd(batch)
        self.graph.replay()
        return self.out

    def capture(self, batch, warm=2):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warm):
                self._fwd(batch)
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = self._fwd(batch)


def _num_triplets(batch):
    """The batch's triplet count from its host metadata (as GraphPlan.from_atom_batch takes it)."""
    from .data import _meta_from_tensors

    host_meta = getattr(batch, "host_meta", None)
    meta = host_meta() if callable(host_meta) else _meta_from_tensors(batch)
    return int(meta["triplets"].sum())


class Evaluator:
    """Train_EMA.test's loop body (trainer.py:52-58) without its per-batch ``.item()``: an eval-mode, no-grad
    forward on a chosen parameter set, and the batch's error statistics added to a device accumulator
    (ops.error_accum: sum |e - y|, sum (e - y)^2, max |e - y|, count, in fp64, fixed order).

    ``params``: None (the model's own weights) or tensors shaped like the model's parameters — like all of
    ``model.parameters()``, or like the trainable ones (``FlatAdam.ema_params()``) — which the model reads IN
    PLACE during the forward (optim.ParamSwap: no parameter bytes are copied per evaluation; ``targets``
    names the Parameters they stand in for when it is neither of the two).  As in the reference, where
    ``ema_model(data)`` renormalises the averaged embedding table (atom_embedding.py:14), a forward
    renormalises the rows of ``params``' embedding table for the elements present in the batch; the live
    weights are not touched.

    ``update`` never syncs with the host; ``result`` is the only sync.  ``capture`` records forward +
    accumulate as ONE HIP graph on a resident batch.  The graph holds the addresses of ``params``: captured on
    the average's views it reads ``FlatAdam.ema``, which never moves, so a replay after further training steps
    evaluates the CURRENT average, not the one at capture time.

    Single-rank: the four numbers cover the batches this process was given.  Ranks that evaluate disjoint
    slices of a split add their accumulators (sums, sums, max, counts) themselves; no collective runs here."""

    def __init__(self, model, params=None, targets=None, swap=None):
        """``swap``: a ready ``optim.ParamSwap`` instead of ``params`` (Trainer.evaluator passes the
        optimizer's, which restores the training views it knows without reading them back)."""
        self.model = model
        self.swap = swap
        if params is not None:
            params = list(params)
            if targets is None:
                targets = list(model.parameters())
                if len(targets) != len(params):
                    targets = [p for p in targets if p.requires_grad]
            self.swap = ParamSwap(targets, params)  # (checks counts and shapes now, not at the first batch)
        dev = next(model.parameters()).device
        # allocated here, outside any capture: the graph and the eager path add into the same four doubles
        # (a K-target model, ``model.num_target`` = K > 1: one row of four per target, ops.error_accum_cols)
        self.num_target = int(getattr(model, "num_target", 1))
        self.acc = torch.zeros((self.num_target, 4) if self.num_target > 1 else 4, dtype=torch.float64, device=dev)
        self.graph = None
        self.out = None

    def reset(self):
        """Zero the accumulator (stream-ordered, no sync)."""
        self.acc.zero_()

    def _update(self, batch):
        was = self.model.training  # eval for the forward (trainer.py:54), the caller's mode restored
        if self.swap is not None:
            self.swap.enter()
        try:
            self.model.eval()
            with torch.no_grad():
                e = self.model(batch)
        finally:
            if self.swap is not None:
                self.swap.leave()
            self.model.train(was)
        y = batch.y
        if y.dtype != torch.float32 or not y.is_contiguous():
            y = y.to(torch.float32).contiguous()
        if self.num_target > 1:
            ops.error_accum_cols(e, y.view(e.shape), self.acc)
        else:
            ops.error_accum(e, y, self.acc)
        return e

    def update(self, batch):
        """Forward on the chosen weights + accumulate; returns the energies [B].  After ``capture()`` it
        replays the graph (``batch`` is then the resident one it was captured on) and returns the graph's own
        output buffer, valid until the next replay."""
        if self.graph is None:
            return self._update(batch)
        self.graph.replay()
        return self.out

    def capture(self, batch, warm=2):
        """Record ``update`` on a resident batch as one HIP graph (warm-up passes on a side stream first; the
        accumulator is left as it was).  A batch the tiled inference attention would take (more than
        ``ops.INFER_TILE`` triplets) is refused: its tiles are whole-molecule ranges from the batch's host
        counts, baked into the graph."""
        if _num_triplets(batch) > ops.INFER_TILE:
            raise ValueError(f"cannot capture an evaluation of more than ops.INFER_TILE = {ops.INFER_TILE} triplets: "
                             "the tiled inference attention's ranges come from per-molecule host counts")
        held = self.acc.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warm):
                self._update(batch)
        torch.cuda.current_stream().wait_stream(side)
        self.acc.copy_(held)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self.out = self._update(batch)
        self.graph = graph

    def result(self, std=1.0):
        """The only sync: ``{"mae": std * acc0 / acc3, "rmse": std * sqrt(acc1 / acc3), "max_abs": std * acc2,
        "count": int(acc3)}`` (``std``: the targets' scale, trainer.py:57).  A K-target model: ``std`` a number or
        K numbers, ``mae`` / ``rmse`` / ``max_abs`` lists of K (per target), ``count`` the molecules."""
        if self.num_target > 1:
            a = self.acc.cpu().tolist()
            if a[0][3] <= 0:
                raise ValueError("nothing was evaluated since the last reset")
            try:
                stds = [float(v) for v in std]
            except TypeError:
                stds = [float(std)] * self.num_target
            if len(stds) != self.num_target:
                raise ValueError(f"{len(stds)} scales for {self.num_target} targets")
            return {"mae": [s * r[0] / r[3] for s, r in zip(stds, a)],
                    "rmse": [s * math.sqrt(r[1] / r[3]) for s, r in zip(stds, a)],
                    "max_abs": [s * r[2] for s, r in zip(stds, a)], "count": int(a[0][3])}
        a = [float(v) for v in self.acc.cpu()]
        if a[3] <= 0:
            raise ValueError("nothing was evaluated since the last reset")
        return {"mae": std * a[0] / a[3], "rmse": std * math.sqrt(a[1] / a[3]), "max_abs": std * a[2],
                "count": int(a[3])}

    def run(self, batches, std=1.0):
        """``reset``, ``update`` per batch, ``result``."""
        self.reset()
        for batch in batches:
            self.update(batch)
        return self.result(std=std)
