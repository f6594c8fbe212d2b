"""Two measurements around ``x2gnn.fit`` (profiles/fit_time.json); one JSON line.  Nothing is gated on them.

(a) What the non-finite guard costs a training step: config 2's resident batch (S160, B = 128), captured steps, two
    trainers on the same weights, ``skip_nonfinite`` off and on.  Interleaved rounds as scripts/dropout_step_time.py:
    every round times STEPS replays of each after WARM warm-up replays, the off trainer twice per round so that its
    own spread stands beside the difference.  Every gradient is finite: this is the cost of the guard that never
    fires (two more words written and four scalars routed through the workspace).

(b) What the epoch loop adds: one ``fit`` epoch (train + validation, no checkpoint, no log) over a synthetic S160
    dataset of MOLS molecules, against the same loop written by hand with ``run_epoch`` / ``evaluate``, interleaved,
    each on a trainer of its own from the same weights.

    python scripts/fit_time.py"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x2-gnn_amd"))
import x2gnn  # noqa: E402
from x2gnn.data import collate  # noqa: E402
from x2gnn.datasets import split_indices  # noqa: E402
from x2gnn.synth import synthetic_molecules  # noqa: E402
from x2gnn.train import Trainer  # noqa: E402

CFG = dict(conv_layers=4, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)  # config.json
BATCH, WARM, STEPS, ROUNDS = 128, 10, 100, 5
MOLS, DIVISION, EPOCH_ROUNDS = 1024, (128, 256), 15


def timed(fn, steps=STEPS):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def trainer(dev, **kw):
    torch.manual_seed(0)
    return Trainer(x2gnn.xgnn_poly(device="cuda", **CFG).to(dev), **kw)


def guard_cost(dev):
    batch = collate(synthetic_molecules(BATCH, "S160", seed=3000)).to(dev)
    off, on = trainer(dev), trainer(dev, skip_nonfinite=True)
    off.capture(batch)
    on.capture(batch)
    off.step(batch), on.step(batch)
    same = bool(torch.equal(on.opt.flat, off.opt.flat) and torch.equal(on.opt.scalars, off.opt.scalars))
    fns = {"off": lambda: off.step(batch), "on": lambda: on.step(batch), "off_again": lambda: off.step(batch)}
    legs = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            legs[k].append(timed(fn))
    torch.cuda.synchronize()
    off_all = legs["off"] + legs["off_again"]
    off_ms, on_ms = float(np.median(off_all)), float(np.median(legs["on"]))
    return {"config": "config 2, S160, B = 128, captured steps", "steps": STEPS, "warmup": WARM, "rounds": ROUNDS,
            "off_ms_per_round": [round(v, 4) for v in legs["off"]],
            "off_again_ms_per_round": [round(v, 4) for v in legs["off_again"]],
            "on_ms_per_round": [round(v, 4) for v in legs["on"]],
            "off_ms": round(off_ms, 4), "on_ms": round(on_ms, 4),
            "off_spread_ms": round(max(off_all) - min(off_all), 4),
            "cost_ms_per_step": round(on_ms - off_ms, 4), "cost_percent": round(100 * (on_ms / off_ms - 1), 2),
            "skipped": int(on.opt.skipped), "first_step_bitwise_equal": same}


def loop_overhead(dev):
    ds = x2gnn.DeviceDataset(synthetic_molecules(MOLS, "S160", seed=4000), dev)
    split = split_indices(MOLS, DIVISION, 41)
    _, val_idx, train_idx = split
    a, b = trainer(dev), trainer(dev)

    def by_fit():
        x2gnn.fit(a, ds, split, epochs=1, batch_size=BATCH)

    def by_hand():
        b.run_epoch(ds.loader(BATCH, shuffle=False, seed=0, indices=train_idx))
        b.evaluate(ds.loader(BATCH, shuffle=False, indices=val_idx), 1.0)

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    by_fit(), by_hand()  # warm-up epoch of each
    legs = {"hand": [], "fit": [], "hand_again": []}
    for _ in range(EPOCH_ROUNDS):
        legs["hand"].append(once(by_hand))
        legs["fit"].append(once(by_fit))
        legs["hand_again"].append(once(by_hand))
    hand_all = legs["hand"] + legs["hand_again"]
    hand_ms, fit_ms = float(np.median(hand_all)), float(np.median(legs["fit"]))
    what = (f"{MOLS} synthetic S160 molecules, B = {BATCH}: {len(train_idx)} train "
            f"({-(-len(train_idx) // BATCH)} eager steps), {len(val_idx)} validation")
    return {"dataset": what, "rounds": EPOCH_ROUNDS,
            "hand_ms_per_epoch": [round(v, 2) for v in legs["hand"]],
            "hand_again_ms_per_epoch": [round(v, 2) for v in legs["hand_again"]],
            "fit_ms_per_epoch": [round(v, 2) for v in legs["fit"]],
            "hand_ms": round(hand_ms, 2), "fit_ms": round(fit_ms, 2),
            "hand_min_ms": round(min(hand_all), 2), "fit_min_ms": round(min(legs["fit"]), 2),
            "hand_spread_ms": round(max(hand_all) - min(hand_all), 2),
            "fit_minus_hand_ms_per_epoch": round(fit_ms - hand_ms, 2),
            "fit_minus_hand_percent": round(100 * (fit_ms / hand_ms - 1), 2)}


def main():
    dev = torch.device("cuda:0")
    print(json.dumps({"name": "fit_time", "guard_cost": guard_cost(dev), "loop_overhead": loop_overhead(dev)}))


if __name__ == "__main__":
    main()
