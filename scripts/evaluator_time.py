"""What an evaluation batch costs: x2gnn.train.Evaluator against Inference on config 2's resident batch (S160,
B = 128), in one process, legs interleaved; one JSON line.

Each of ROUNDS rounds times, over STEPS calls after WARM warm-up calls (time.perf_counter around a synchronised
loop),
  (a)  Inference.step, eager (the forward on the live weights + the energies' sum),
  (b)  Evaluator.update on the averaged weights, eager (the forward on FlatAdam.ema in place + x2g_error_accum),
  (c0) Inference.step replaying its captured graph,
  (c)  Evaluator.update replaying its captured graph,
so (a)'s and (c0)'s spreads over their repetitions are known beside the differences.  Also x2g_error_accum alone
(HIP events around the launch, median over 30 calls).

    python scripts/evaluator_time.py"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x2-gnn_amd"))
import x2gnn  # noqa: E402
from x2gnn import ops  # noqa: E402
from x2gnn.data import collate  # noqa: E402
from x2gnn.synth import synthetic_molecules  # noqa: E402
from x2gnn.train import Inference, Trainer  # noqa: E402

CFG = dict(conv_layers=4, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)  # config.json
BATCH, WARM, STEPS, ROUNDS = 128, 5, 30, 5


def timed(fn):
    """ms per call over STEPS calls after WARM warm-up calls."""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / STEPS


def accum_alone(e, y, acc, n=30, warm=5):
    """x2g_error_accum's GPU time in microseconds (events around the launch), median and minimum."""
    us = []
    for i in range(warm + n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.error_accum(e, y, acc)
        e1.record()
        torch.cuda.synchronize()
        if i >= warm:
            us.append(1e3 * e0.elapsed_time(e1))
    return round(float(np.median(us)), 2), round(min(us), 2)


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    tr = Trainer(x2gnn.xgnn_poly(device="cuda", **CFG).to(dev))
    batch = collate(synthetic_molecules(BATCH, "S160", seed=3000)).to(dev)
    for _ in range(3):  # an average that differs from the live weights
        tr.step(batch)
    inf_eager, inf_graph = Inference(tr.model), Inference(tr.model)
    ev_eager, ev_graph = tr.evaluator("ema"), tr.evaluator("ema")
    inf_graph.capture(batch)
    ev_graph.capture(batch)
    fns = {"inference_eager": lambda: inf_eager.step(batch), "evaluator_eager": lambda: ev_eager.update(batch),
           "inference_graph": lambda: inf_graph.step(batch), "evaluator_graph": lambda: ev_graph.update(batch)}
    legs = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            legs[k].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in legs.items()}
    spread = {k: max(v) - min(v) for k, v in legs.items()}
    e = ev_eager.update(batch)
    acc_us, acc_us_min = accum_alone(e, batch.y, ev_eager.acc)
    res = ev_eager.result()
    out = {"name": "evaluator_time", "config": "config 2, S160, B = 128", "steps": STEPS, "warmup": WARM,
           "rounds": ROUNDS}
    for k in fns:
        out[k + "_ms_per_call"] = [round(v, 4) for v in legs[k]]
        out[k + "_ms"] = round(med[k], 4)
        out[k + "_spread_ms"] = round(spread[k], 4)
    out.update({
        "eager_evaluator_minus_inference_ms": round(med["evaluator_eager"] - med["inference_eager"], 4),
        "graph_evaluator_minus_inference_ms": round(med["evaluator_graph"] - med["inference_graph"], 4),
        "error_accum_kernel_us": acc_us, "error_accum_kernel_us_min": acc_us_min,
        "eager_within_spread_plus_launch": bool(med["evaluator_eager"] - med["inference_eager"]
                                                <= spread["inference_eager"] + acc_us * 1e-3),
        "graph_within_spread_plus_launch": bool(med["evaluator_graph"] - med["inference_graph"]
                                                <= spread["inference_graph"] + acc_us * 1e-3),
        "molecules_evaluated": res["count"]})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
