"""What attention dropout costs a training step: config 2's resident batch (S160, B = 128), captured steps,
interleaved rounds; one JSON line (profiles/attn_dropout_time.json).

Leg 2 (always, one process): two trainers on the same weights, attn_dropout = 0 and P_DROP, each capturing its
step; every round times STEPS replays of each after WARM warm-up replays (time.perf_counter around a
synchronised loop), the p = 0 trainer twice per round so that its own spread is known beside the difference.
Then the center kernels alone, in an eager step of each trainer: HIP events around every center launch (a sleep
kernel ahead of the start event, as ops._timed does), the median over REPS steps of the per-step sum by entry.

Leg 1 (--base LIB: a libx2g.so built from the parent commit, scripts/build_base.sh): child processes of this
script (--child), X2G_LIB set to the base library or unset, each timing the p = 0 captured step like leg 2;
rounds alternate base, this tree, base, so the parent's spread against itself in the same session stands beside
the difference.  The base library has no staged entries: p = 0 never asks for one.

    python scripts/dropout_step_time.py [--base x2-gnn_amd/lib/ab/libx2g_base.so]"""
import argparse
import json
import os
import subprocess
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
from x2gnn.train import Trainer  # noqa: E402

CFG = dict(conv_layers=4, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)  # config.json
BATCH, WARM, STEPS, ROUNDS, REPS, P_DROP = 128, 10, 100, 5, 7, 0.1
CENTER = ("x2g_sbf_attention_fwd_center_sf", "x2g_sbf_attention_fwd_center_sf_tiled", "x2g_sbf_attention_bwd_center")


def timed(fn, steps=STEPS):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def trainer(dev, p):
    torch.manual_seed(0)
    kw = dict(attn_dropout=p) if p > 0 else {}  # (a base tree's xgnn_poly has no such argument)
    return Trainer(x2gnn.xgnn_poly(device="cuda", **CFG, **kw).to(dev))


def center_kernel_us(tr, batch):
    """{entry (without _drop): median over REPS eager steps of the step's summed launch times, microseconds}."""
    inner, evs = ops.call, []

    def rec(name, *args):
        base = name[:-5] if name.endswith("_drop") else name
        if base not in CENTER:
            return inner(name, *args)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(200_000)
        a.record()
        inner(name, *args)
        b.record()
        evs.append((base, a, b))

    sums = {k: [] for k in CENTER}
    ops.call = rec
    try:
        for i in range(REPS + 2):
            evs.clear()
            tr.forward_backward(batch)
            torch.cuda.synchronize()
            if i >= 2:
                for k in CENTER:
                    sums[k].append(sum(1e3 * a.elapsed_time(b) for n, a, b in evs if n == k))
    finally:
        ops.call = inner
    return {k: round(float(np.median(v)), 2) for k, v in sums.items() if any(v)}


def child():
    dev = torch.device("cuda:0")
    batch = collate(synthetic_molecules(BATCH, "S160", seed=3000)).to(dev)
    tr = trainer(dev, 0.0)
    tr.capture(batch)
    ms = [timed(lambda: tr.step(batch)) for _ in range(3)]
    print(json.dumps({"ms": [round(v, 4) for v in ms], "loss": float(tr.step(batch))}))


def leg1(base):
    runs = {"base": [], "this": []}
    for name in ("base", "this", "base", "this", "base"):
        env = dict(os.environ)
        env.pop("X2G_LIB", None)
        if name == "base":
            env["X2G_LIB"] = os.path.abspath(base)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True,
                             text=True, timeout=600)
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        if out.returncode != 0 or not line:
            sys.exit(f"leg 1 child ({name}) failed: {out.returncode}\n{out.stderr[-2000:]}")
        runs[name].append(json.loads(line[-1]))
    med = {k: float(np.median([min(r["ms"]) for r in v])) for k, v in runs.items()}
    base_ms = [min(r["ms"]) for r in runs["base"]]
    return {"leg1_base_ms_per_process": [r["ms"] for r in runs["base"]],
            "leg1_this_ms_per_process": [r["ms"] for r in runs["this"]],
            "leg1_base_ms": round(med["base"], 4), "leg1_this_p0_ms": round(med["this"], 4),
            "leg1_base_spread_ms": round(max(base_ms) - min(base_ms), 4),
            "leg1_this_minus_base_ms": round(med["this"] - med["base"], 4),
            "leg1_within_base_spread": bool(abs(med["this"] - med["base"]) <= max(base_ms) - min(base_ms)),
            "leg1_losses_equal": len({r["loss"] for v in runs.values() for r in v}) == 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    dev = torch.device("cuda:0")
    batch = collate(synthetic_molecules(BATCH, "S160", seed=3000)).to(dev)
    tr0, trp = trainer(dev, 0.0), trainer(dev, P_DROP)
    k0, kp = center_kernel_us(tr0, batch), center_kernel_us(trp, batch)
    tr0.capture(batch)
    trp.capture(batch)
    legs = {"p0": [], "p0_again": [], "p": []}
    fns = {"p0": lambda: tr0.step(batch), "p": lambda: trp.step(batch), "p0_again": lambda: tr0.step(batch)}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            legs[k].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in legs.items()}
    p0_all = legs["p0"] + legs["p0_again"]
    out = {"name": "dropout_step_time", "config": "config 2, S160, B = 128, captured steps", "steps": STEPS,
           "warmup": WARM, "rounds": ROUNDS, "p": P_DROP,
           "leg2_p0_ms_per_round": [round(v, 4) for v in legs["p0"]],
           "leg2_p0_again_ms_per_round": [round(v, 4) for v in legs["p0_again"]],
           "leg2_p_ms_per_round": [round(v, 4) for v in legs["p"]],
           "leg2_p0_ms": round(float(np.median(p0_all)), 4), "leg2_p_ms": round(med["p"], 4),
           "leg2_p0_spread_ms": round(max(p0_all) - min(p0_all), 4),
           "leg2_cost_ms_per_step": round(med["p"] - float(np.median(p0_all)), 4),
           "leg2_cost_percent": round(100 * (med["p"] / float(np.median(p0_all)) - 1), 2),
           "center_kernels_us_per_step_p0": k0, "center_kernels_us_per_step_p": kp,
           "center_kernels_cost_percent": {k: round(100 * (kp[k] / k0[k] - 1), 1) for k in k0 if k in kp},
           "dropout_step_counter": trp.model.fin_model.attn_dropout_state.tolist()}
    if args.base:
        out.update(leg1(args.base))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
