"""What the conv combine pass (csrc/conv_combine.hip: SBFTransformerConv's beta=True / concat=False) costs; one JSON
line (profiles/conv_combine_time.json).

Leg 1 (kernels alone): config 2's shape (E = 21,058 line nodes, H*C = 128, gated, concat) through the raw ABI.
SETS operand sets (together larger than the 256 MB last-level cache, so a replay streams from HBM as the step
does) are launched once each in one captured graph; HIP events around REPLAYS replays give the time per launch,
forward and backward (the backward launch includes its slab sum).  The HBM fraction is measured against the
arithmetic byte counts: forward 3 rows of 512 B + 12 B per line node, backward 5 rows + 4 B.

Leg 2 (one process): two trainers on the same seed, conv_beta False and True, each capturing config 2's step
(S160, B = 128); every round times STEPS replays of each after WARM warm-up replays, the conv_beta=False trainer
twice per round so that its own spread stands beside the difference.

Leg 3 (--parent DIR: a checkout of the parent commit with its library built): ``python bench.py --gpus 1`` of DIR
and of this tree as child processes, alternating parent, this, parent, this, parent; the parent's spread against
itself stands beside the difference.  The default model makes the same launches in both.

    python scripts/conv_combine_time.py [--parent DIR]"""
import argparse
import ctypes
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
from x2gnn import _lib  # noqa: E402
from x2gnn.data import collate  # noqa: E402
from x2gnn.synth import synthetic_molecules  # noqa: E402
from x2gnn.train import Trainer  # noqa: E402

CFG = dict(conv_layers=4, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)  # config.json
BATCH, WARM, STEPS, ROUNDS = 128, 10, 100, 5
E, H, C, SETS, REPLAYS = 21058, 16, 8, 12, 20
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak
BENCH_STEPS, BENCH_WARM = 200, 5


def timed(fn, steps=STEPS):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def kernels_alone(dev):
    lib, D = _lib.load(), H * C
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    w = rn(3 * D) / (3 * D) ** 0.5
    sets = [dict(attn=rn(E, D), x=rn(E, D), dy=rn(E, D), y=rn(E, D), beta=rn(E), stats=rn(E, 2), da=rn(E, D),
                 dx=rn(E, D)) for _ in range(SETS)]
    dw = torch.zeros(3 * D, device=dev)
    ws_bytes = int(lib.x2g_conv_combine_bwd_workspace(E, H, C, 1))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream()

    def fwd(s, st):
        _lib.check(lib.x2g_conv_combine_fwd(p(s["attn"]), p(s["x"]), p(w), E, H, C, 1, p(s["y"]), p(s["beta"]),
                                            p(s["stats"]), st), "x2g_conv_combine_fwd")

    def bwd(s, st):
        _lib.check(lib.x2g_conv_combine_bwd(p(s["dy"]), p(s["attn"]), p(s["x"]), p(w), p(s["beta"]), E, H, C, 1,
                                            p(s["da"]), p(s["dx"]), p(dw), 0, None, p(ws), ws_bytes, st),
                   "x2g_conv_combine_bwd")

    out = {}
    for name, fn in (("fwd", fwd), ("bwd", bwd)):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            st = ctypes.c_void_p(side.cuda_stream)
            for s in sets:  # (beta in [0, 1] for the backward: the forward's)
                fwd(s, st)
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                for s in sets:
                    fn(s, st)
            for _ in range(3):
                graph.replay()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(side)
            for _ in range(REPLAYS):
                graph.replay()
            b.record(side)
            side.synchronize()
        out[name] = 1e3 * a.elapsed_time(b) / (REPLAYS * SETS)
    fwd_bytes, bwd_bytes = E * (3 * 4 * D + 12), E * (5 * 4 * D + 4)
    return {"shape": f"E = {E}, H*C = {D}, gated, concat; {SETS} operand sets per replay",
            "fwd_us_per_launch": round(out["fwd"], 2), "bwd_us_per_launch_with_slab_sum": round(out["bwd"], 2),
            "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes,
            "fwd_hbm_fraction": round(fwd_bytes / (out["fwd"] * 1e-6) / (HBM_PEAK_GBS * 1e9), 3),
            "bwd_hbm_fraction": round(bwd_bytes / (out["bwd"] * 1e-6) / (HBM_PEAK_GBS * 1e9), 3)}


def trainer(dev, beta):
    torch.manual_seed(0)
    return Trainer(x2gnn.xgnn_poly(device="cuda", conv_beta=beta, **CFG).to(dev))


def step_ab(dev):
    batch = collate(synthetic_molecules(BATCH, "S160", seed=3000)).to(dev)
    tr0, tr1 = trainer(dev, False), trainer(dev, True)
    tr0.capture(batch)
    tr1.capture(batch)
    legs = {"off": [], "off_again": [], "on": []}
    fns = {"off": lambda: tr0.step(batch), "on": lambda: tr1.step(batch), "off_again": lambda: tr0.step(batch)}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            legs[k].append(timed(fn))
    off = legs["off"] + legs["off_again"]
    med_off, med_on = float(np.median(off)), float(np.median(legs["on"]))
    return {"config": "config 2, S160, B = 128, captured steps", "steps": STEPS, "warmup": WARM, "rounds": ROUNDS,
            "beta_off_ms_per_round": [round(v, 4) for v in legs["off"]],
            "beta_off_again_ms_per_round": [round(v, 4) for v in legs["off_again"]],
            "beta_on_ms_per_round": [round(v, 4) for v in legs["on"]],
            "beta_off_ms": round(med_off, 4), "beta_on_ms": round(med_on, 4),
            "beta_off_spread_ms": round(max(off) - min(off), 4),
            "cost_ms_per_step": round(med_on - med_off, 4), "cost_percent": round(100 * (med_on / med_off - 1), 2)}


def bench_ab(parent):
    runs = {"parent": [], "this": []}
    for name in ("parent", "this", "parent", "this", "parent"):
        root = os.path.abspath(parent) if name == "parent" else ROOT
        env = dict(os.environ)
        env.pop("X2G_LIB", None)
        env.pop("X2G_HEADER", None)
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps",
                              str(BENCH_STEPS), "--warmup", str(BENCH_WARM)], env=env, cwd=root, capture_output=True,
                             text=True, timeout=600)
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        if out.returncode != 0 or not line:
            sys.exit(f"bench.py ({name}) failed: {out.returncode}\n{out.stderr[-2000:]}")
        runs[name].append(json.loads(line[-1]))
        print(f"bench.py ({name}): {line[-1][:120]}", file=sys.stderr, flush=True)
    key = next(k for k in ("value", "molecules_per_s", "metric_value") if k in runs["this"][0])
    vals = {k: [float(r[key]) for r in v] for k, v in runs.items()}
    med = {k: float(np.median(v)) for k, v in vals.items()}
    spread = max(vals["parent"]) - min(vals["parent"])
    return {"bench_metric": key, "bench_parent": vals["parent"], "bench_this": vals["this"],
            "bench_parent_median": round(med["parent"], 2), "bench_this_median": round(med["this"], 2),
            "bench_parent_spread": round(spread, 2), "bench_this_minus_parent": round(med["this"] - med["parent"], 2),
            "bench_within_parent_spread": bool(abs(med["this"] - med["parent"]) <= spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"name": "conv_combine_time", "kernels": kernels_alone(dev), "step": step_ab(dev)}
    if args.parent:
        torch.cuda.empty_cache()
        out["bench"] = bench_ab(args.parent)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
