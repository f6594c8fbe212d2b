"""What SBFTransformerV2's per-layer atom context costs (csrc/atom_context.hip); one JSON line
(profiles/atom_context_time.json).

Leg 1 (kernels alone): config 2's shape (the resident batch's own row pointer: N = 2,304 atoms, E about 21k line
nodes, D = 128) through the raw ABI.  SETS operand sets are launched once each in one captured graph; HIP events
around REPLAYS replays give the time per launch of x2g_atom_context_fwd (with the four saved operands) and
x2g_atom_context_bwd (dx written).

Leg 2 (one process, captured steps of config 2: S160, B = 128): (a) xgnn_poly, (b) xgnn_poly_v2 with the fused
atom-context kernels, (c) xgnn_poly_v2 with ops._ATOM_CTX = False (segment_sum -> a three-stage row chain and their
adjoints).  Every round times STEPS replays of each after WARM warm-up replays, (b) twice per round so that its
own spread stands beside the differences.

    python scripts/atom_context_time.py"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x2-gnn_amd"))
import x2gnn  # noqa: E402
from x2gnn import _lib, ops  # noqa: E402
from x2gnn.data import collate  # noqa: E402
from x2gnn.synth import synthetic_molecules  # noqa: E402
from x2gnn.train import Trainer  # noqa: E402

CFG = dict(conv_layers=4, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)  # config.json
BATCH, WARM, STEPS, ROUNDS = 128, 10, 100, 5
D, SETS, REPLAYS = 128, 12, 20


def timed(fn, steps=STEPS):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def kernels_alone(dev, host_batch):
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    src = host_batch.edge_index[0].numpy()
    N, E = int(host_batch.x.shape[0]), int(src.shape[0])
    rowptr = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(src, minlength=N))]).astype(np.int32)).to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    w0, w1, we = (rn(D, D) / D ** 0.5 for _ in range(3))
    b0, b1 = 0.1 * rn(D), 0.1 * rn(D)
    sets = [dict(x=rn(E, D), d_tab=rn(N, D), dx=rn(E, D), **{k: rn(N, D) for k in ("tab", "A", "z0", "h", "g", "d_g",
                                                                                  "d_z0")}) for _ in range(SETS)]
    side = torch.cuda.Stream()

    def fwd(s, st):
        _lib.check(lib.x2g_atom_context_fwd(p(s["x"]), p(rowptr), N, E, D, p(w0), p(b0), p(w1), p(b1), p(we),
                                            p(s["tab"]), p(s["A"]), p(s["z0"]), p(s["h"]), p(s["g"]), st),
                   "x2g_atom_context_fwd")

    def bwd(s, st):
        _lib.check(lib.x2g_atom_context_bwd(p(s["d_tab"]), p(s["z0"]), p(rowptr), N, E, D, p(w0), p(w1), p(we),
                                            p(s["d_g"]), p(s["d_z0"]), p(s["dx"]), 0, st), "x2g_atom_context_bwd")

    out = {}
    for name, fn in (("fwd", fwd), ("bwd", bwd)):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            st = ctypes.c_void_p(side.cuda_stream)
            for s in sets:
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
    return {"shape": f"N = {N}, E = {E}, D = {D}; {SETS} operand sets per replay, {-(-N // 16)} workgroups",
            "fwd_us_per_launch": round(out["fwd"], 2), "bwd_us_per_launch": round(out["bwd"], 2)}


def trainer(dev, make):
    torch.manual_seed(0)
    return Trainer(make(device="cuda", **CFG).to(dev))


def step_legs(dev, host_batch):
    batch = host_batch.to(dev)
    tr_a = trainer(dev, x2gnn.xgnn_poly)
    tr_a.capture(batch)
    tr_b = trainer(dev, x2gnn.xgnn_poly_v2)
    tr_b.capture(batch)
    ops._ATOM_CTX = False  # (read while the step is captured: the graph keeps the composition's launches)
    try:
        tr_c = trainer(dev, x2gnn.xgnn_poly_v2)
        tr_c.capture(batch)
    finally:
        ops._ATOM_CTX = True
    fns = {"poly": lambda: tr_a.step(batch), "v2_fused": lambda: tr_b.step(batch),
           "v2_composed": lambda: tr_c.step(batch), "v2_fused_again": lambda: tr_b.step(batch)}
    legs = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            legs[k].append(timed(fn))
    fused = legs["v2_fused"] + legs["v2_fused_again"]
    med = {"poly": float(np.median(legs["poly"])), "v2_fused": float(np.median(fused)),
           "v2_composed": float(np.median(legs["v2_composed"]))}
    out = {"config": "config 2, S160, B = 128, captured steps", "steps": STEPS, "warmup": WARM, "rounds": ROUNDS}
    out.update({k + "_ms_per_round": [round(v, 4) for v in vs] for k, vs in legs.items()})
    out.update({k + "_ms": round(v, 4) for k, v in med.items()})
    out["v2_fused_spread_ms"] = round(max(fused) - min(fused), 4)
    out["v2_fused_over_poly"] = round(med["v2_fused"] / med["poly"], 4)
    out["v2_fused_over_v2_composed"] = round(med["v2_fused"] / med["v2_composed"], 4)
    out["fused_minus_composed_ms"] = round(med["v2_fused"] - med["v2_composed"], 4)
    out["fused_faster_beyond_spread"] = bool(med["v2_composed"] - med["v2_fused"] > out["v2_fused_spread_ms"])
    return out


def main():
    dev = torch.device("cuda:0")
    host_batch = collate(synthetic_molecules(BATCH, "S160", seed=3000))
    out = {"name": "atom_context_time", "kernels": kernels_alone(dev, host_batch), "step": step_legs(dev, host_batch)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
