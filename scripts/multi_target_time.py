"""What K targets on one trunk cost a training step: config 3's shape (S160, B = 256, config.json widths), captured
Trainer steps on a resident batch, interleaved rounds; one JSON line (profiles/multi_target_time.json).

Legs 2 and 3 (always, one process): three trainers on resident batches of the same molecules, xgnn_poly (K = 1),
xgnn_poly(num_target=12) and xgnn_poly_multi(6, 6), each capturing its step; every round times STEPS replays of each
after WARM warm-up replays (time.perf_counter around a synchronised loop), K = 1 twice per round so that its own
spread stands beside the differences.

Per entry: HIP events around eager launches (a sleep kernel ahead of the start event), the median of REPS, of the
K-target head forward, pooled forward and backward at K = 12 against the K = 1 entries on the same rows (G = 5
readouts of [N, 128], N the batch's atom count), with the bytes each moves and the fraction of HBM_GBS they make.

Leg 1 (--base LIB: a libx2g.so built from the parent commit, scripts/build_base.sh): child processes of this script
(--child), X2G_LIB set to the base library or unset, each timing the K = 1 captured step; base, this tree, base,
this tree, base, so that the parent's process-to-process spread stands beside the difference.

    python scripts/multi_target_time.py [--base x2-gnn_amd/lib/ab/libx2g_base.so] [--legs 1,2,3,entries]"""
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
from x2gnn import _lib, ops  # noqa: E402
from x2gnn.data import collate  # noqa: E402
from x2gnn.synth import synthetic_molecules  # noqa: E402
from x2gnn.train import Trainer  # noqa: E402

CFG = dict(conv_layers=4, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)  # config.json
BATCH, WARM, STEPS, ROUNDS, REPS = 256, 10, 100, 5, 7
HBM_GBS = 8000.0  # MI355X peak HBM bandwidth, GB/s: the yardstick for "fraction of HBM"


def timed(fn, steps=STEPS):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def molecules(k):
    """Config 3's batch with k labels per molecule (seeded; the values do not change the work)."""
    mols = synthetic_molecules(BATCH, "S160", seed=3000)
    if k > 1:
        ys = np.random.default_rng(1).standard_normal((BATCH, k)).astype(np.float32)
        mols = [dict(m, y=ys[i]) for i, m in enumerate(mols)]
    return mols


def trainer(dev, kind):
    torch.manual_seed(0)
    if kind == "k1":
        m = x2gnn.xgnn_poly(device="cuda", **CFG)
    elif kind == "k12":
        m = x2gnn.xgnn_poly(device="cuda", num_target=12, **CFG)
    else:
        m = x2gnn.xgnn_poly_multi(device="cuda", atom_targets=6, mol_targets=6, **CFG)
    return Trainer(m.to(dev))


def child():
    dev = torch.device("cuda:0")
    batch = collate(molecules(1)).to(dev)
    tr = trainer(dev, "k1")
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
                             text=True, timeout=300)
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        if out.returncode != 0 or not line:
            sys.exit(f"leg 1 child ({name}) failed: {out.returncode}\n{out.stderr[-2000:]}")
        runs[name].append(json.loads(line[-1]))
    med = {k: float(np.median([min(r["ms"]) for r in v])) for k, v in runs.items()}
    base_ms = [min(r["ms"]) for r in runs["base"]]
    return {"leg1_base_ms_per_process": [r["ms"] for r in runs["base"]],
            "leg1_this_ms_per_process": [r["ms"] for r in runs["this"]],
            "leg1_base_ms": round(med["base"], 4), "leg1_this_k1_ms": round(med["this"], 4),
            "leg1_base_spread_ms": round(max(base_ms) - min(base_ms), 4),
            "leg1_this_minus_base_ms": round(med["this"] - med["base"], 4),
            "leg1_within_base_spread": bool(abs(med["this"] - med["base"]) <= max(base_ms) - min(base_ms)),
            "leg1_losses_equal": len({r["loss"] for v in runs.values() for r in v}) == 1}


def legs23(dev):
    b1, b12 = collate(molecules(1)).to(dev), collate(molecules(12)).to(dev)
    trs = {"k1": (trainer(dev, "k1"), b1), "k12": (trainer(dev, "k12"), b12), "multi": (trainer(dev, "multi"), b12)}
    for tr, b in trs.values():
        tr.capture(b)
    order = ("k1", "k12", "multi", "k1_again")
    legs = {k: [] for k in order}
    for _ in range(ROUNDS):
        for k in order:
            tr, b = trs[k[:-6] if k.endswith("_again") else k]
            legs[k].append(timed(lambda: tr.step(b)))
    k1_all = legs["k1"] + legs["k1_again"]
    k1 = float(np.median(k1_all))
    out = {"atoms": int(b1.x.shape[0]), "edges": int(b1.edge_index.shape[1])}
    for k in order:
        out[f"{k}_ms_per_round"] = [round(v, 4) for v in legs[k]]
    out.update(k1_ms=round(k1, 4), k1_spread_ms=round(max(k1_all) - min(k1_all), 4))
    for k, leg in (("k12", "leg2"), ("multi", "leg3")):
        ms = float(np.median(legs[k]))
        out.update({f"{leg}_{k}_ms": round(ms, 4), f"{leg}_minus_k1_ms": round(ms - k1, 4),
                    f"{leg}_ratio": round(ms / k1, 4)})
    return out


def event_us(fn):
    """Median over REPS of one launch sequence's HIP-event time, microseconds."""
    ts = []
    for i in range(REPS + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(200_000)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= 2:
            ts.append(1e3 * a.elapsed_time(b))
    return float(np.median(ts))


def entries(dev, rows, n_seg):
    """The K = 12 head entries against the K = 1 entries on the same rows: G = 5, D = 128."""
    G, D, K = 5, 128, 12
    lib = _lib.load()
    st = _lib.stream_ptr()
    f32 = dict(dtype=torch.float32, device=dev)
    h = [torch.randn(rows, D, **f32) for _ in range(G)]
    dh = [torch.empty(rows, D, **f32) for _ in range(G)]
    seg = torch.linspace(0, rows, n_seg + 1, device=dev).to(torch.int32).contiguous()
    seg[-1] = rows

    def ptrs(ts):
        return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    out = {}
    for k in (1, K):
        w = [torch.randn(k, D, **f32) / D ** 0.5 for _ in range(G)]
        b = [torch.randn(k, **f32) for _ in range(G)]
        dw, db = [torch.empty(k, D, **f32) for _ in range(G)], [torch.empty(k, **f32) for _ in range(G)]
        o_row, o_seg = torch.empty(rows, k, **f32), torch.empty(n_seg, k, **f32)
        d_row, d_seg = torch.randn(rows, k, **f32), torch.randn(n_seg, k, **f32)
        if k == 1:
            fwd_g = (ops.HeadGroup * G)(*[ops.HeadGroup(h[g].data_ptr(), w[g].data_ptr(), b[g].data_ptr(), None, None,
                                                        None) for g in range(G)])
            bwd_g = (ops.HeadGroup * G)(*[ops.HeadGroup(h[g].data_ptr(), w[g].data_ptr(), None, dh[g].data_ptr(),
                                                        dw[g].data_ptr(), db[g].data_ptr()) for g in range(G)])
            wsb = int(lib.x2g_readout_head_bwd_workspace(rows, D, G))
            ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
            calls = {
                "fwd": lambda: _lib.call("x2g_readout_head_fwd", fwd_g, G, rows, D, _lib.ptr(o_row), st),
                "pool_fwd": lambda: _lib.call("x2g_readout_head_pool_fwd", fwd_g, G, rows, D, _lib.ptr(seg), n_seg,
                                              _lib.ptr(o_seg), st),
                "pool_bwd": lambda: _lib.call("x2g_readout_head_pool_bwd", _lib.ptr(d_seg), _lib.ptr(seg), n_seg, bwd_g,
                                              G, rows, D, 0, _lib.ptr(ws), wsb, st)}
        else:
            wsb = int(lib.x2g_readout_heads_k_bwd_workspace(rows, D, k, G))
            ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
            hp, wp, bp, dhp, dwp, dbp = ptrs(h), ptrs(w), ptrs(b), ptrs(dh), ptrs(dw), ptrs(db)
            calls = {
                "fwd": lambda: _lib.call("x2g_readout_heads_k_fwd", hp, wp, bp, G, rows, D, k, None, 0,
                                         _lib.ptr(o_row), st),
                "pool_fwd": lambda: _lib.call("x2g_readout_heads_k_fwd", hp, wp, bp, G, rows, D, k, _lib.ptr(seg),
                                              n_seg, _lib.ptr(o_seg), st),
                "pool_bwd": lambda: _lib.call("x2g_readout_heads_k_bwd", _lib.ptr(d_seg), _lib.ptr(seg), n_seg, hp, wp,
                                              dhp, dwp, dbp, G, rows, D, k, 0, _lib.ptr(ws), wsb, st)}
        hbytes, wbytes = 4 * G * rows * D, 4 * G * k * (D + 1)
        moved = {"fwd": hbytes + wbytes + 4 * rows * k, "pool_fwd": hbytes + wbytes + 4 * n_seg * k + 4 * (n_seg + 1),
                 "pool_bwd": 2 * hbytes + 2 * wbytes + 4 * n_seg * k + 2 * wsb}  # h in, dh out; slabs out and in
        for name, fn in calls.items():
            us = event_us(fn)
            out[f"{name}_k{k}"] = {"us": round(us, 2), "bytes": int(moved[name]),
                                   "hbm_fraction": round(moved[name] / (us * 1e-6) / (HBM_GBS * 1e9), 4)}
        del calls
    for name in ("fwd", "pool_fwd", "pool_bwd"):
        out[f"{name}_k12_over_k1"] = round(out[f"{name}_k12"]["us"] / out[f"{name}_k1"]["us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--legs", default="1,2,3,entries")
    args = ap.parse_args()
    if args.child:
        return child()
    want = set(args.legs.split(","))
    dev = torch.device("cuda:0")
    out = {"name": "multi_target_time", "config": "config 3 shape: S160, B = 256, config.json widths, captured steps",
           "steps": STEPS, "warmup": WARM, "rounds": ROUNDS, "reps": REPS}
    if want & {"2", "3"}:
        out.update(legs23(dev))
    if "entries" in want:
        b = collate(molecules(1))
        out["entries"] = dict(entries(dev, int(b.x.shape[0]), BATCH), rows=int(b.x.shape[0]), segments=BATCH,
                              groups=5, dim=128, hbm_gbs=HBM_GBS)
    if args.base and "1" in want:
        out.update(leg1(args.base))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
