"""What building a dataset from geometries costs with the radius graph on the device (csrc/radius_graph.hip) and
without it; writes one JSON line (profiles/radius_graph_time.json by default).

Workload: 512 records of the S160 generator (18 atoms and about 150 directed edges each), 39 AOs per heavy atom and 9
per hydrogen, seeded random symmetric float64 matrices of 432 x 432 per molecule (1.5 GB for both matrices of all
molecules, on the host).

Legs, interleaved over ROUNDS rounds after a warm-up; medians with their min and max:
  a  round_trip     datasets.records_to_data + DeviceDataset(datas): the path before this kernel (bonds in a Python
                    loop on the CPU, every feature row to the host and back)                    wall clock with a sync
  b  from_records   DeviceDataset.from_records                                                   wall clock with a sync
  c  radius_graph   x2gnn.radius_graph alone on resident positions (two launches, one host read) wall clock with a sync
  d  host_graph     bonds(distance_matrix(R)) per record + device_dataset.molecule_stats         wall clock
  count, fill       the two entry points alone through the C ABI, device events over REPS calls, beside the bytes they
                    have to move (positions read once per launch, every output written once)
Legs a and b both upload the same matrices chunk by chunk; that copy is most of b.

    python scripts/radius_graph_time.py [--out PATH]"""
import argparse
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
from x2gnn import _lib  # noqa: E402
from x2gnn import datasets as ds  # noqa: E402
from x2gnn.device_dataset import molecule_stats  # noqa: E402
from x2gnn.features import AO_PAD, AOMatrices  # noqa: E402
from x2gnn.synth import SHAPES, random_geometry  # noqa: E402

MOLS, WARM, REPS, ROUNDS = 512, 2, 50, 5
CUTOFF = 5.0


def workload(seed=4000):
    geo, rng = np.random.default_rng(seed), np.random.default_rng(seed + 1)
    recs, parts = [], []
    for k in range(MOLS):
        z, pos = random_geometry(geo, SHAPES["S160"])
        recs.append(ds.MolRecord(atom="", R=torch.from_numpy(pos.astype(np.float32)), Z=torch.from_numpy(z),
                                 N=torch.tensor([len(z)]), Label=torch.tensor([float(rng.normal())]),
                                 idx=torch.tensor([k])))
        counts = np.where(z == 1, 9, AO_PAD)
        ends = np.cumsum(counts)
        sl = np.stack([np.zeros_like(ends), np.zeros_like(ends), ends - counts, ends], axis=1).astype(np.int64)
        nao = int(ends[-1])

        def sym():
            A = rng.choice([-1.0, 1.0], size=(nao, nao)) * 10.0 ** rng.uniform(-6.0, 1.0, size=(nao, nao))
            return np.triu(A) + np.triu(A, 1).T

        parts.append((sym(), sym(), sl, int(z.sum())))
    return recs, AOMatrices.from_molecules(parts)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS, None


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radius_graph_time.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    recs, ao = workload()
    start = np.concatenate([[0], np.cumsum([r.Z.shape[0] for r in recs])]).astype(np.int64)
    pos = torch.cat([r.R for r in recs]).to(dev)
    N, M = int(start[-1]), MOLS

    def host_graph():
        eis = [ds.bonds(ds.distance_matrix(r.R), CUTOFF).numpy() for r in recs]
        edges = np.array([e.shape[1] for e in eis], np.int64)
        return eis, edges, molecule_stats(np.diff(start), edges, np.concatenate(eis, axis=1))

    # the two entry points alone, on buffers made once
    g = x2gnn.radius_graph(pos, start, CUTOFF, global_ids=True)
    E = g.num_edges
    lib, p = _lib.load(), _lib.ptr
    start_d = torch.from_numpy(start).to(dev)
    degree, row_start = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N + 1, dtype=torch.int64, device=dev)
    per_mol = [torch.empty(M, dtype=torch.int64, device=dev) for _ in range(3)]
    last = torch.empty(M, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.x2g_radius_graph_count_workspace(N)), 8), dtype=torch.uint8, device=dev)
    local, glob = (torch.empty((2, E), dtype=torch.int64, device=dev) for _ in range(2))
    i64, f32, st = ctypes.c_int64, ctypes.c_float, _lib.stream_ptr(dev)

    def count():
        _lib.call("x2g_radius_graph_count", p(pos), p(start_d), i64(N), i64(M), f32(CUTOFF), p(degree), p(row_start),
                  p(per_mol[0]), p(per_mol[1]), p(per_mol[2]), p(last), p(ws), ctypes.c_size_t(ws.numel()), st)

    def fill():
        _lib.call("x2g_radius_graph_fill", p(pos), p(start_d), p(row_start), i64(N), i64(M), f32(CUTOFF), i64(E),
                  p(local), p(glob), st)

    count()
    fill()
    same = bool(torch.equal(local, g.edge_index) and torch.equal(glob, g.edge_index_global))

    legs = {
        "round_trip": (wall, lambda: x2gnn.DeviceDataset(ds.records_to_data(recs, ao, dev, CUTOFF), dev)),
        "from_records": (wall, lambda: x2gnn.DeviceDataset.from_records(recs, ao, dev, CUTOFF)),
        "radius_graph": (wall, lambda: x2gnn.radius_graph(pos, start, CUTOFF)),
        "host_graph": (wall, host_graph),
        "count": (events, count),
        "fill": (events, fill),
    }
    for k, (how, fn) in legs.items():
        for _ in range(WARM):
            out = how(fn)[1]
        if k == "round_trip":
            old = out
        elif k == "from_records":
            new = out
    equal = all(torch.equal(getattr(new, k), getattr(old, k)) for k in ("x", "atom_pos", "edge_index", "edge_attr", "y"))
    equal = equal and all(np.array_equal(getattr(new, k), getattr(old, k))
                          for k in ("nodes", "edges", "triplets", "max_degree", "symmetric"))
    del old, new, out
    ms = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, (how, fn) in legs.items():
            ms[k].append(how(fn)[0])
    med = {k: float(np.median(v)) for k, v in ms.items()}
    count_bytes = 12 * N + 8 * (M + 1) + 4 * N + 8 * (N + 1) + 28 * M
    fill_bytes = 12 * N + 8 * (M + 1) + 8 * N + 32 * E
    out = {"name": "radius_graph_time",
           "workload": f"{MOLS} S160 records: N = {N} atoms, E = {E} edges, {int(ao.ovlp.numel()) * 16 / 1e6:.0f} MB of "
                       f"float64 matrices on the host, {E * 338 * 4 / 1e6:.0f} MB of edge_attr",
           "rounds": ROUNDS, "warmup_calls": WARM, "reps_per_round_kernel_legs": REPS,
           "a_round_trip": stats(ms["round_trip"]), "b_from_records": stats(ms["from_records"]),
           "c_radius_graph": stats(ms["radius_graph"]), "d_host_graph": stats(ms["host_graph"]),
           "count": stats(ms["count"]), "fill": stats(ms["fill"]),
           "a_over_b": round(med["round_trip"] / med["from_records"], 2),
           "d_over_c": round(med["host_graph"] / med["radius_graph"], 1),
           "ms_per_round": {k: [round(v, 4) for v in vs] for k, vs in ms.items()},
           "bytes": {"count_min": count_bytes, "fill_min_with_global_ids": fill_bytes,
                     "count_gb_per_s_at_median": round(count_bytes / (med["count"] * 1e-3) / 1e9, 2),
                     "fill_gb_per_s_at_median": round(fill_bytes / (med["fill"] * 1e-3) / 1e9, 2)},
           "pairs_evaluated_per_launch": int((np.diff(start) ** 2).sum()),
           "raw_calls_equal_radius_graph": same, "from_records_equals_round_trip": bool(equal)}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
