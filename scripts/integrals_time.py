"""What the one-electron integrals cost on the device (csrc/integrals.hip) and what a dataset built from a basis set
costs against one built from matrices made elsewhere; writes one JSON line (profiles/integrals_time.json by default).

Workload: the 512 S160 records of scripts/radius_graph_time.py (18 atoms and about 150 directed edges each), with
their geometry written into each record's text, in a synthetic basis of the reference's 39 / 9 shape (BASIS below: a
heavy atom 5 s / 4 p / 3 d / 1 f with 6- and 3-primitive contractions, hydrogen 3 s / 2 p; made-up numbers, the ones
the tests use).

Legs, interleaved over ROUNDS rounds after a warm-up; medians with their min and max:
  kernel_bonds   x2g_one_electron_blocks alone on the unique unordered bond pairs, heaviest first   device events
  kernel_all     the same on every unordered atom pair, the diagonal included                        device events
  from_basis     DeviceDataset.from_records(records, basis): bonds, integrals and features on the
                 device, positions, Z and labels uploaded                                          wall clock with a sync
  from_matrices  DeviceDataset.from_records(records, AOMatrices): the complete float64 matrices (here
                 the all-pairs run's, copied to the host beforehand) uploaded chunk by chunk          wall clock with a sync
No CPU integral code is at hand here: a comparison with pyscf is not measured.

    python scripts/integrals_time.py [--out PATH]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "x2-gnn_amd"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, _p)
import x2gnn  # noqa: E402
from radius_graph_time import CUTOFF, MOLS, stats, wall  # noqa: E402
from x2gnn import datasets as ds  # noqa: E402
from x2gnn import integrals  # noqa: E402
from x2gnn.features import AOMatrices  # noqa: E402
from x2gnn.synth import SHAPES, random_geometry  # noqa: E402

WARM, REPS, ROUNDS = 1, 3, 5
SYMBOL = {1: "H", 6: "C", 7: "N", 8: "O", 9: "F"}


def _heavy(s):
    """5 s / 4 p / 3 d / 1 f = 39 functions, every exponent scaled by ``s`` (pyscf's format)."""
    return [[0, [4200.0 * s, 0.002], [630.0 * s, 0.015], [145.0 * s, 0.075], [41.0 * s, 0.26], [12.5 * s, 0.6],
             [1.9 * s, 0.24]],
            [0, [21.0 * s, 0.12], [4.9 * s, 0.9], [1.5 * s, -0.05]],
            [0, [0.48 * s, 1.0]], [0, [0.15 * s, 1.0]], [0, [0.045 * s, 1.0]],
            [1, [21.0 * s, 0.03], [4.9 * s, 0.15], [1.5 * s, 0.45]],
            [1, [0.48 * s, 1.0]], [1, [0.15 * s, 1.0]], [1, [0.045 * s, 1.0]],
            [2, [2.5 * s, 1.0]], [2, [0.63 * s, 1.0]], [2, [0.16 * s, 1.0]], [3, [0.8 * s, 1.0]]]


BASIS = {"C": _heavy(1.0), "N": _heavy(1.3), "O": _heavy(1.7), "F": _heavy(2.1),
         "H": [[0, [33.9, 0.025], [5.1, 0.19], [1.16, 0.85]], [0, [0.33, 1.0]], [0, [0.10, 1.0]], [1, [1.5, 1.0]],
               [1, [0.375, 1.0]]]}


def workload(seed=4000):
    geo, rng = np.random.default_rng(seed), np.random.default_rng(seed + 1)
    recs = []
    for k in range(MOLS):
        z, pos = random_geometry(geo, SHAPES["S160"])
        pos = np.asarray(pos, np.float64)
        text = f"{len(z)}\n{float(rng.normal())!r}\n" + "".join(
            f"{SYMBOL[int(a)]} {x!r} {y!r} {w!r}\n" for a, (x, y, w) in zip(z, pos.tolist()))
        recs.append(ds.MolRecord(atom=text, R=torch.from_numpy(pos.astype(np.float32)), Z=torch.from_numpy(z),
                                 N=torch.tensor([len(z)]), Label=torch.tensor([float(k)]), idx=torch.tensor([k])))
    return recs


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "integrals_time.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    basis = x2gnn.Basis.from_pyscf(BASIS)
    recs = workload()
    pos64, start = integrals.record_geometries(recs)
    Z = np.concatenate([r.Z.numpy() for r in recs])
    pos_d = torch.from_numpy(pos64).to(dev)
    g = x2gnn.radius_graph(pos_d.to(torch.float32), start, CUTOFF, global_ids=True)

    bonds = integrals.plan_one_electron(pos_d, Z, start, basis, pairs=g.edge_index_global)
    every = integrals.plan_one_electron(pos_d, Z, start, basis)
    pairs_b, pairs_a = bonds.num_pairs, every.num_pairs
    full = every.run()
    torch.cuda.synchronize()
    host = AOMatrices(*(getattr(full, k) if k == "atom_start" else getattr(full, k).cpu()
                        for k in ("ovlp", "hcore", "mat_start", "mol_nao", "hcore_div", "ao_begin", "ao_end",
                                  "atom_start")))

    legs = {
        "kernel_bonds": (events, bonds.run),
        "kernel_all": (events, every.run),
        "from_basis": (wall, lambda: x2gnn.DeviceDataset.from_records(recs, basis, dev, CUTOFF)),
        "from_matrices": (wall, lambda: x2gnn.DeviceDataset.from_records(recs, host, dev, CUTOFF)),
    }
    outs = {}
    for k, (how, fn) in legs.items():
        for _ in range(WARM):
            outs[k] = how(fn)[1]
    equal = bool(torch.equal(outs["from_basis"].edge_attr, outs["from_matrices"].edge_attr))
    E = int(outs["from_basis"].edge_attr.shape[0])
    outs.clear()
    ms = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, (how, fn) in legs.items():
            ms[k].append(how(fn)[0])
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"name": "integrals_time",
           "workload": f"{MOLS} S160 records: N = {int(start[-1])} atoms, E = {E} edges, synthetic 39 / 9 basis, "
                       f"{int(full.ovlp.numel()) * 16 / 1e6:.0f} MB of complete float64 matrices",
           "rounds": ROUNDS, "warmup_calls": WARM, "reps_per_round_kernel_legs": REPS,
           "pairs": {"bonds": pairs_b, "all": pairs_a},
           "kernel_bonds": stats(ms["kernel_bonds"]), "kernel_all": stats(ms["kernel_all"]),
           "from_basis": stats(ms["from_basis"]), "from_matrices": stats(ms["from_matrices"]),
           "us_per_pair": {"bonds": round(med["kernel_bonds"] * 1e3 / pairs_b, 3),
                           "all": round(med["kernel_all"] * 1e3 / pairs_a, 3)},
           "from_matrices_over_from_basis": round(med["from_matrices"] / med["from_basis"], 3),
           "ms_per_round": {k: [round(v, 4) for v in vs] for k, vs in ms.items()},
           "edge_attr_equal": equal, "pyscf_comparison": "not measured"}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
