"""What the edge features from AO matrices cost (csrc/ao_features.hip); writes one JSON line
(profiles/ao_features_time.json by default).

Workload: 128 synthetic molecules of the S160 generator (config 2's N and E: 18 atoms and about 150 directed edges
each), 39 AOs per heavy atom and 9 per hydrogen, seeded random symmetric float64 matrices: 432 x 432 per molecule,
about 380 MB for both matrices of all molecules, more than the 256 MiB the last-level cache holds.

Legs, interleaved over ROUNDS rounds after a warm-up, each timed with device events over REPS calls; medians with
their min and max:
  kernel     x2gnn.features.ao_edge_features, one launch for all molecules
  composed   the same features from torch index and norm ops on the GPU: a vectorised gather into [E, 2, 39, 39]
             float32 and group sums by two small matrix products, which is what a user would otherwise write.  It has
             no fixed summation order and no NaN rows for invalid edges.
  bytes      what the kernel has to move (every block read once as float64, every row written once as float32) over
             the kernel's time, beside the HBM rate measured for this chip (6.3 TB/s achievable, 8 TB/s spec).
The reference's host loop took 0.35 ms per edge on one CPU core (20 edges, pyscf stubbed); that figure is carried as
context, it is not measured here.

    python scripts/ao_features_time.py [--out PATH]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x2-gnn_amd"))
from x2gnn.features import AO_GROUPS, AO_PAD, AOMatrices, ao_edge_features  # noqa: E402
from x2gnn.synth import synthetic_molecules  # noqa: E402

MOLS, WARM, REPS, ROUNDS = 128, 5, 20, 7
HOST_LOOP_MS_PER_EDGE = 0.35
HBM_ACHIEVABLE_TBS, HBM_SPEC_TBS = 6.3, 8.0


def workload(seed=3000):
    mols = synthetic_molecules(MOLS, "S160", seed=seed)
    rng = np.random.default_rng(seed + 1)
    parts, eis, at = [], [], 0
    for m in mols:
        counts = np.where(np.asarray(m["x"]) == 1, 9, AO_PAD)
        ends = np.cumsum(counts)
        sl = np.stack([np.zeros_like(ends), np.zeros_like(ends), ends - counts, ends], axis=1).astype(np.int64)
        nao = int(ends[-1])

        def sym():
            A = rng.choice([-1.0, 1.0], size=(nao, nao)) * 10.0 ** rng.uniform(-6.0, 1.0, size=(nao, nao))
            return np.triu(A) + np.triu(A, 1).T

        parts.append((sym(), sym(), sl, int(np.asarray(m["x"]).sum())))
        eis.append(np.asarray(m["edge_index"], np.int64) + at)
        at += len(counts)
    return AOMatrices.from_molecules(parts), np.concatenate(eis, axis=1)


def composed(ao, ei, atom_mol, gmat):
    """[E, 338] from torch ops: gather the padded blocks, square, sum by groups, root; the 5 x 5 corner signed."""
    i, j = ei[0], ei[1]
    m = atom_mol[i].long()
    nao, start = ao.mol_nao[m].long(), ao.mat_start[m]
    bi, bj = ao.ao_begin[i].long(), ao.ao_begin[j].long()
    r, c = ao.ao_end[i].long() - bi, ao.ao_end[j].long() - bj
    r0 = torch.where((r == 9) & (c == 9), 2, 0)
    c0 = torch.where((c == 9) & ((r == AO_PAD) | (r == 9)), 2, 0)
    k = torch.arange(AO_PAD, device=ei.device)
    rr, cc = k[None, :] - r0[:, None], k[None, :] - c0[:, None]                 # block coordinates of each pad index
    rok, cok = (rr >= 0) & (rr < r[:, None]), (cc >= 0) & (cc < c[:, None])
    rows = (bi[:, None] + rr.clamp(min=0)).clamp(max=(nao - 1)[:, None])
    cols = (bj[:, None] + cc.clamp(min=0)).clamp(max=(nao - 1)[:, None])
    idx = start[:, None, None] + rows[:, :, None] * nao[:, None, None] + cols[:, None, :]
    ok = rok[:, :, None] & cok[:, None, :]
    S = torch.where(ok, ao.ovlp[idx], 0.0)
    H = torch.where(ok, ao.hcore[idx] / ao.hcore_div[m][:, None, None], 0.0)
    P = torch.stack([S, H], dim=1).to(torch.float32)                            # [E, 2, 39, 39]
    f = torch.sqrt(gmat.T @ (P * P) @ gmat)                                     # [E, 2, 13, 13]
    f[:, :, :5, :5] = P[:, :, :5, :5]
    return f.reshape(ei.shape[1], -1)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS  # ms per call


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ao_features_time.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ao_host, ei_host = workload()
    ao, ei = ao_host.to(dev), torch.from_numpy(ei_host).to(dev)
    atom_mol = ao.atom_mol()
    gmat = torch.zeros(AO_PAD, len(AO_GROUPS), device=dev)
    for g, (lo, hi) in enumerate(AO_GROUPS):
        gmat[lo:hi, g] = 1.0
    E, N = int(ei.shape[1]), ao.num_atoms
    width = (ao_host.ao_end - ao_host.ao_begin).numpy().astype(np.int64)
    read = int((width[ei_host[0]] * width[ei_host[1]]).sum()) * 8 * 2
    written = E * 338 * 4

    legs = {"kernel": lambda: ao_edge_features(ao, ei, atom_mol), "composed": lambda: composed(ao, ei, atom_mol, gmat)}
    got, alt = legs["kernel"](), legs["composed"]()
    nz = got != 0
    agree = float(((got - alt).abs()[nz] / got.abs()[nz]).max())
    zeros_agree = bool(((got == 0) == (alt == 0)).all())
    for fn in legs.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    kern = stats(ms["kernel"])
    out = {"name": "ao_features_time",
           "workload": f"{MOLS} S160 molecules: N = {N} atoms, E = {E} edges, {int(ao.ovlp.numel()) * 16 / 1e6:.0f} MB "
                       f"of float64 matrices",
           "reps_per_round": REPS, "rounds": ROUNDS, "warmup_calls": WARM,
           "kernel": kern, "composed": stats(ms["composed"]),
           "kernel_ms_per_round": [round(v, 4) for v in ms["kernel"]],
           "composed_ms_per_round": [round(v, 4) for v in ms["composed"]],
           "composed_over_kernel": round(float(np.median(ms["composed"]) / np.median(ms["kernel"])), 2),
           "composed_max_rel_diff_from_kernel": agree, "composed_zero_cells_agree": zeros_agree,
           "bytes": {"blocks_read": read, "rows_written": written,
                     "tb_per_s_at_kernel_median": round((read + written) / (kern["median_ms"] * 1e-3) / 1e12, 3),
                     "hbm_achievable_tb_per_s": HBM_ACHIEVABLE_TBS, "hbm_spec_tb_per_s": HBM_SPEC_TBS},
           "kernel_us_per_edge": round(1e3 * kern["median_ms"] / E, 5),
           "reference_host_loop_ms_per_edge_cpu_not_measured_here": HOST_LOOP_MS_PER_EDGE}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
