"""Fresh-batch training rate from a device-resident dataset (x2gnn.DeviceDataset) against the resident-batch
eager step and against the 4-worker DataLoader path, in one process, legs interleaved; one JSON line.

The set-up is bench.py's loader_probe: config 2 at S160, B = 128, 4 molecule groups (here repeated into a dataset of
2048 molecules), the same model and Trainer, 5 warm-up and 30 timed steps per leg, time.perf_counter around a
synchronised loop.  Each of ROUNDS rounds runs
  (a) the eager step on one resident batch,
  (b) the eager step on a fresh DeviceDataset.batch() per step (shuffled indices),
  (c) the eager step fed by a DataLoader of 4 workers (pinned, non-blocking H2D), as loader_probe does,
so (a)'s spread over its repetitions is known beside the result.  Also batch() alone at config 2 and at S5A: the
launch's GPU time (HIP events around x2g_batch_assemble), its algorithmic bytes (2 * E * F * 4 plus the small
outputs) as a fraction of 8 TB/s, the host time of the call and the synchronised wall time of a call.

    python scripts/device_loader_time.py"""
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
from x2gnn.data import collate  # noqa: E402
from x2gnn.synth import synthetic_molecules  # noqa: E402
from x2gnn.train import Trainer  # noqa: E402

CFG = dict(conv_layers=4, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)  # config.json
BATCH, GROUPS, REPEAT, WARM, STEPS, WORKERS, ROUNDS = 128, 4, 4, 5, 30, 4, 3
HBM_BYTES_PER_S = 8e12


class _LoaderBatches(torch.utils.data.Dataset):
    """Batch i = collate of molecule group i % len(groups) (made in a DataLoader worker)."""

    def __init__(self, groups, n):
        self.groups, self.n = groups, n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return collate(self.groups[i % len(self.groups)])


def timed_steps(tr, batches):
    """ms per step over STEPS steps after WARM warm-up steps; ``batches`` yields WARM + STEPS batches."""
    it = iter(batches)
    for _ in range(WARM):
        tr.step(next(it))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        tr.step(next(it))
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / STEPS


def batch_alone(ds, rng, n=30, warm=5):
    """x2g_batch_assemble's GPU time (events around the launch), the host time of batch() and its synchronised
    wall time, medians over ``n`` calls of BATCH shuffled molecules; and the algorithmic bytes of a call."""
    real_call = _lib.call
    events = []

    def call(name, *args):
        if name != "x2g_batch_assemble":
            return real_call(name, *args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real_call(name, *args)
        e1.record()
        events.append((e0, e1))

    _lib.call = call
    try:
        host, wall, nbytes = [], [], []
        for i in range(warm + n):
            idx = rng.choice(len(ds), size=BATCH, replace=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b = ds.batch(idx)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if i >= warm:
                host.append(t1 - t0)
                wall.append(t2 - t0)
                N, E, F = b.num_nodes, int(b.edge_index.shape[1]), ds.num_features
                small = sum(v.numel() * v.element_size() for k, v in b._store.items()
                            if torch.is_tensor(v) and k != "edge_attr")
                # edge_attr read and written; the small outputs written, and read once from the dataset
                nbytes.append(2 * E * F * 4 + 2 * small)
        gpu = [e0.elapsed_time(e1) * 1e-3 for e0, e1 in events[warm:]]
    finally:
        _lib.call = real_call
    g, by = float(np.median(gpu)), float(np.median(nbytes))
    return {"kernel_us": round(1e6 * g, 2), "kernel_us_min": round(1e6 * min(gpu), 2),
            "algorithmic_mbytes": round(by / 1e6, 3), "fraction_of_8TBps": round(by / g / HBM_BYTES_PER_S, 4),
            "host_call_us": round(1e6 * float(np.median(host)), 1),
            "synchronised_call_us": round(1e6 * float(np.median(wall)), 1)}


def main():
    from torch.utils.data import DataLoader

    dev = torch.device("cuda:0")
    groups = [synthetic_molecules(BATCH, "S160", seed=3000 + g) for g in range(GROUPS)]
    mols = [m for _ in range(REPEAT) for g in groups for m in g]
    ds = x2gnn.DeviceDataset(mols, dev)
    torch.manual_seed(0)
    tr = Trainer(x2gnn.xgnn_poly(device="cuda", **CFG).to(dev))
    resident = collate(groups[0]).to(dev)
    rng = np.random.default_rng(0)
    legs = {"resident": [], "device": [], "loader": []}
    for r in range(ROUNDS):
        legs["resident"].append(timed_steps(tr, (resident for _ in range(WARM + STEPS))))
        order = [rng.choice(len(ds), size=BATCH, replace=False) for _ in range(WARM + STEPS)]
        legs["device"].append(timed_steps(tr, (ds.batch(i) for i in order)))
        dl = DataLoader(_LoaderBatches(groups, WARM + STEPS), batch_size=None, num_workers=WORKERS, pin_memory=True,
                        prefetch_factor=4, persistent_workers=False)
        legs["loader"].append(timed_steps(tr, (b.to(dev, non_blocking=True) for b in dl)))
        del dl
    alone = batch_alone(ds, rng)
    s5a = x2gnn.DeviceDataset(synthetic_molecules(2 * BATCH, "S5A", seed=3100), dev)
    alone_s5a = batch_alone(s5a, rng)
    a, b, c = (float(np.median(legs[k])) for k in ("resident", "device", "loader"))
    spread = max(legs["resident"]) - min(legs["resident"])
    bar = a + alone["synchronised_call_us"] * 1e-3 + spread
    print(json.dumps({
        "name": "device_loader_time", "config": "config 2, S160, B = 128", "dataset_molecules": len(ds),
        "steps": STEPS, "warmup": WARM, "rounds": ROUNDS, "workers": WORKERS,
        "resident_ms_per_step": [round(v, 4) for v in legs["resident"]],
        "device_dataset_ms_per_step": [round(v, 4) for v in legs["device"]],
        "dataloader_ms_per_step": [round(v, 4) for v in legs["loader"]],
        "resident_ms": round(a, 4), "resident_spread_ms": round(spread, 4), "device_dataset_ms": round(b, 4),
        "dataloader_ms": round(c, 4), "device_dataset_molecules_per_s": round(BATCH / b * 1e3, 1),
        "dataloader_molecules_per_s": round(BATCH / c * 1e3, 1), "dataloader_over_device_dataset": round(c / b, 3),
        "fresh_bar_ms": round(bar, 4), "fresh_within_bar": bool(b <= bar),
        "batch_alone_s160": alone, "batch_alone_s5a": alone_s5a}))


if __name__ == "__main__":
    main()
