"""What the multi-target model tests share (host and GPU): the reference-made fixture ``model_multi.npz`` seen one
model at a time, the oracle with K-wide readouts, and batches with K-wide labels."""
import numpy as np
import torch

from conftest import golden
from helpers import batch_from_fixture, model_cfg
from weights import load_seeded

MODELS = ("poly", "global", "global_add")


class FixtureView:
    """One model of model_multi.npz with the keys of a make_golden.py model fixture (``energies``, ``gnorm.<name>``,
    ``grad.<name>``, ``emb_after``, ...): the model's own keys are stored under ``<model>.``, the inputs once."""

    def __init__(self, z, model):
        self.z, self.prefix = z, model + "."
        own = [k[len(self.prefix):] for k in z.files if k.startswith(self.prefix)]
        shared = [k for k in z.files if not any(k.startswith(m + ".") for m in MODELS)]
        self.files = own + shared

    def __getitem__(self, key):
        return self.z[self.prefix + key] if self.prefix + key in self.z.files else self.z[key]


def fixture(model):
    return FixtureView(golden("model_multi.npz"), model)


def widen(module, K):
    """Replace each readout's last nn.Linear(c, 1) by nn.Linear(c, K) (the oracle's readouts are built one wide)."""
    for r in module.fin_model.readouts:
        last = r.mlp[-1]
        r.mlp[-1] = type(last)(last.in_features, K)
    return module


def oracle_k(kind, pool_option, K, seed, cfg):
    """oracle.ref_cpu.XGNN with K-wide readouts and seeded weights; its result is the [B, K] energies flattened."""
    from oracle.ref_cpu import XGNN

    m = widen(XGNN(global_pool=pool_option if kind == "global" else None, **cfg), K)
    load_seeded(m, seed)
    return m


def oracle_of(z):
    return oracle_k(str(z["kind"]), str(z["pool_option"]), int(z["num_target"]), int(z["weight_seed"]), model_cfg(z))


def batch_k(z, shipped=True):
    """The fixture's batch; ``y`` is its [B, K] labels."""
    b = batch_from_fixture(z, shipped=shipped)
    y = np.asarray(z["y"], np.float32)
    assert y.ndim == 2 and b._store["y"].shape == (y.shape[0], y.shape[1])
    return b


def small_batch(K, seed=9):
    """The three molecules of model_small.npz (its first three; the batch is rebuilt from them) with seeded [3, K]
    labels, as molecule dicts for ``collate`` / ``DeviceDataset``."""
    z = golden("model_small.npz")
    nodes, edges, trips = z["nodes"][:3], z["edges"][:3], z["triplets"][:3]
    a0 = np.concatenate([[0], np.cumsum(z["nodes"])])
    e0 = np.concatenate([[0], np.cumsum(z["edges"])])
    ys = np.random.default_rng(seed).standard_normal((3, K)).astype(np.float32)
    mols = []
    for i in range(3):
        ei = z["edge_index"][:, e0[i]:e0[i + 1]].astype(np.int64) - a0[i]
        mols.append({"x": z["x"][a0[i]:a0[i + 1]].astype(np.int64), "atom_pos": z["atom_pos"][a0[i]:a0[i + 1]],
                     "edge_index": ei, "edge_attr": z["edge_attr"][e0[i]:e0[i + 1]], "edge_num": int(edges[i]),
                     "triplet_num": int(trips[i]), "y": ys[i] if K > 1 else float(ys[i, 0])})
    assert [len(m["x"]) for m in mols] == list(nodes)
    return mols


def copy_shared(dst, src, skip=("mlp.4.",)):
    """Load every parameter of ``src`` whose name and shape ``dst`` has too (the trunk and the hidden readout layers);
    returns the names left alone."""
    sd, own = src.state_dict(), dst.state_dict()
    left = []
    with torch.no_grad():
        for k, v in own.items():
            if k in sd and sd[k].shape == v.shape and not any(s in k for s in skip):
                v.copy_(sd[k])
            else:
                left.append(k)
    return left
