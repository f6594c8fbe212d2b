"""Generate ``model_multi.npz`` by running the REFERENCE with K-wide readouts (test infrastructure).

Run where the reference can be imported (``ref_import``), like make_golden.py:

    python tests/golden/make_multi_golden.py

The reference's trunks construct their readouts with ``num_target=1`` (model.py:19,64), but its readout classes take
the width (readout.py:12,46).  This builds the reference's ``xgnn_poly`` and ``xgnn_poly_global`` (mean and add
pool), replaces ``fin_model.readouts`` with the reference's own ``AtomWise(num_target=3)`` / ``MolWise(num_target=3)``,
loads seeded weights (``weights.load_seeded``) and stores, in make_golden.py's key scheme under one prefix per model
(``poly.``, ``global.``, ``global_add.``): the flattened energies ``[B * 3]`` (the reference's ``.view(-1)`` of the
K-wide result, row-major), the smooth-L1 loss against ``y`` ``[B, 3]`` flattened likewise, every parameter gradient's
norm and a few gradients element by element.  The inputs (three small molecules) are stored once.  Data only.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "x2-gnn_amd"))
sys.path.insert(0, HERE)

from make_golden import pack_batch  # noqa: E402
from ref_import import import_reference  # noqa: E402
from weights import load_seeded  # noqa: E402
from x2gnn.synth import synthetic_molecules  # noqa: E402

torch.set_num_threads(8)

K = 3
CFG = dict(conv_layers=2, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)
MODELS = {"poly": ("poly", "mean", 301), "global": ("global", "mean", 302), "global_add": ("global", "add", 303)}
SEL = ["fin_model.readouts.0.mlp.4.weight", "fin_model.readouts.2.mlp.4.weight", "fin_model.readouts.2.mlp.4.bias",
       "fin_model.readouts.1.lin_rbf.weight", "fin_model.convs.1.lin_sbf.bias", "emb_block.embedding.weight",
       "rbf_layer.frequencies"]


def build(ref, kind, pool_option, seed_w):
    c, r = CFG["in_channels"], CFG["rbf_dim"]
    if kind == "poly":
        model = ref.xgnn.xgnn_poly(device="cpu", **CFG)
        make = lambda: ref.readout.AtomWise(in_channels=c, rbf_dim=r, num_target=K)  # noqa: E731
    else:
        model = ref.xgnn.xgnn_poly_global(device="cpu", pool_option=pool_option, **CFG)
        make = lambda: ref.readout.MolWise(in_channels=c, rbf_dim=r, num_target=K,  # noqa: E731
                                           pool_option=pool_option)
    model.fin_model.readouts = torch.nn.ModuleList([make() for _ in range(CFG["conv_layers"] + 1)])
    load_seeded(model, seed=seed_w)
    return model


def main():
    ref = import_reference()
    out = {}
    mols = synthetic_molecules(3, "S160", seed=51)
    b = pack_batch("", mols, out)
    y = np.random.default_rng(52).standard_normal((len(mols), K)).astype(np.float32)
    out["y"] = y
    out["cfg_keys"] = np.array(list(CFG.keys()))
    out["cfg_vals"] = np.array(list(CFG.values()))
    out["num_target"] = np.int64(K)
    out["models"] = np.array(list(MODELS))
    for name, (kind, pool_option, seed_w) in MODELS.items():
        model = build(ref, kind, pool_option, seed_w)
        res = model(b)
        assert tuple(res.shape) == (len(mols) * K,)
        loss = torch.nn.functional.smooth_l1_loss(res, torch.from_numpy(y).view(-1))
        loss.backward()
        p = name + "."
        out[p + "energies"] = res.detach().numpy()
        out[p + "loss"] = np.float32(loss.item())
        out[p + "weight_seed"] = np.int64(seed_w)
        out[p + "kind"] = np.array(kind)
        out[p + "pool_option"] = np.array(pool_option)
        out[p + "emb_after"] = model.emb_block.embedding.weight.detach().numpy().copy()
        for n, q in model.named_parameters():
            gr = q.grad
            out[p + "gnorm." + n] = np.float64(0.0 if gr is None else gr.double().norm().item())
            if gr is not None and n in SEL:
                out[p + "grad." + n] = gr.numpy()
        print(f"{name}: energies {res.detach().numpy().round(4)} loss {loss.item():.6f}")
    np.savez_compressed(os.path.join(HERE, "model_multi.npz"), **out)


if __name__ == "__main__":
    main()
