"""Generate ``model_v2.npz`` by running the REFERENCE's ``SBFTransformerV2`` (model.py:100-150; test infrastructure).

Run where the reference can be imported (``ref_import``), like make_golden.py:

    python tests/golden/make_v2_golden.py

The reference ships no featurisation for V2: its ``forward`` reads ``data.edge_attr`` as an atom index per triplet
(``atoms_rep[data.edge_attr]``, model.py:139).  The unmodified reference is driven through its own ``xgnn_poly``:
``fin_model`` is set to the reference's ``SBFTransformerV2`` and ``emb_block`` to a module that returns
``arange(N)``, so that ``atom_embeddings[atom_j]`` (xgnn.py:57-58) is ``atom_j``, the triplet's middle atom.  Seeded
weights (``weights.load_seeded``), three S160 synthetic molecules, and stored in make_golden.py's key scheme: the
inputs, the energies, the smooth-L1 loss against ``y``, every parameter gradient's norm, a few gradients element by
element, and the ``state_dict`` keys with their shapes.  Data only.
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

CFG = dict(conv_layers=2, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)
WEIGHT_SEED = 401
SEL = ["fin_model.edgenn.1.0.weight", "fin_model.edgenn.0.2.bias", "fin_model.convs.1.lin_edge.weight",
       "fin_model.convs.0.lin_sbf.bias", "fin_model.readouts.2.mlp.4.weight", "fin_model.dense_bf_skip.0.weight",
       "rbf_layer.frequencies"]


class AtomIndex(torch.nn.Module):
    """In ``emb_block``'s place: the atoms' own indices, so the per-triplet ``edge_attr`` is ``atom_j``."""

    def forward(self, x):
        return torch.arange(x.shape[0], device=x.device)


def build(ref):
    model = ref.xgnn.xgnn_poly(device="cpu", **CFG)
    model.fin_model = ref.model.SBFTransformerV2(
        conv_layers=CFG["conv_layers"], emb_size=CFG["embedding_size"], sbf_dim=CFG["sbf_dim"],
        rbf_dim=CFG["rbf_dim"], in_channels=CFG["in_channels"], heads=CFG["heads"])
    model.emb_block = AtomIndex()
    load_seeded(model, seed=WEIGHT_SEED)
    return model


def main():
    ref = import_reference()
    out = {}
    mols = synthetic_molecules(3, "S160", seed=61)
    b = pack_batch("", mols, out)
    out["cfg_keys"] = np.array(list(CFG.keys()))
    out["cfg_vals"] = np.array(list(CFG.values()))
    out["kind"] = np.array("poly_v2")
    out["weight_seed"] = np.int64(WEIGHT_SEED)
    model = build(ref)
    sd = model.state_dict()
    out["state_keys"] = np.array(list(sd.keys()))
    out["state_shapes"] = np.array([" ".join(str(int(d)) for d in v.shape) for v in sd.values()])
    res = model(b)
    assert tuple(res.shape) == (len(mols),)
    loss = torch.nn.functional.smooth_l1_loss(res, b.y)
    loss.backward()
    out["energies"] = res.detach().numpy()
    out["loss"] = np.float32(loss.item())
    for n, q in model.named_parameters():
        gr = q.grad
        out["gnorm." + n] = np.float64(0.0 if gr is None else gr.double().norm().item())
        if gr is not None and n in SEL:
            out["grad." + n] = gr.numpy()
    assert all("grad." + n in out for n in SEL)
    print(f"energies {res.detach().numpy().round(4)} loss {loss.item():.6f}")
    np.savez_compressed(os.path.join(HERE, "model_v2.npz"), **out)


if __name__ == "__main__":
    main()
