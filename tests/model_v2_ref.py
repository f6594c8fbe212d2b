"""xgnn_poly_v2 stated on the CPU with the oracle's modules (oracle/ref_cpu.py): the reference's SBFTransformerV2
(model.py:100-150) behind xgnn_poly's featurisation with the triplet's middle atom as ``edge_attr`` (what
tests/golden/make_v2_golden.py makes the reference compute).  Literal: the pooled atom rows are gathered per triplet
and edgenn / lin_edge run on T rows.  Parameter names are x2gnn.xgnn_poly_v2's, so ``weights.load_seeded`` fills
both alike; ``.double()`` makes it the float64 statement."""
import torch
import torch.nn as nn

from oracle import ref_cpu


class TrunkV2(ref_cpu.Trunk):
    def __init__(self, L, sbf_dim, rbf_dim, c, heads):
        super().__init__(L, c, sbf_dim, rbf_dim, c, heads)
        self.edgenn = nn.ModuleList([nn.Sequential(nn.Linear(c, c), nn.SiLU(), nn.Linear(c, c)) for _ in range(L)])

    def forward(self, x, edge_index, edge_attr, batch, sbf, rbf, ei0, atom_batch):
        n_atoms = atom_batch.shape[0]
        sbf = sbf.to(x.dtype)  # (the oracle's basis: formed in float64, handed over as float32)
        out = x
        results = self.readouts[0](out, rbf, n_atoms, ei0)
        for i, conv in enumerate(self.convs):
            res0 = out
            atoms_rep = ref_cpu.scatter_sum(out, ei0, n_atoms)                  # model.py:138
            e = self.edgenn[i](atoms_rep[edge_attr])                            # :139-140
            out = conv(sbf, rbf, out, edge_index, e)
            out = ref_cpu.graph_layer_norm(out, batch, 1e-8)
            out = self.bf_skip[i](out)
            out = self.AF(self.dense_bf_skip[i](out))
            out = out + res0
            out = self.af_skip[i](out)
            results = results + self.readouts[i + 1](out, rbf, n_atoms, ei0)
        b = int(batch.max()) + 1
        return ref_cpu.scatter_sum(results, atom_batch, b).view(-1) / len(self.convs)   # :149-150


class _AtomIndex(nn.Module):
    def forward(self, z):
        return torch.arange(z.shape[0])


class XGNNV2(ref_cpu.XGNN):
    def __init__(self, conv_layers=4, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128):
        super().__init__(conv_layers, sbf_dim, rbf_dim, in_channels, heads, embedding_size)
        self.emb_block = _AtomIndex()  # atom_embeddings[atom_j] (xgnn.py:57-58) is then atom_j
        self.fin_model = TrunkV2(conv_layers, sbf_dim, rbf_dim, in_channels, heads)


def statement(cfg, seed, batch, dtype=torch.float64):
    """(model, energies) of a host batch with ``load_seeded`` weights; the inputs widened to ``dtype``."""
    from weights import load_seeded

    m = XGNNV2(**cfg)
    load_seeded(m, seed)
    m = m.to(dtype)
    e = m(batch.x, batch.edge_index, batch.edge_attr.to(dtype), batch.atom_pos.to(dtype), batch.edge_num, batch.batch)
    return m, e
