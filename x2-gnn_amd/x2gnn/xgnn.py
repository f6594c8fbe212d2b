"""X2-GNN models (reference xgnn.py:15-137): ``xgnn_poly`` (extensive targets, per-atom
readout) and ``xgnn_poly_global`` (intensive targets, per-molecule readout).

``forward(data)`` takes a collated atom batch (``x`` = atomic numbers, ``edge_index`` sorted by
(src, dst), ``edge_attr`` [E,338], ``atom_pos``, ``edge_num``, ``batch``) and returns one energy
per molecule, like the reference.  What changes is where the work runs:

* the triplet builder runs on the GPU (``ops.vertex_to_edge``) instead of scipy on the host
  (xgnn.py:52-53), with its size taken from host metadata — no device->host traffic;
* angles and the 42-wide spherical basis are computed in one kernel straight from positions;
* the atom-embedding / ``edgenn`` / ``lin_edge`` chain runs on the 10-row element table instead
  of T per-triplet copies (exact: every triplet into line node e=(a->b) carries the embedding
  of atom b, xgnn.py:57-58), and the attention kernels read row Z[b] per destination;
* the trunk gets a prebuilt :class:`GraphPlan` instead of rediscovering sizes with host syncs.
"""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.nn import SiLU

from . import ops
from .data import Data
from .layers import EmbeddingBlock, F_B_2D, Linear, RadialBasis, poly_envelop
from .model import SBFTransformer, SBFTransformerGlobal, SBFTransformerMulti, SBFTransformerV2
from .plan import GraphPlan


class _XGNNBase(nn.Module):
    def _build(self, trunk, sbf_dim, rbf_dim, in_channels, embedding_size, device):
        self.device = device
        self.num_target = trunk.num_target  # the width of forward's result ([B] when 1, the multi model apart)
        self.cutoff = 5.0  # xgnn.py:30-33 (envelope, sbf and rbf layers all use 5.0)
        self.AF = SiLU()
        self.emb_block = EmbeddingBlock(embedding_size=embedding_size)
        self.envelop_function = poly_envelop(cutoff=5.0, exponent=5)
        self.sbf_layer = F_B_2D(sbf_dim, rbf_dim, 5.0, 5)
        self.rbf_layer = RadialBasis(cutoff=5.0, embedding_size=rbf_dim)
        self.fin_model = trunk
        self.mat_trans = Linear(338, 2 * embedding_size)
        self.rbf_trans = Linear(rbf_dim, embedding_size)  # unused by the reference forward too
        self.emb_trans = Linear(embedding_size * 2, in_channels)

    def _fused_basis(self):
        env, rbf = self.envelop_function, self.rbf_layer
        return (env.exponent == 5 and abs(env.inv_cutoff * self.cutoff - 1.0) < 1e-12
                and isinstance(getattr(rbf, "frequencies", None), torch.Tensor) and rbf.frequencies.numel() <= 16
                and abs(rbf.inv_cutoff * self.cutoff - 1.0) < 1e-12)

    def line_graph_data(self, data, lazy_sbf=False):
        """Featurisation (reference xgnn.py:39-72) -> (line-graph Data, GraphPlan).  ``lazy_sbf`` (the
        model's own forward): edge_sbf's [T, S] rows are written only if a consumer reads them rather than
        their factors (ops.materialize_sbf; the fused center forward reads only the factors)."""
        if "batch" not in data._store:  # single molecule: the reference adds a zero batch vector
            data.batch = torch.zeros(data.x.shape[0], dtype=torch.int64, device=data.x.device)
        plan = GraphPlan.from_atom_batch(data)
        lg = plan.lg
        pos = data.atom_pos
        if self._fused_basis():  # distances, envelope, radial basis and the 42 Bessel terms: one kernel
            dist, env, node_rbf, bessel = ops.edge_basis(pos, lg, self.rbf_layer.frequencies, self.cutoff,
                                                         self.sbf_layer.num_spherical, self.sbf_layer.num_radial)
            env = env.unsqueeze(1)
        else:
            dist = (pos.index_select(0, lg.edge_src) - pos.index_select(0, lg.edge_dst)).norm(dim=1)
            env = self.envelop_function(dist).unsqueeze(1)
            node_rbf = self.rbf_layer(dist) * env
            bessel = None
        fused_feat = ops.featurize_supported(data.edge_attr, env, self.mat_trans, self.emb_trans)
        if fused_feat:  # both Linear layers, the envelope scale and SiLUs in one kernel (csrc/feature.hip)
            neo_x = ops.featurize(data.edge_attr, env, self.mat_trans, self.emb_trans)
        else:
            neo_x = self.mat_trans.fused(data.edge_attr * env, act=ops.ACT_SILU)
        # under molecule sharding the embedding's per-batch rules count the global batch's atoms
        # (dist.collate_shard); otherwise this batch's
        edge_term, edge_proj = self._edge_term(data, plan)
        sbf = self.sbf_layer.from_positions(dist, pos, lg, bessel, lazy=lazy_sbf)
        if not fused_feat:
            neo_x = self.emb_trans.fused(neo_x, act=ops.ACT_SILU)
        line = Data(x=neo_x, edge_sbf=sbf, node_rbf=node_rbf, **edge_term)
        line._store["_x2g_plan"] = plan
        if edge_proj is not None:
            line._store["_x2g_edge_proj"] = edge_proj
        return line, plan

    def _edge_term(self, data, plan):
        """(the line-graph Data's edge-term fields, per-layer lin_edge tables or None): the element table and the
        row of it each line node's triplets read (xgnn.py:57-58)."""
        table, edge_proj = self._edge_tables(data.x, data._store.get("_x2g_count_z"))
        return dict(edge_attr=table, edge_attr_row=plan.dst_type), edge_proj

    def _edge_tables(self, atomic_num, count_z=None):
        """(element table, per-layer lin_edge tables or None).  The embedding Linear, edgenn and every
        conv's lin_edge all act on the <= 10-row element table (xgnn.py:57-58): where compiled they
        run as ONE small-table chain (ops.table_chain, one launch each way); the trunk then reads
        its lin_edge tables from ``_x2g_edge_proj`` instead of applying edgenn / lin_edge itself.
        (Run on a second stream under the triplet build / featurisation it measured 0.4 % slower in
        the step: its workgroup holds a CU the full-chip MFMA kernels then wait for.)"""
        emb = self.emb_block
        rows = emb.element_rows(atomic_num, count_z)
        trunk_stages = self.fin_model.edge_table_stages() if rows is not None else None
        if trunk_stages is not None:
            act = ops.ACT_SILU if emb.activate else ops.ACT_NONE
            stages = [(emb.lin, act, -1)] + [(m, a, p + 1) for (m, a, p) in trunk_stages]
            if len(stages) <= ops.TABLE_MAX_STAGES and ops.table_chain_supported(rows, [m for m, _, _ in stages]):
                outs = ops.table_chain(rows, stages)
                return outs[0], tuple(outs[3:])
        return emb.element_table(atomic_num, count_z), None

    def forward(self, data):
        line, plan = self.line_graph_data(data, lazy_sbf=ops.LAZY_SBF)
        return self.fin_model(line, edge_index_0=plan.lg.edge_src, atom_batch=data.batch)


class xgnn_poly(_XGNNBase):
    def __init__(self, conv_layers=4, sbf_dim=7, rbf_dim=16, in_channels=256, heads=16, embedding_size=128,
                 device="cpu", attn_dropout=0.0, dropout_seed=0, num_target=1, conv_beta: bool = False):
        super().__init__()
        trunk = SBFTransformer(conv_layers=conv_layers, emb_size=embedding_size, sbf_dim=sbf_dim, rbf_dim=rbf_dim,
                               in_channels=in_channels, heads=heads, attn_dropout=attn_dropout,
                               dropout_seed=dropout_seed, num_target=num_target, beta=conv_beta)
        self._build(trunk, sbf_dim, rbf_dim, in_channels, embedding_size, device)


class xgnn_poly_global(_XGNNBase):
    def __init__(self, conv_layers=4, sbf_dim=7, rbf_dim=16, in_channels=256, heads=16, embedding_size=128,
                 device="cpu", pool_option="mean", attn_dropout=0.0, dropout_seed=0, num_target=1,
                 conv_beta: bool = False):
        super().__init__()
        trunk = SBFTransformerGlobal(conv_layers=conv_layers, emb_size=embedding_size, sbf_dim=sbf_dim,
                                     rbf_dim=rbf_dim, in_channels=in_channels, heads=heads, pool_option=pool_option,
                                     attn_dropout=attn_dropout, dropout_seed=dropout_seed, num_target=num_target,
                                     beta=conv_beta)
        self._build(trunk, sbf_dim, rbf_dim, in_channels, embedding_size, device)


class xgnn_poly_multi(_XGNNBase):
    """All targets on one trunk (SBFTransformerMulti): ``forward`` returns [B, mol_targets + atom_targets], the
    ``mol_targets`` per-molecule (intensive) columns first, then the ``atom_targets`` per-atom-summed (extensive)
    ones, QM9's order for its 12 properties at (6, 6)."""

    def __init__(self, conv_layers=4, sbf_dim=7, rbf_dim=16, in_channels=256, heads=16, embedding_size=128,
                 device="cpu", atom_targets=6, mol_targets=6, pool_option="mean", attn_dropout=0.0, dropout_seed=0,
                 conv_beta: bool = False):
        super().__init__()
        trunk = SBFTransformerMulti(conv_layers=conv_layers, emb_size=embedding_size, sbf_dim=sbf_dim,
                                    rbf_dim=rbf_dim, in_channels=in_channels, heads=heads, atom_targets=atom_targets,
                                    mol_targets=mol_targets, pool_option=pool_option, attn_dropout=attn_dropout,
                                    dropout_seed=dropout_seed, beta=conv_beta)
        self._build(trunk, sbf_dim, rbf_dim, in_channels, embedding_size, device)


class xgnn_poly_v2(_XGNNBase):
    """xgnn_poly's featurisation in front of SBFTransformerV2 (reference model.py:100-150), whose edge term is
    recomputed per layer from the line-node features pooled per atom.  V2 reads no element embedding, so there is
    no ``emb_block``: the per-triplet ``edge_attr`` is the triplet's middle atom (what ``atom_embeddings[atom_j]``,
    xgnn.py:57-58, indexes), and ``edge_atom_row`` the same atom per destination line node (the plan's
    ``edge_dst``), which lets the trunk run the chain on the atom rows."""

    def __init__(self, conv_layers=4, sbf_dim=7, rbf_dim=16, in_channels=128, heads=16, embedding_size=128,
                 device="cpu"):
        super().__init__()
        trunk = SBFTransformerV2(conv_layers=conv_layers, emb_size=embedding_size, sbf_dim=sbf_dim, rbf_dim=rbf_dim,
                                 in_channels=in_channels, heads=heads)
        self._build(trunk, sbf_dim, rbf_dim, in_channels, embedding_size, device)
        del self.emb_block

    def _edge_term(self, data, plan):
        return dict(edge_attr=plan.lg.atom_j, edge_atom_row=plan.lg.edge_dst), None
