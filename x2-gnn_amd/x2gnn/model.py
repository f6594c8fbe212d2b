"""SBF-transformer trunk over the line graph (reference model.py:11-98), same module tree and
``forward(data, edge_index_0, atom_batch)`` surface.

Per layer: conv -> graph LayerNorm (per molecule) -> ResidualLayer -> SiLU(Linear) -> +residual
-> 2 x ResidualLayer -> readout; energies are the per-atom readouts summed over layers and
pooled per molecule.  Graph kernels (attention, LayerNorm, pools) run in libx2g.so; the dense
E- and N-row layers are fp32 GEMMs.

``data`` is the line-graph ``Data`` of the reference (x[E,D], edge_index[2,T], edge_attr,
batch[E], edge_sbf[T,42], node_rbf[E,R]).  Two additions let ``xgnn_poly`` skip work the
reference repeats per triplet: ``data._x2g_plan`` (a prebuilt :class:`GraphPlan`) and
``data.edge_attr_row`` — when present, ``edge_attr`` is a per-element table [10, D] and line
node e uses row ``edge_attr_row[e]``, so ``edgenn`` and every ``lin_edge`` run on 10 rows
instead of T (the reference's edge_attr rows are copies of those rows, xgnn.py:57-58).

``SBFTransformerV2`` (reference model.py:100-150) is the same trunk with the edge term recomputed in every layer
from the line-node features pooled per atom; with ``data.edge_atom_row`` that chain runs on the N atom rows
(``ops.atom_context``) and the attention reads one table row per center atom.
"""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.nn import ModuleList, Sequential, SiLU

from . import ops
from .layers import AtomWise, Linear, MolWise, ResidualLayer, run_mlp
from .plan import GraphPlan
from .sbftransformer_conv import SBFTransformerConv


class LayerNorm(nn.Module):
    """torch_geometric.nn.LayerNorm(mode='graph', affine=False) on contiguous molecule segments."""

    def __init__(self, in_channels, eps=1e-5, affine=False, mode="graph"):
        super().__init__()
        if affine or mode != "graph":
            raise NotImplementedError("graph mode, affine=False (X2-GNN's configuration)")
        self.in_channels, self.eps = in_channels, eps

    def forward(self, x, batch=None, rowptr=None, num_graphs=None):
        if rowptr is None and batch is None:
            xc = x - x.mean()
            return xc / (xc.std(unbiased=False) + self.eps)
        if rowptr is None:
            num_graphs = int(batch.max()) + 1
            rowptr = ops.csr_rowptr(batch, num_graphs)
        return ops.graph_layer_norm(x, rowptr, num_graphs, self.eps)


def _plan_of(data, edge_index_0, atom_batch):
    plan = data._store.get("_x2g_plan") if hasattr(data, "_store") else None
    return plan if plan is not None else GraphPlan.from_line_data(data, edge_index_0, atom_batch)


class _ReadoutFamily:
    """One family of readouts (one per layer output) during a trunk forward: collects the layer outputs, then
    runs the family's batched pool and its batched readout MLPs, or readout by readout where those do not apply."""

    def __init__(self, readouts, readout_fn, feature_fn=None, pool_fn=None, pool_out=None):
        self.readouts, self.readout_fn, self.feature_fn = readouts, readout_fn, feature_fn
        self.pool_fn, self.pool_out = pool_fn, pool_out

    def start(self, is_cuda):
        self.results, self.feats = None, []
        self.grouped = is_cuda and self.feature_fn is not None
        self.pooled_xs = [] if self.grouped and self.pool_fn is not None else None

    def add(self, i, x):
        if self.pooled_xs is not None:
            self.pooled_xs.append(x)
        elif self.grouped:
            self.feats.append(self.feature_fn(i, x))
        else:
            r = self.readout_fn(i, x)
            self.results = r if self.results is None else self.results + r

    def finish(self):
        feats, results = self.feats, self.results
        if self.pooled_xs is not None:
            feats = self.pool_fn(self.pooled_xs)
            if feats is None:
                feats = [self.feature_fn(i, x) for i, x in enumerate(self.pooled_xs)]
        if self.grouped:
            mlps = [r.mlp for r in self.readouts]
            if ops.readout_mlps_supported(feats, mlps):
                r = ops.readout_mlps(feats, mlps, pool=self.pool_out)
                if self.pool_out is not None:
                    r._x2g_pooled = True
                return r
            for m, f in zip(mlps, feats):
                r = run_mlp(m, f)
                results = r if results is None else results + r
        return results


def glorot_ortho_(tensor, scale=2.0, generator=None):
    """The reference's ``Glorot_Ortho_`` (initializer.py:29-35): orthogonal, rescaled to the Glorot variance.
    ``generator``: where the draws come from (None: torch's global generator, as the reference)."""
    nn.init.orthogonal_(tensor, generator=generator)
    with torch.no_grad():
        tensor.mul_(torch.sqrt(scale / ((tensor.shape[0] + tensor.shape[1]) * tensor.var())))
    return tensor


class _Trunk(nn.Module):
    def _build(self, conv_layers, emb_size, sbf_dim, rbf_dim, in_channels, heads, readout, attn_dropout=0.0,
               dropout_seed=0, beta=False):
        self.in_channels = in_channels
        self.rbf_dim = rbf_dim
        self.edgenn = Sequential(Linear(emb_size, emb_size), SiLU(), Linear(emb_size, emb_size))
        self.convs = ModuleList([
            SBFTransformerConv(in_channels=in_channels, out_channels=int(in_channels / heads), heads=heads,
                               sbf_dim=sbf_dim * rbf_dim, rbf_dim=rbf_dim, dropout=attn_dropout, edge_dim=emb_size,
                               beta=beta)
            for _ in range(conv_layers)])
        self.readouts = ModuleList([readout() for _ in range(conv_layers + 1)])
        self.bf_skip = ModuleList([ResidualLayer(in_channels) for _ in range(conv_layers)])
        self.af_skip = ModuleList([Sequential(ResidualLayer(in_channels), ResidualLayer(in_channels))
                                   for _ in range(conv_layers)])
        self.dense_bf_skip = ModuleList([Linear(in_channels, in_channels, bias=True) for _ in range(conv_layers)])
        self.AF = SiLU()
        self.LayerNorm = LayerNorm(in_channels=in_channels, eps=1e-8, affine=False)
        self.conv_layers = conv_layers
        # attention dropout's (seed, step): a training forward advances the step on the device (a captured step
        # on every replay) and hands a copy, with the layer's index as salt, to every conv.  Non-persistent: the
        # model's state_dict is the same with and without dropout (Trainer.state_dict carries it).
        self.attn_dropout = float(attn_dropout)
        self.register_buffer("attn_dropout_state", torch.tensor([int(dropout_seed), 0], dtype=torch.int64),
                             persistent=False)

    def _dropout_key(self):
        """This forward's key (None: no dropout — eval, or p = 0 — and the state is not touched)."""
        if not (self.training and self.attn_dropout > 0):
            return None
        self.attn_dropout_state[1] += 1
        return self.attn_dropout_state.clone()

    def edge_table_stages(self):
        """edgenn -> every conv's lin_edge as (Linear, act, parent) stages for ops.table_chain (parent
        -1 = the element table, 0 = edgenn's output), or None for another layout."""
        mods = list(self.edgenn)
        if len(mods) != 3 or not (isinstance(mods[0], Linear) and isinstance(mods[1], SiLU)
                                  and isinstance(mods[2], Linear)):
            return None
        if any(c.lin_edge is None for c in self.convs):
            return None
        return ([(mods[0], ops.ACT_SILU, -1), (mods[2], ops.ACT_NONE, 0)]
                + [(c.lin_edge, ops.ACT_NONE, 1) for c in self.convs])

    def _layers(self, data, plan, families):
        """The conv layers with their readouts: ``families``, the _ReadoutFamily list of this forward (one for the
        single-family trunks, two for SBFTransformerMulti); returns their results in that order.  A family with
        ``pool_out = (seg_rowptr, S)``: the batched readout heads may sum the per-atom results per molecule
        themselves (the result then carries ``_x2g_pooled``)."""
        edge_term = self._edge_terms(data, plan)
        out = data.x
        # The readouts (reference model.py:41,50) hang off the layer chain; results accumulate in
        # layer order (deterministic).  (Run on a second stream, overlapping the next layer, they
        # measured slower: 6.30 vs 6.00 ms/step — the persistent one-workgroup-per-CU kernels of the
        # main chain lose more to the shared CUs than the overlap gains; that path is gone.)
        # Batched readout MLPs: each family collects every readout's MLP input, then one batched launch per
        # MLP layer for all its readouts (ops.readout_mlps) instead of three launches per readout; the
        # readouts' edge -> atom pools of every layer output as one launch each way (pool_fn,
        # ops.rbf_pool_batch) after the last layer; per readout where that is unsupported (_ReadoutFamily)
        for f in families:
            f.start(out.is_cuda)

        def readout(i, x):
            for f in families:
                f.add(i, x)

        # gradient fan-in in place: the layer inputs and the radial basis feed several fused ops each
        fan = self._fan_in_ok(data, out)
        if fan:
            data.node_rbf._x2g_fanin = ops.FanIn()
            out._x2g_fanin = ops.FanIn()
        readout(0, out)
        sbf = data.edge_sbf
        drop_key = self._dropout_key()
        # (every layer's S projected up front in one launch, x2g_sbf_project_batch, measured 1.2 % slower in
        # the step A/B, profiles/r4ab1_step_ab_sbatch_feat.log: each layer's S written right before its
        # attention is still in the MALL when the attention reads it; projected 3 layers early it is not)
        for i in range(self.conv_layers):
            res0 = out
            edge_attr, edge_row, edge_proj = edge_term(i, out)
            out = self.convs[i](sbf=sbf, rbf=data.node_rbf, x=out, edge_index=data._store.get("edge_index"),
                                edge_attr=edge_attr, line_graph=plan.lg, edge_row=edge_row, edge_proj=edge_proj,
                                dropout_key=drop_key, dropout_salt=i)
            stats = getattr(out, "_x2g_rowstats", None)
            if stats is not None and self._ln_fusable(out, i):
                # the LayerNorm runs inside the tail's row chain, from the conv's per-row statistics
                out = self._tail(i, out, res0, ln=(stats, plan.line_ptr, plan.num_graphs, self.LayerNorm.eps))
            else:
                out = self.LayerNorm(out, rowptr=plan.line_ptr, num_graphs=plan.num_graphs)
                out = self._tail(i, out, res0)
            if fan:
                out._x2g_fanin = ops.FanIn()
            readout(i + 1, out)
        return [f.finish() for f in families]

    def _edge_terms(self, data, plan):
        """The one hook of a trunk's layers: a function (layer i, its input x) -> the conv's (edge_attr, edge_row,
        edge_proj).  Here the edge term is a constant of the forward: the lin_edge tables precomputed by the
        featurisation's table chain (``_x2g_edge_proj``), or edgenn applied once."""
        per_dst = "edge_attr_row" in data._store
        edge_proj = data._store.get("_x2g_edge_proj") if per_dst else None
        edge_attr = run_mlp(self.edgenn, data.edge_attr) if edge_proj is None else None
        edge_row = data.edge_attr_row if per_dst else None
        return lambda i, x: (edge_attr, edge_row, edge_proj[i] if edge_proj is not None else None)

    def _pool_batch(self, xs, rbf, edge_index_0, plan, readouts=None):
        """Every readout's edge -> atom pool (readout.py:39-41 / 66-67) in one launch each way, or
        None where the batched kernels do not cover the shapes."""
        lins = [r.lin_rbf for r in (self.readouts if readouts is None else readouts)]
        if rbf is None or len(xs) != len(lins) or not ops.rbf_pool_batch_supported(xs, rbf, [l.weight for l in lins]):
            return None
        return ops.rbf_pool_batch(xs, rbf, [l.weight for l in lins], [l.bias for l in lins], edge_index_0,
                                  plan.atom_rowptr, plan.num_atoms)

    def _tail_linears(self, i):
        lins = [self.bf_skip[i].lin0, self.bf_skip[i].lin1, self.dense_bf_skip[i]]
        for r in self.af_skip[i]:
            lins += [r.lin0, r.lin1]
        return lins

    def _fan_in_ok(self, data, x):
        """True when every consumer of the layer inputs (readout rbf pool, conv projections, the
        tail's residual) and of the radial basis (readout pools, conv gates) is a fan-aware fused op,
        so their input gradients can be summed in place (ops.FanIn) instead of by autograd adds."""
        if not (ops._FAN_IN and x.is_cuda and x.dim() == 2 and torch.is_grad_enabled()):
            return False
        rbf = data.node_rbf
        if rbf is None or not ops.gate_supported(x.shape[1], rbf.shape[1]):
            return False
        for i, c in enumerate(self.convs):
            if not c.root_weight or not ops.conv_proj_fused_supported(
                    x, rbf, (c.lin_query.weight, c.lin_key.weight, c.lin_value.weight, c.lin_skip.weight),
                    (c.lin_query.bias, c.lin_key.bias, c.lin_value.bias, c.lin_skip.bias)):
                return False
            if not (ops._CHAIN and ops.chain_supported(x, self._tail_linears(i))):
                return False
        return True

    def _ln_fusable(self, x, i):
        """True when the graph LayerNorm before layer i's tail can run inside its row chain."""
        return ops._CHAIN and ops.chain_supported(x, self._tail_linears(i))

    def _tail(self, i, out, res0, ln=None):
        """bf_skip -> SiLU(dense_bf_skip(.)) + res0 -> af_skip (model.py:47-50): one row-chain
        kernel each way (ops.row_chain, 7 Linear stages) where compiled, else layer by layer.
        ``ln``: the row chain applies the preceding graph LayerNorm to ``out`` itself."""
        lins = self._tail_linears(i)
        if ops._CHAIN and ops.chain_supported(out, lins):
            S, H, RH, RE = ops.CHAIN_SILU, ops.CHAIN_HOLD, ops.CHAIN_RES_HELD, ops.CHAIN_RES_EXT
            flags = [S | H, S | RH, S | RE, S | H, S | RH, S | H, S | RH]
            return ops.row_chain(out, res0, lins, flags, ln=ln)
        out = self.bf_skip[i](out)
        out = self.dense_bf_skip[i].fused(out, act=ops.ACT_SILU, res=res0)  # SiLU(dense(out)) + res0
        return self.af_skip[i](out)


def _check_targets(n, least=1):
    n = int(n)
    if not least <= n <= ops.HEADS_K_MAX_TARGETS:
        raise ValueError(f"{least} .. {ops.HEADS_K_MAX_TARGETS} targets per readout family, got {n}")
    return n


class _AtomReadouts:
    """The per-atom family of a trunk: AtomWise ``self.readouts``, summed per molecule (model.py:11-54)."""

    def _atom_family(self, data, edge_index_0, plan):
        def readout(i, x):
            return self.readouts[i](x=x, rbf=data.node_rbf, num_atoms=plan.num_atoms, edge_index_0=edge_index_0,
                                    atom_rowptr=plan.atom_rowptr)

        def features(i, x):
            return self.readouts[i].features(x=x, rbf=data.node_rbf, num_atoms=plan.num_atoms,
                                             edge_index_0=edge_index_0, atom_rowptr=plan.atom_rowptr)

        def pools(xs):
            return self._pool_batch(xs, data.node_rbf, edge_index_0, plan, self.readouts)

        # the global add pool (model.py:53) fused into the batched readout heads where they run
        pool_out = (plan.mol_ptr, plan.out_graphs) if plan.out_graphs == plan.num_graphs else None
        return _ReadoutFamily(self.readouts, readout, features, pools, pool_out)

    @staticmethod
    def _atom_pooled(per_atom, plan):
        """[B, K]: the family's result summed per molecule (by the fused heads already, or here)."""
        if getattr(per_atom, "_x2g_pooled", False):
            return per_atom
        return ops.segment_sum(per_atom, plan.mol_ptr, plan.out_graphs)


class _MolReadouts:
    """The per-molecule family of a trunk: MolWise readouts (model.py:56-98)."""

    def _mol_family(self, data, edge_index_0, atom_batch, plan, readouts):
        kw = dict(rbf=data.node_rbf, num_atoms=plan.num_atoms, edge_index_0=edge_index_0, atom_batch=atom_batch,
                  dim_size=plan.out_graphs, atom_rowptr=plan.atom_rowptr, mol_rowptr=plan.mol_ptr[: plan.out_graphs + 1])

        def readout(i, x):
            return readouts[i](x=x, **kw)

        def features(i, x):
            return readouts[i].features(x=x, **kw)

        def pools(xs):
            atoms = self._pool_batch(xs, data.node_rbf, edge_index_0, plan, readouts)
            if atoms is None:
                return None
            return [r.finish(a, atom_batch, plan.out_graphs, kw["mol_rowptr"]) for r, a in zip(readouts, atoms)]

        return _ReadoutFamily(readouts, readout, features, pools)


class SBFTransformer(_Trunk, _AtomReadouts):
    """Trunk with per-atom readouts (extensive targets, reference model.py:11-54).  ``num_target`` = K: the
    readouts end in Linear(D, K) and ``forward`` returns [B, K] (K = 1: [B], the reference's tensor)."""

    def __init__(self, conv_layers, emb_size, sbf_dim, rbf_dim=16, in_channels=128, heads=8, attn_dropout=0.0,
                 dropout_seed=0, num_target=1, beta: bool = False):
        super().__init__()
        self.num_target = num_target = _check_targets(num_target)
        self._build(conv_layers, emb_size, sbf_dim, rbf_dim, in_channels, heads,
                    lambda: AtomWise(in_channels=in_channels, rbf_dim=rbf_dim, num_target=num_target),
                    attn_dropout=attn_dropout, dropout_seed=dropout_seed, beta=beta)

    def forward(self, data, edge_index_0, atom_batch):
        plan = _plan_of(data, edge_index_0, atom_batch)
        (per_atom,) = self._layers(data, plan, [self._atom_family(data, edge_index_0, plan)])
        out = self._atom_pooled(per_atom, plan)
        return out.view(-1) if self.num_target == 1 else out


class SBFTransformerGlobal(_Trunk, _MolReadouts):
    """Trunk with per-molecule readouts (intensive targets, reference model.py:56-98); ``num_target`` as
    SBFTransformer's."""

    def __init__(self, conv_layers, emb_size, sbf_dim, rbf_dim=16, in_channels=128, heads=8, pool_option="mean",
                 attn_dropout=0.0, dropout_seed=0, num_target=1, beta: bool = False):
        super().__init__()
        self.num_target = num_target = _check_targets(num_target)
        self._build(conv_layers, emb_size, sbf_dim, rbf_dim, in_channels, heads,
                    lambda: MolWise(in_channels=in_channels, rbf_dim=rbf_dim, num_target=num_target,
                                    pool_option=pool_option),
                    attn_dropout=attn_dropout, dropout_seed=dropout_seed, beta=beta)

    def forward(self, data, edge_index_0, atom_batch):
        plan = _plan_of(data, edge_index_0, atom_batch)
        (out,) = self._layers(data, plan, [self._mol_family(data, edge_index_0, atom_batch, plan, self.readouts)])
        return out.view(-1) if self.num_target == 1 else out


class SBFTransformerMulti(_Trunk, _AtomReadouts, _MolReadouts):
    """One trunk, two readout families (the multi-head readout of all 12 QM9 properties): ``readouts``, AtomWise
    with ``atom_targets`` outputs summed per molecule (extensive targets), and ``mol_readouts``, MolWise with
    ``mol_targets`` outputs (intensive targets).  ``forward`` returns [B, mol_targets + atom_targets], the
    per-molecule columns first (QM9's order: targets 0-5 intensive, 6-11 extensive).  Either count may be 0; that
    family then has no modules, and the model is SBFTransformer / SBFTransformerGlobal with a 2-d result."""

    def __init__(self, conv_layers, emb_size, sbf_dim, rbf_dim=16, in_channels=128, heads=8, atom_targets=6,
                 mol_targets=6, pool_option="mean", attn_dropout=0.0, dropout_seed=0, beta: bool = False):
        super().__init__()
        self.atom_targets, self.mol_targets = _check_targets(atom_targets, 0), _check_targets(mol_targets, 0)
        self.num_target = self.atom_targets + self.mol_targets
        if self.num_target < 1:
            raise ValueError("atom_targets + mol_targets must be at least 1")
        self._build(conv_layers, emb_size, sbf_dim, rbf_dim, in_channels, heads,
                    lambda: AtomWise(in_channels=in_channels, rbf_dim=rbf_dim, num_target=max(self.atom_targets, 1)),
                    attn_dropout=attn_dropout, dropout_seed=dropout_seed, beta=beta)
        if not self.atom_targets:
            self.readouts = ModuleList()
        self.mol_readouts = ModuleList([MolWise(in_channels=in_channels, rbf_dim=rbf_dim, num_target=self.mol_targets,
                                                pool_option=pool_option)
                                        for _ in range(conv_layers + 1 if self.mol_targets else 0)])

    def forward(self, data, edge_index_0, atom_batch):
        plan = _plan_of(data, edge_index_0, atom_batch)
        families = []
        if self.atom_targets:
            families.append(self._atom_family(data, edge_index_0, plan))
        if self.mol_targets:
            families.append(self._mol_family(data, edge_index_0, atom_batch, plan, self.mol_readouts))
        res = self._layers(data, plan, families)
        if self.atom_targets:
            res[0] = self._atom_pooled(res[0], plan)
        if len(res) == 1:
            return res[0]
        return torch.cat([res[1], res[0]], dim=1)


class SBFTransformerV2(_Trunk, _AtomReadouts):
    """The trunk whose edge term is recomputed per layer from the current line-node features (reference
    model.py:100-150): ``atoms_rep = scatter_add(x, edge_index_0)``, then per layer
    ``edge_attr = edgenn[i](atoms_rep[data.edge_attr])`` with ``data.edge_attr`` an integer [T] atom index per triplet,
    then the conv's lin_edge; the energies are divided by ``conv_layers``.  Same constructor (``K`` is unused, as in
    the reference), module tree and ``state_dict`` keys.

    When ``data`` carries ``edge_atom_row`` (int [E]: the plan's ``edge_dst``, the target atom of each line node,
    which is what ``data.edge_attr`` holds for every triplet into it: xgnn_poly_v2 sets both) the chain runs on the N
    atom rows (``ops.atom_context``) and the attention reads one table row per center atom.  Otherwise the literal
    form runs on T rows: correct for any index, and slow."""

    def __init__(self, conv_layers, emb_size, sbf_dim, rbf_dim=16, in_channels=128, K=2, heads=8):
        super().__init__()
        if emb_size != in_channels:
            # (the reference fails at the first forward: lin_edge is emb_size wide, edgenn in_channels wide)
            raise ValueError(f"SBFTransformerV2: emb_size ({emb_size}) must equal in_channels ({in_channels}): "
                             "edgenn's output is the input of every conv's lin_edge")
        self.num_target = 1
        self._build(conv_layers, emb_size, sbf_dim, rbf_dim, in_channels, heads,
                    lambda: AtomWise(in_channels=in_channels, rbf_dim=rbf_dim, num_target=1))
        self.edgenn = ModuleList([Sequential(Linear(in_channels, in_channels), SiLU(), Linear(in_channels, in_channels))
                                  for _ in range(conv_layers)])
        self.reset_parameters()

    def reset_parameters(self):
        """The reference's (model.py:118-130)."""
        for layer in self.dense_bf_skip:
            glorot_ortho_(layer.weight)
            nn.init.zeros_(layer.bias)
        for conv in self.convs:
            glorot_ortho_(conv.lin_sbf.weight)
            glorot_ortho_(conv.lin_rbf.weight)
            nn.init.zeros_(conv.lin_sbf.bias)
        for edge_nn in self.edgenn:
            for lin in (edge_nn[0], edge_nn[2]):
                glorot_ortho_(lin.weight)
                nn.init.zeros_(lin.bias)

    def edge_table_stages(self):
        return None  # (no per-element table: the edge term depends on the layer's input)

    def _edge_terms(self, data, plan):
        atom_row = data._store.get("edge_atom_row")

        def term(i, x):
            nn_i, conv = self.edgenn[i], self.convs[i]
            if atom_row is not None:  # one table row per atom, read per center atom
                tab = ops.atom_context(x, plan.atom_rowptr, plan.lg.edge_src, nn_i[0], nn_i[2], conv.lin_edge)
                return None, atom_row, tab
            atoms_rep = ops.segment_sum(x, plan.atom_rowptr, plan.num_atoms)
            return run_mlp(nn_i, atoms_rep.index_select(0, data.edge_attr)), None, None

        return term

    def _fan_in_ok(self, data, x):
        """The layer input has one more consumer, the atom context: fan-aware where its kernels run (the dx
        accumulate flag); the composition and the literal form leave the fan-in to autograd."""
        if not super()._fan_in_ok(data, x) or "edge_atom_row" not in data._store or not ops._ATOM_CTX:
            return False
        return all(ops.atom_context_supported(x, [e[0], e[2], c.lin_edge]) for e, c in zip(self.edgenn, self.convs))

    def forward(self, data, edge_index_0, atom_batch):
        plan = _plan_of(data, edge_index_0, atom_batch)
        (per_atom,) = self._layers(data, plan, [self._atom_family(data, edge_index_0, plan)])
        return self._atom_pooled(per_atom, plan).view(-1) / self.conv_layers
