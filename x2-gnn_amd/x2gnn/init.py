"""The reference's initialisation for a from-scratch run: ``reference_init_(model)``.

The reference initialises most ``Linear`` weights with ``Glorot_Ortho_`` (initializer.py:29-35: orthogonal, rescaled
to variance 2 / (fan_in + fan_out)) and zero biases, inside each module's ``reset_parameters``.  Here the
constructors keep torch's default initialisation (the tests build models under ``torch.manual_seed`` and rely on
those bits; ``SBFTransformerV2`` alone applies its trunk's rules itself), and this function applies the reference's
rules afterwards, in place, to a whole model, a bare trunk or a bare conv.

"Glorot": ``model.glorot_ortho_`` on the weight and a zero bias where there is one.  "default":
``nn.Linear.reset_parameters()``.

=====================================================================  =========  ================================
module                                                                 rule       reference
=====================================================================  =========  ================================
``mat_trans``, ``rbf_trans``, ``emb_trans``                            Glorot     xgnn.py:26-36
``emb_block.lin``                                                      Glorot     atom_embedding.py:16-17
``emb_block.embedding``                                                N(0, 1), padding row 0      (same)
every ``ResidualLayer.lin0`` / ``lin1``                                Glorot     residual_layer.py:15-19
trunk ``dense_bf_skip[i]``, ``edgenn[0]`` / ``[2]`` (V2: every layer)  Glorot     model.py:29-36, 118-130
``AtomWise.lin_rbf`` and every ``Linear`` of its ``mlp``               Glorot     readout.py:26-32
``MolWise.lin_rbf``                                                    Glorot     readout.py:60-62
``MolWise.mlp``                                                        default    (same)
conv ``lin_sbf.weight``, ``lin_rbf.weight``; ``lin_sbf.bias`` zero     Glorot     sbftransformer_conv.py:77-82
conv ``lin_key`` / ``query`` / ``value`` / ``edge`` / ``skip`` / ``beta``  default  sbftransformer_conv.py:84-91
``rbf_layer.frequencies``                                              untouched  radial_basis_layer.py (n pi)
=====================================================================  =========  ================================

(The reference writes ``torch.nn.init.zeros`` for the conv's ``lin_sbf.bias``, a typo for ``zeros_``; the conv's
``lin_rbf`` has no bias.)

The result is NOT bit-equal to a reference model built under the same seed: the reference interleaves construction
and initialisation, so its draws come in another order.  What is equal is the distribution of every tensor.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from .layers import AtomWise, EmbeddingBlock, MolWise, RadialBasis, ResidualLayer
from .model import _Trunk, glorot_ortho_
from .sbftransformer_conv import SBFTransformerConv
from .xgnn import _XGNNBase


class _Rules:
    """Applies the rules (``dry``: only names them) and keeps {parameter name: rule} of what they visited."""

    def __init__(self, generator=None, dry=False):
        self.generator, self.dry = generator, dry
        self.visited = {}

    def _mark(self, prefix, mod, weight, bias=None):
        for n, _ in mod.named_parameters(recurse=False):
            self.visited[prefix + n] = bias if n == "bias" and bias is not None else weight

    def glorot(self, prefix, lin):
        if not self.dry:
            with torch.no_grad():
                glorot_ortho_(lin.weight, generator=self.generator)
                if lin.bias is not None:
                    lin.bias.zero_()
        self._mark(prefix, lin, "glorot", "zero")

    def default(self, prefix, lin):
        if self.dry:
            pass
        elif self.generator is None:
            lin.reset_parameters()
        else:  # nn.Linear.reset_parameters with the draws taken from the generator
            nn.init.kaiming_uniform_(lin.weight, a=math.sqrt(5), generator=self.generator)
            if lin.bias is not None:
                bound = 1 / math.sqrt(lin.in_features) if lin.in_features > 0 else 0
                nn.init.uniform_(lin.bias, -bound, bound, generator=self.generator)
        self._mark(prefix, lin, "default")

    def embedding(self, prefix, emb):
        if self.dry:
            pass
        elif self.generator is None:
            emb.reset_parameters()
        else:  # nn.Embedding.reset_parameters
            nn.init.normal_(emb.weight, generator=self.generator)
            if emb.padding_idx is not None:
                with torch.no_grad():
                    emb.weight[emb.padding_idx].fill_(0)
        self._mark(prefix, emb, "embedding")

    def untouched(self, prefix, mod):
        self._mark(prefix, mod, "untouched")


def _linears(prefix, mod):
    """(name prefix, Linear) of every nn.Linear under ``mod`` (itself included), in module order."""
    return [(f"{prefix}{n}." if n else prefix, m) for n, m in mod.named_modules() if isinstance(m, nn.Linear)]


def _apply(r, name, mod):
    """The rules of one module whose class names them; ``name`` is its dotted path in the model ('' = the root)."""
    pre = name + "." if name else ""
    if isinstance(mod, _XGNNBase):
        for n in ("mat_trans", "rbf_trans", "emb_trans"):
            r.glorot(f"{pre}{n}.", getattr(mod, n))
    elif isinstance(mod, EmbeddingBlock):
        r.embedding(pre + "embedding.", mod.embedding)
        r.glorot(pre + "lin.", mod.lin)
    elif isinstance(mod, ResidualLayer):
        r.glorot(pre + "lin0.", mod.lin0)
        r.glorot(pre + "lin1.", mod.lin1)
    elif isinstance(mod, _Trunk):
        for p, lin in _linears(pre + "dense_bf_skip.", mod.dense_bf_skip) + _linears(pre + "edgenn.", mod.edgenn):
            r.glorot(p, lin)
    elif isinstance(mod, AtomWise):
        for p, lin in [(pre + "lin_rbf.", mod.lin_rbf)] + _linears(pre + "mlp.", mod.mlp):
            r.glorot(p, lin)
    elif isinstance(mod, MolWise):
        r.glorot(pre + "lin_rbf.", mod.lin_rbf)
        for p, lin in _linears(pre + "mlp.", mod.mlp):
            r.default(p, lin)
    elif isinstance(mod, SBFTransformerConv):
        r.glorot(pre + "lin_sbf.", mod.lin_sbf)
        r.glorot(pre + "lin_rbf.", mod.lin_rbf)
        for n in ("lin_key", "lin_query", "lin_value", "lin_edge", "lin_skip", "lin_beta"):
            lin = getattr(mod, n, None)
            if lin is not None:
                r.default(f"{pre}{n}.", lin)
    elif isinstance(mod, RadialBasis):
        r.untouched(pre, mod)


def _run(model, rules):
    for name, mod in model.named_modules():
        _apply(rules, name, mod)
    return rules.visited


def reference_init_rules(model):
    """{parameter name: "glorot" | "zero" | "default" | "embedding" | "untouched"}: what ``reference_init_`` does
    to each parameter of ``model`` (nothing is written).  A parameter no rule names raises ValueError naming it."""
    rules = _run(model, _Rules(dry=True))
    missed = sorted(set(dict(model.named_parameters())) - set(rules))
    if missed:
        raise ValueError(f"reference_init_: no rule for the parameters {missed}")
    return rules


def reference_init_(model, generator=None):
    """Apply the reference's ``reset_parameters`` rules (the module docstring's table) to ``model`` in place and
    return it.  ``model``: ``xgnn_poly``, ``xgnn_poly_global``, ``xgnn_poly_multi``, ``xgnn_poly_v2``, a bare trunk
    or a bare ``SBFTransformerConv``.

    It runs on whatever device the parameters are on; the documented use is on the CPU, before ``.to(device)``::

        model = reference_init_(x2gnn.xgnn_poly(**cfg), torch.Generator().manual_seed(0)).to("cuda")

    ``generator``: every draw comes from it (it must live on the parameters' device), so two calls with equally
    seeded generators give equal bits; None: torch's global generator.

    A parameter no rule names raises ValueError naming it, before anything is written: a module added later
    cannot be left at torch's default silently."""
    reference_init_rules(model)
    _run(model, _Rules(generator))
    return model
