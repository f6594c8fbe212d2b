"""x2gnn — MI355X-native X2-GNN message-passing hot path.

Host side (this package): the reference's model / operator surface (``xgnn_poly``,
``SBFTransformer``, ``SBFTransformerConv``, PyG-style ``Data``/``Batch``) on PyTorch-ROCm.
Device side: ``libx2g.so`` (hand-written gfx950 HIP kernels behind the C ABI in
``include/x2g.h``), loaded through :mod:`x2gnn._lib`.
"""
from .data import Batch, Data, collate, molecule_to_data
from .device_dataset import DeviceDataset
from .features import AOMatrices, ao_edge_features, bi_gen_edge_feature_6
from .fit import fit
from .graph import radius_graph
from .init import reference_init_
from .integrals import Basis, geom_scf_6, one_electron_matrices
from .layers import AtomWise, EmbeddingBlock, F_B_2D, MolWise, RadialBasis, ResidualLayer, poly_envelop
from .model import LayerNorm, SBFTransformer, SBFTransformerGlobal, SBFTransformerMulti, SBFTransformerV2
from .plan import GraphPlan
from .sbftransformer_conv import SBFTransformerConv
from .schedule import Plateau
from .train import Evaluator, Inference, Trainer
from .xgnn import xgnn_poly, xgnn_poly_global, xgnn_poly_multi, xgnn_poly_v2

__all__ = [
    "AOMatrices", "AtomWise", "Basis", "Batch", "Data", "DeviceDataset", "EmbeddingBlock", "Evaluator", "F_B_2D",
    "GraphPlan", "Inference", "LayerNorm", "MolWise", "Plateau", "RadialBasis", "ResidualLayer", "SBFTransformer",
    "SBFTransformerConv", "SBFTransformerGlobal", "SBFTransformerMulti", "SBFTransformerV2", "Trainer",
    "ao_edge_features", "bi_gen_edge_feature_6", "collate", "fit", "geom_scf_6", "molecule_to_data",
    "one_electron_matrices", "poly_envelop", "radius_graph", "reference_init_", "xgnn_poly", "xgnn_poly_global",
    "xgnn_poly_multi", "xgnn_poly_v2",
]
