"""SBFTransformerV2 / xgnn_poly_v2 without a GPU: the module tree against the reference's (the ``state_dict`` keys and
shapes tests/golden/model_v2.npz recorded from it), the constructor's refusal, the exported symbols, the attention
route of a per-atom edge table, and the float64 statement the GPU tests use (tests/model_v2_ref.py) against the
reference's own energies and gradients."""
import types

import numpy as np
import pytest
import torch

from conftest import golden
from helpers import batch_from_fixture, energy_rel_err, model_cfg


def test_state_dict_equals_the_reference():
    import x2gnn

    z = golden("model_v2.npz")
    want = [(str(k), tuple(int(d) for d in str(s).split())) for k, s in zip(z["state_keys"], z["state_shapes"])]
    m = x2gnn.xgnn_poly_v2(**model_cfg(z))
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    trunk = [k[len("fin_model."):] for k, _ in want if k.startswith("fin_model.")]
    t = x2gnn.SBFTransformerV2(conv_layers=2, emb_size=128, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16)
    assert list(t.state_dict()) == trunk
    for i in range(2):
        for j in (0, 2):
            assert f"edgenn.{i}.{j}.weight" in trunk and f"edgenn.{i}.{j}.bias" in trunk
    assert not any(k.startswith("emb_block") for k, _ in want)
    assert {k.split(".")[0] for k in trunk} == {"edgenn", "convs", "readouts", "bf_skip", "af_skip", "dense_bf_skip"}


def test_constructor():
    import x2gnn

    with pytest.raises(ValueError, match="emb_size"):
        x2gnn.SBFTransformerV2(conv_layers=2, emb_size=64, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16)
    with pytest.raises(ValueError, match="emb_size"):
        x2gnn.xgnn_poly_v2(conv_layers=1, rbf_dim=6, embedding_size=64)
    t = x2gnn.SBFTransformerV2(1, 128, 7, K=5)  # the reference's positional order and defaults (K unused)
    assert t.rbf_dim == 16 and t.convs[0].heads == 8 and t.in_channels == 128
    m = x2gnn.xgnn_poly_v2()
    assert m.fin_model.conv_layers == 4 and len(m.fin_model.edgenn) == 4 and m.fin_model.convs[0].heads == 16


def test_reset_parameters():
    """The reference's reset_parameters (model.py:118-130): Glorot-orthogonal weights (orthogonal rows rescaled to
    the variance 2 / (fan_in + fan_out)) and zero biases on edgenn, dense_bf_skip, lin_sbf; lin_rbf's weight too."""
    import x2gnn

    torch.manual_seed(3)
    t = x2gnn.SBFTransformerV2(conv_layers=2, emb_size=128, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16)
    for e in t.edgenn:
        for lin in (e[0], e[2]):
            w = lin.weight.detach().double()
            assert abs(float(w.var()) - 2.0 / 256) < 1e-9 and float(lin.bias.detach().abs().max()) == 0
            gram = w @ w.T
            assert float((gram - torch.diag(torch.diag(gram))).abs().max()) < 1e-6 * float(gram.diag().max())
    for lin in list(t.dense_bf_skip) + [c.lin_sbf for c in t.convs]:
        assert float(lin.bias.detach().abs().max()) == 0
        assert abs(float(lin.weight.detach().var()) * sum(lin.weight.shape) - 2.0) < 1e-5
    assert abs(float(t.convs[1].lin_rbf.weight.detach().var()) * (128 + 6) - 2.0) < 1e-5
    before = t.edgenn[0][0].weight.detach().clone()
    t.reset_parameters()
    assert not torch.equal(before, t.edgenn[0][0].weight)


def test_symbols():
    import x2gnn
    from x2gnn import _lib, ops

    assert "SBFTransformerV2" in x2gnn.__all__ and "xgnn_poly_v2" in x2gnn.__all__
    assert callable(ops.atom_context) and ops._ATOM_CTX is True
    lib = _lib.load()
    for name in ("x2g_atom_context_fwd", "x2g_atom_context_bwd"):
        assert name in _lib.ATOMCTX_SIGNATURES and getattr(lib, name).argtypes == _lib.ATOMCTX_SIGNATURES[name]
        assert name not in _lib.SIGNATURES  # (outside the recorded ABI)


# ------------------------------------------------------------------------------------------------ the route
PER_DST = 2
DST_ATOM, SRC_ATOM, ATOM_INFO = object(), object(), object()


def _line_graph(**kw):
    """tests/test_attention_route.py's symmetric batch (100 atoms of degree <= 12 in 7 packs) with the per-atom
    pair GraphPlan sets."""
    f = dict(E=600, N=100, T=5000, edge_rev=object(), rev_trip=object(), max_degree=12, atom_type=object(),
             src_type=object(), dst_type=object(), dst_atom=DST_ATOM, src_atom=SRC_ATOM, center_order=object(),
             pack_order=object(), center_packs=np.zeros(8, dtype=np.int32), center_rows=16, pack_info=object(),
             atom_pack_info=lambda: ATOM_INFO, center_hubs=0, center_mixed=False,
             sbf_factors=(object(), object(), object()), sbf_pending=None, mol_counts=None, _infer_tile_cache={})
    f.update(kw)
    return types.SimpleNamespace(**f)


def _route(lg, edge_row=DST_ATOM, edge_rows=100, keeps=True, dropout=False):
    from x2gnn import ops

    return ops._attention_route(lg, PER_DST, edge_rows, edge_row, 16, 8, True, 42, keeps, False, dropout, True)


def test_per_atom_table_takes_the_center_route(monkeypatch):
    """A table of N = 100 rows whose per-destination rows are lg.dst_atom: the fused center forward reading
    lg.src_atom per source and the atom's own index from the second info tensor, the P-row center backward; no
    16-row limit (that is the fold passes').  Dropout composes."""
    from x2gnn import ops

    lg = _line_graph()
    r = _route(lg)
    assert (r.forward, r.backward, r.atom_table) == ("fused", "center_p", True)
    assert r.src_row is SRC_ATOM and r.info is ATOM_INFO and r.factors == lg.sbf_factors[1:]
    assert _route(lg, dropout=True).dropout_refusal is None
    assert _route(lg, keeps=False).backward is None and _route(lg, keeps=False).forward == "fused"
    # the same table under the element pair's identity is not recognised, and keeps the 16-row limit
    r = _route(lg, edge_row=lg.dst_type)
    assert (r.atom_table, r.factors, r.backward, r.src_row) == (False, None, "dst_plain", lg.src_type)
    assert "dst_atom" in _route(lg, edge_row=object(), dropout=True).dropout_refusal
    monkeypatch.setattr(ops, "_CENTER_P", False)
    assert _route(lg).backward == "center_s"


@pytest.mark.parametrize("why", ["_CENTER", "unsymmetric", "degree", "_CENTER_BWD"])
def test_per_atom_table_off_the_center_route(monkeypatch, why):
    """Off the center route the fold passes (<= 16 table rows) are not chosen: no factors, the destination-major
    forward (or the S-reading center forward when only the center backward is off) and the plain two-pass
    backward."""
    from x2gnn import ops

    lg = _line_graph()
    if why in ("_CENTER", "_CENTER_BWD"):
        monkeypatch.setattr(ops, why, False)
    elif why == "unsymmetric":
        lg = _line_graph(edge_rev=None, rev_trip=None, max_degree=None)
    else:
        lg = _line_graph(max_degree=ops.CENTER_MAX_DEGREE + 1)
    r = _route(lg)
    assert (r.factors, r.backward, r.atom_table) == (None, "dst_plain", True)
    assert r.forward == ("center" if why == "_CENTER_BWD" else "dst")
    assert r.alpha and r.sproj and not r.sbf_p and r.reads_sbf


# ------------------------------------------------------------------------------------------------ the statement
def test_float64_statement_equals_the_reference():
    """tests/model_v2_ref.py (what the GPU tests call the float64 statement) against the energies and gradients the
    reference's SBFTransformerV2 gave (float32 there: the energy tolerance of the GPU tests, gradients 2e-3)."""
    import model_v2_ref

    z = golden("model_v2.npz")
    b = batch_from_fixture(z, shipped=False)
    m, e = model_v2_ref.statement(model_cfg(z), int(z["weight_seed"]), b)
    assert energy_rel_err(e.detach().numpy(), z["energies"]) < 1e-4
    torch.nn.functional.smooth_l1_loss(e, b.y.double()).backward()
    assert [n for n, _ in m.named_parameters()] == [k[len("gnorm."):] for k in z.files if k.startswith("gnorm.")]
    top = max(float(z[k]) for k in z.files if k.startswith("gnorm."))
    for n, p in m.named_parameters():
        ref = float(z["gnorm." + n])
        got = 0.0 if p.grad is None else float(p.grad.norm())
        assert abs(got - ref) <= 2e-3 * ref + 1e-6 * top, (n, got, ref)
        if "grad." + n in z.files:
            g = z["grad." + n]
            assert np.abs(p.grad.numpy() - g).max() <= 2e-3 * np.abs(g).max() + 1e-6 * top, n
