"""The fp64 statement of the conv combine pass (tests/conv_combine_ref.py) against torch-float64 autograd of the
reference's four lines, the float32 emulation that fixes K, wrong variants that have to leave the bound, and the
constructor surface of SBFTransformerConv's ``concat`` / ``beta`` options.  No GPU."""
import numpy as np
import pytest
import torch

import conv_combine_ref as cr

SMALL = [(4, 8, 5), (16, 8, 7), (8, 16, 3)]  # (H, C, rows)


def _torch_statement(attn, x_r, w_beta, H, C, concat, dy):
    """out.view / out.mean, lin_skip's x_r, the gate and the blend exactly as the reference writes them
    (sbftransformer_conv.py:115-127), in float64 with autograd."""
    t = lambda a: None if a is None else torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    a, x, w = t(attn), t(x_r), t(w_beta)
    out = a.view(-1, H, C)
    out = out.reshape(-1, H * C) if concat else out.mean(dim=1)
    if w is not None:
        beta = torch.sigmoid(torch.cat([out, x, out - x], dim=-1) @ w.view(-1, 1))
        out = beta * x + (1 - beta) * out
    elif x is not None:
        out = out + x
    out.backward(torch.tensor(np.asarray(dy, np.float64)))
    g = lambda v: None if v is None else v.grad.numpy()  # noqa: E731
    return out.detach().numpy(), g(a), g(x), g(w)


def _close(got, want):
    scale = max(float(np.abs(want).max()), 1e-300)
    assert np.abs(got - want).max() <= 1e-12 * scale


@pytest.mark.parametrize("H,C,rows", SMALL)
@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("mode", ["gated", "skip", "no_xr"])
def test_statement_equals_torch_float64(H, C, rows, concat, mode):
    i = cr.combine_inputs(H, C, concat, rows)
    x = None if mode == "no_xr" else i["x_r"]
    w = i["w_beta"] if mode == "gated" else None
    y, da, dx, dw = _torch_statement(i["attn"], x, w, H, C, concat, i["dy"])
    fwd = cr.combine_fwd(i["attn"], x, w, H, C, concat)
    bwd = cr.combine_bwd(i["dy"], i["attn"], x, w, H, C, concat)
    _close(fwd["y"][0], y)
    _close(bwd["d_attn"][0], da)
    if x is not None:
        _close(bwd["d_xr"][0], dx)
    if w is not None:
        _close(bwd["dw"][0], dw)
    mu = y.mean(1)
    _close(fwd["stats"][0], np.stack([mu, ((y - mu[:, None]) ** 2).sum(1)], 1))
    for v, u in list(fwd.values()) + list(bwd.values()):
        assert (u >= np.abs(v) * (1 - 1e-12)).all()  # a unit is never below its value's magnitude


def test_emulation_ratios_and_k():
    rep = cr.emulation_report()
    assert set(rep) == set(cr.K) == set(cr.EMULATION_RATIO)
    for fam, (r, output, case) in rep.items():
        print(f"{fam}: {r:.3f} ({output}, {case})")
        assert r <= cr.EMULATION_RATIO[fam], (fam, r, output, case)
        assert 4 * cr.EMULATION_RATIO[fam] <= cr.K[fam]
        assert cr.K[fam] == 2.0 ** round(np.log2(cr.K[fam])) and cr.K[fam] < 8 * cr.EMULATION_RATIO[fam] + 1


def _leaves(fam, got, ref_unit):
    return cr.ratio(got, *ref_unit) > cr.K[fam]


@pytest.mark.parametrize("H,C,concat", [(16, 8, True), (16, 8, False), (4, 8, False), (16, 16, True)])
def test_wrong_variants_leave_the_bound(H, C, concat):
    i = cr.combine_inputs(H, C, concat, 65)
    a, x, w, dy = (np.asarray(i[k], np.float64) for k in ("attn", "x_r", "w_beta", "dy"))
    D = x.shape[1]
    fwd = cr.combine_fwd(a, x, w, H, C, concat)
    bwd = cr.combine_bwd(dy, a, x, w, H, C, concat)
    m = a if concat else a.reshape(-1, H, C).mean(1)
    beta = fwd["beta"][0][:, None]
    assert not _leaves("fwd", fwd["y"][0], fwd["y"])
    # the operands swapped: beta * out + (1 - beta) * x_r
    assert _leaves("fwd", beta * m + (1 - beta) * x, fwd["y"])
    # the third block of w_beta dropped
    w_no3 = w.copy()
    w_no3[2 * D:] = 0
    assert _leaves("fwd", cr.combine_fwd(a, x, w_no3, H, C, concat)["y"][0], fwd["y"])
    assert _leaves("bwd", cr.combine_bwd(dy, a, x, w_no3, H, C, concat)["d_xr"][0], bwd["d_xr"])
    if not concat:  # / H left out of the mean's backward
        assert _leaves("bwd", bwd["d_attn"][0] * H, bwd["d_attn"])
    # a 1e-5 relative perturbation of every per-row output
    for fam, (v, u) in (("fwd", fwd["y"]), ("fwd", fwd["beta"]), ("bwd", bwd["d_attn"]), ("bwd", bwd["d_xr"])):
        assert _leaves(fam, v * (1 + 1e-5), (v, u)), fam
    # the row statistics and dw_beta: 1e-5 at Dout <= 32; at Dout = 128 / 256 their worst-case units (M2's 2 |d| unit(y)
    # per channel, dw_beta's unit(s) of 3 Dout terms in every row's ds) are themselves above 1e-5 of the value: 1e-4
    eps = 1e-5 if D <= 32 else 1e-4
    for fam, (v, u) in (("stats", fwd["stats"]), ("dw", bwd["dw"])):
        assert _leaves(fam, v * (1 + eps), (v, u)), fam


def test_equal_rows_have_zero_units():
    """attn == x_r with concat: dbeta, ds and all of dw_beta have unit 0 (the kernel must return exact zeros)."""
    i = cr.combine_inputs(16, 8, True, 65, "equal")
    bwd = cr.combine_bwd(i["dy"], i["attn"], i["x_r"], i["w_beta"], 16, 8, True)
    for k in ("dbeta", "ds", "dw"):
        assert (bwd[k][0] == 0).all() and (bwd[k][1] == 0).all()
    emu = cr.emu_bwd(i["dy"], i["attn"], i["x_r"], i["w_beta"], 16, 8, True)
    assert (emu["dw"] == 0).all()


def test_saturated_inputs_reach_both_signs():
    i = cr.combine_inputs(16, 8, True, 65, "saturated")
    s = cr.combine_fwd(i["attn"], i["x_r"], i["w_beta"], 16, 8, True)["s"][0]
    assert s.max() >= 100 and s.min() <= -100
    emu = cr.emu_fwd(i["attn"], i["x_r"], i["w_beta"], 16, 8, True)
    assert np.isfinite(emu["beta"]).all() and np.isfinite(emu["y"]).all()
    assert (emu["beta"][s >= 95] == 1).all() and (emu["beta"][s <= -95] == 0).all()


def test_tiles():
    assert [cr.combine_tile(W) for W in cr.WIDTHS] == [32, 16, 8, 4]
    assert cr.combine_splits(0, 128) == 0 and cr.combine_splits(1, 128) == 1
    assert cr.combine_splits(8 * 128, 128) == 128 and cr.combine_splits(8 * 128 + 1, 128) == 128
    assert cr.combine_splits(8 * 127 + 1, 128) == 128 and cr.combine_splits(8 * 127, 128) == 127


# ------------------------------------------------------------------------------------------------ constructor surface
def test_constructor_surface():
    from x2gnn.sbftransformer_conv import SBFTransformerConv

    kw = dict(sbf_dim=42, rbf_dim=6, edge_dim=16)
    c = SBFTransformerConv(128, 8, heads=16, beta=True, **kw)
    assert c.beta and tuple(c.lin_beta.weight.shape) == (1, 384) and tuple(c.lin_skip.weight.shape) == (128, 128)
    assert "lin_beta.weight" in c.state_dict() and "lin_beta.bias" not in c.state_dict()
    c = SBFTransformerConv(128, 8, heads=16, beta=True, concat=False, **kw)
    assert tuple(c.lin_skip.weight.shape) == (8, 128) and tuple(c.lin_beta.weight.shape) == (1, 24)
    c = SBFTransformerConv(128, 8, heads=16, concat=False, **kw)
    assert tuple(c.lin_skip.weight.shape) == (8, 128) and c.lin_beta is None
    c = SBFTransformerConv(128, 8, heads=16, beta=True, root_weight=False, **kw)
    assert c.lin_beta is None and not c.beta
    default = SBFTransformerConv(128, 8, heads=16, **kw)
    assert sorted(default.state_dict()) == sorted([
        "lin_key.weight", "lin_key.bias", "lin_query.weight", "lin_query.bias", "lin_value.weight", "lin_value.bias",
        "lin_edge.weight", "lin_skip.weight", "lin_skip.bias", "lin_sbf.weight", "lin_sbf.bias", "lin_rbf.weight"])
    assert default.lin_beta is None and not default.beta and default.concat


def test_model_keyword():
    import x2gnn

    cfg = dict(conv_layers=2, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)
    base = x2gnn.xgnn_poly(**cfg)
    assert sorted(x2gnn.xgnn_poly(conv_beta=False, **cfg).state_dict()) == sorted(base.state_dict())
    for make in (x2gnn.xgnn_poly, x2gnn.xgnn_poly_global, x2gnn.xgnn_poly_multi):
        plain, gated = make(**cfg), make(conv_beta=True, **cfg)
        extra = sorted(set(gated.state_dict()) - set(plain.state_dict()))
        assert len(extra) == 2 and all(k.endswith("lin_beta.weight") for k in extra), extra
        assert not set(plain.state_dict()) - set(gated.state_dict())
        assert all(tuple(gated.state_dict()[k].shape) == (1, 384) for k in extra)


def test_binding_tables():
    from x2gnn import _lib

    names = {"x2g_conv_combine_fwd", "x2g_conv_combine_bwd", "x2g_conv_combine_splits",
             "x2g_conv_combine_bwd_workspace"}
    assert set(_lib.CONV_SIGNATURES) == names == set(_lib.CONV_RESTYPES)
    for table in (_lib.SIGNATURES, _lib.STAGED_SIGNATURES, _lib.MULTI_SIGNATURES):
        assert not names & set(table)
    assert len(_lib.CONV_SIGNATURES["x2g_conv_combine_fwd"]) == 11
    assert len(_lib.CONV_SIGNATURES["x2g_conv_combine_bwd"]) == 17
    import ctypes

    assert _lib.CONV_RESTYPES["x2g_conv_combine_bwd_workspace"] is ctypes.c_size_t
    assert _lib.CONV_RESTYPES["x2g_conv_combine_splits"] is ctypes.c_int32
