"""SBFTransformerConv's ``beta=True`` / ``concat=False`` at module and model level.

Module level: the conv against a torch-float64 statement, tests/attention_ref.attention_ref for the attention and
the reference's four lines (sbftransformer_conv.py:115-127) after it, on attention_ref.edge_case_graph(40) and the
small molecular graph of tests/test_gpu_attention_fp64.py.  The attention part (the tensor the combine pass
receives, and every end-to-end gradient) keeps that file's bound (its ``_Checker``: max(8 e32, floor), capped at
1e-4 of scale); the combine part (y, d_attn, d_xr, dw_beta from the float32 operands the pass actually received)
keeps conv_combine_ref's unit bound.

Model level: a two-layer xgnn_poly(conv_beta=True) on the molecules of tests/device_dataset_cases.py.
"""
import numpy as np
import pytest
import torch

import attention_ref as ar
import conv_combine_ref as cr
from device_dataset_cases import mixed_molecules
from test_gpu_attention_fp64 import EDGE_NONE, EDGE_PER_DST, TABLE_ROWS, _Checker, _graph, _inputs, _line_graph
from test_gpu_model import record_calls

pytestmark = pytest.mark.gpu

H, C, DIN = 16, 8, 128
OPTIONS = [(True, True), (False, False), (True, False)]  # (beta, concat)
CFG = dict(conv_layers=2, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)


def _conv(cuda, beta, concat):
    from x2gnn.sbftransformer_conv import SBFTransformerConv

    torch.manual_seed(5)
    return SBFTransformerConv(DIN, C, heads=H, sbf_dim=42, rbf_dim=6, concat=concat, beta=beta).to(cuda)


def _case_inputs(gname):
    """The attention test's seeded inputs of the graph plus the module's own: feat [E, 128], rbf [E, 6], dy."""
    g, x = _graph(gname), dict(_inputs(gname, "unit", H, C))
    gen = torch.Generator().manual_seed(977 + g.E)
    x["feat"], x["rbf"] = torch.randn(g.E, DIN, generator=gen), torch.randn(g.E, 6, generator=gen)
    x["dy"] = torch.randn(g.E, H * C, generator=gen)
    return g, x


def _statement(P, g, x, mode, beta, concat, dtype):
    """The conv in ``dtype`` on the CPU: the five projections, attention_ref with a zero skip, the four lines; every
    gradient by autograd (the attention's through attention_ref's own)."""
    leaf = lambda t: t.detach().cpu().to(dtype).clone().requires_grad_(True)  # noqa: E731
    L = {n: leaf(t) for n, t in P.items()}
    feat, rbf = leaf(x["feat"]), leaf(x["rbf"])
    src, dst = torch.from_numpy(g.trip[0]), torch.from_numpy(g.trip[1])
    row_dst = torch.from_numpy(g.row_dst)
    lin = lambda n, t: t @ L[n + ".weight"].t() + (L[n + ".bias"] if n + ".bias" in L else 0)  # noqa: E731
    x_src = feat * (rbf @ L["lin_rbf.weight"].t())
    q, k, v, x_r = lin("lin_query", feat), lin("lin_key", x_src), lin("lin_value", x_src), lin("lin_skip", feat)
    if mode == EDGE_PER_DST:  # the fused forward forms radial[src] * Y itself: the unrounded product
        sbf = ar.sbf_from_factors(x["radial"].to(dtype), x["y"].to(dtype), src)
        table = leaf(x["table"])
        e_t = table[row_dst[dst]]
    else:
        sbf, table, e_t = x["sbf"].to(dtype), None, None
    att = dict(S=None, trip_src=src, trip_dst=dst, heads=H, channels=C, dtype=dtype,
               lin=(sbf, L["lin_sbf.weight"], L["lin_sbf.bias"]))
    zero = torch.zeros(g.E, H * C, dtype=dtype)
    r = ar.attention_ref(q, k, v, zero, e_t=e_t, **att)
    attn = r["out"].clone().requires_grad_(True)
    out = attn.view(-1, H, C)
    out = out.reshape(-1, H * C) if concat else out.mean(dim=1)
    if beta:
        b = torch.sigmoid(torch.cat([out, x_r, out - x_r], dim=-1) @ L["lin_beta.weight"].t())
        y = b * x_r + (1 - b) * out
    else:
        y = out + x_r
    dy = x["dy"][:, :y.shape[1]].to(dtype)
    y.backward(dy)
    r2 = ar.attention_ref(q, k, v, zero, e_t=e_t, dout=attn.grad, **att)
    torch.autograd.backward([q, k, v], [r2["dq"], r2["dk"], r2["dv"]])
    res = dict(out=r["out"], y=y.detach(), d_feat=feat.grad, d_rbf=rbf.grad)
    res.update({"d_" + n: t.grad for n, t in L.items() if not n.startswith("lin_sbf")})
    res["d_lin_sbf.weight"], res["d_lin_sbf.bias"] = r2["dW"], r2["db"]
    res["_dk_abs"] = r2["dk"].abs().sum(0)  # (not an output: the magnitude of the terms d_lin_key.bias sums)
    if table is not None:
        res["d_table"] = ar.rows_sum(ar.rows_sum(r2["de_t"], dst, g.E), row_dst, TABLE_ROWS)
    return res


def _run_conv(conv, lg, g, x, mode, cuda, monkeypatch):
    """The module's forward and backward; returns its outputs, gradients and what ops.conv_combine received."""
    from x2gnn import ops

    seen, inner = {}, ops.conv_combine

    def spy(attn, x_r, w_beta, heads, channels, concat):
        y = inner(attn, x_r, w_beta, heads, channels, concat)
        seen.update(attn=attn, x_r=x_r, y=y)
        attn.register_hook(lambda gr: seen.__setitem__("d_attn", gr))
        x_r.register_hook(lambda gr: seen.__setitem__("d_xr", gr))
        return y

    monkeypatch.setattr(ops, "conv_combine", spy)
    feat, rbf = x["feat"].to(cuda).requires_grad_(True), x["rbf"].to(cuda).requires_grad_(True)
    table = None
    if mode == EDGE_PER_DST:
        sbf = x["sbf"].to(cuda)
        lg.sbf_factors = (sbf, x["radial"].to(cuda), x["y"].to(cuda))
        table = x["table"].to(cuda).requires_grad_(True)
        y = conv(sbf, rbf, feat, None, line_graph=lg, edge_row=lg.dst_type, edge_proj=table)
    else:
        y = conv(x["sbf"].to(cuda), rbf, feat, None, line_graph=lg)
    dy = x["dy"][:, :y.shape[1]].contiguous().to(cuda)
    conv.zero_grad(set_to_none=True)
    y.backward(dy)
    got = dict(out=seen["attn"], y=y.detach(), d_feat=feat.grad, d_rbf=rbf.grad)
    got.update({"d_" + n: p.grad for n, p in conv.named_parameters()})
    if table is not None:
        got["d_table"] = table.grad
    return got, seen, dy


def _check_conv(name, conv, got, seen, dy, refs, mode, beta, concat):
    ck = _Checker(name, "unit", H, C)
    for n in refs[0]:
        if not n.startswith("_") and n != "d_lin_key.bias":
            ck.check(f"SBFTransformerConv[beta={beta}, concat={concat}]", mode, refs, n, got[n])
    ck.done()
    # lin_key's bias shifts every logit of a (destination, head) alike, so its exact gradient is 0 (the column sums of
    # dk cancel) and no relative error exists: the checker's cap, 1e-4, of the magnitude of the terms summed instead
    assert float(got["d_lin_key.bias"].abs().max()) <= 1e-4 * float(refs[0]["_dk_abs"].max())
    # the combine pass on the float32 operands it received
    npf = lambda t: t.detach().cpu().numpy()  # noqa: E731
    w = npf(conv.lin_beta.weight).reshape(-1) if beta else None
    fwd = cr.combine_fwd(npf(seen["attn"]), npf(seen["x_r"]), w, H, C, concat)
    bwd = cr.combine_bwd(npf(dy), npf(seen["attn"]), npf(seen["x_r"]), w, H, C, concat)
    figures = dict(y=cr.ratio(npf(seen["y"]), *fwd["y"]) / cr.K["fwd"],
                   d_attn=cr.ratio(npf(seen["d_attn"]), *bwd["d_attn"]) / cr.K["bwd"],
                   d_xr=cr.ratio(npf(seen["d_xr"]), *bwd["d_xr"]) / cr.K["bwd"])
    if beta:
        figures["dw_beta"] = cr.ratio(npf(conv.lin_beta.weight.grad).reshape(-1), *bwd["dw"]) / cr.K["dw"]
    stats = getattr(seen["y"], "_x2g_rowstats", None)
    assert (stats is not None) == concat  # Dout = 128 carries the row statistics, Dout = 8 does not
    if stats is not None:
        figures["row_stats"] = cr.ratio(npf(stats), *fwd["stats"]) / cr.K["stats"]
    print(name, beta, concat, {k: round(v, 3) for k, v in figures.items()})
    assert all(v <= 1.0 for v in figures.values()), figures


@pytest.mark.parametrize("beta,concat", OPTIONS)
@pytest.mark.parametrize("gname", ["edge", "mol"])
def test_conv_against_float64(cuda, monkeypatch, gname, beta, concat):
    from x2gnn.plan import GraphPlan

    g, x = _case_inputs(gname)
    conv = _conv(cuda, beta, concat)
    assert tuple(conv.lin_skip.weight.shape) == (H * C if concat else C, DIN) and (conv.lin_beta is not None) == beta
    if gname == "mol":
        lg, mode = GraphPlan.from_atom_batch(g.batch.to(cuda)).lg, EDGE_PER_DST
    else:
        lg, mode = _line_graph(g, cuda), EDGE_NONE
    P = dict(conv.named_parameters())
    refs = tuple(_statement(P, g, x, mode, beta, concat, dt) for dt in (torch.float64, torch.float32))
    got, seen, dy = _run_conv(conv, lg, g, x, mode, cuda, monkeypatch)
    _check_conv(gname, conv, got, seen, dy, refs, mode, beta, concat)


def test_combine_follows_either_attention_route(cuda, monkeypatch):
    """The same conv on the center route and with ops._CENTER off: both within the bounds of the one reference
    (which attention kernels ran is read from the calls); the combine pass is launched once each way either time."""
    from x2gnn import ops
    from x2gnn.plan import GraphPlan

    g, x = _case_inputs("mol")
    conv = _conv(cuda, True, True)
    P = dict(conv.named_parameters())
    refs = tuple(_statement(P, g, x, EDGE_PER_DST, True, True, dt) for dt in (torch.float64, torch.float32))
    for center in (True, False):
        with monkeypatch.context() as mp:
            mp.setattr(ops, "_CENTER", center)
            calls = record_calls(mp)
            lg = GraphPlan.from_atom_batch(g.batch.to(cuda)).lg
            got, seen, dy = _run_conv(conv, lg, g, x, EDGE_PER_DST, cuda, mp)
            names = [n for n, _ in calls]
            assert any("center" in n for n in names) == center
            assert names.count("x2g_conv_combine_fwd") == 1 and names.count("x2g_conv_combine_bwd") == 1
            assert names.index("x2g_conv_combine_fwd") > max(i for i, n in enumerate(names) if "attention_fwd" in n)
            _check_conv(f"mol[center={center}]", conv, got, seen, dy, refs, EDGE_PER_DST, True, True)


# ------------------------------------------------------------------------------------------------ model level
def _batch(cuda):
    from x2gnn.data import collate

    return collate(mixed_molecules()).to(cuda)


def _model(cuda, **kw):
    import x2gnn

    torch.manual_seed(0)
    return x2gnn.xgnn_poly(device="cuda", **CFG, **kw).to(cuda)


def _fwd_bwd(m, b):
    m.zero_grad(set_to_none=True)
    e = m(b)
    torch.nn.functional.smooth_l1_loss(e, b.y).backward()
    torch.cuda.synchronize()
    return e.detach().clone(), [None if p.grad is None else p.grad.detach().clone() for p in m.parameters()]


def test_model_fused_layernorm_equals_separate(cuda, monkeypatch):
    """ops._LN_FUSE on (the combine pass' row statistics feed x2g_chain_fwd_ln) and off: energies and gradients as
    test_gpu_model.test_fused_variants_equal_separate demands of the existing model."""
    from x2gnn import ops

    b, m = _batch(cuda), _model(cuda, conv_beta=True)
    outs = []
    for on in (True, False):
        monkeypatch.setattr(ops, "_LN_FUSE", on)
        calls = record_calls(monkeypatch)
        outs.append(_fwd_bwd(m, b))
        names = [n for n, _ in calls]
        assert names.count("x2g_conv_combine_fwd") == 2 and names.count("x2g_conv_combine_bwd") == 2
        assert ("x2g_chain_fwd_ln" in names) == on
        stats = [a[9] for n, a in calls if n == "x2g_conv_combine_fwd"]
        assert all((s is not None) == on for s in stats)
    torch.testing.assert_close(outs[0][0], outs[1][0], rtol=1e-5, atol=1e-6)
    top = max(float(g.abs().max()) for g in outs[1][1] if g is not None)
    assert all(g is not None for n, g in zip(dict(m.named_parameters()), outs[0][1]) if n.endswith("lin_beta.weight"))
    for a, c in zip(outs[0][1], outs[1][1]):
        if c is None:
            assert a is None
            continue
        torch.testing.assert_close(a, c, rtol=1e-4, atol=1e-5 * top)


def test_model_captured_steps_equal_eager_steps(cuda):
    from x2gnn.train import Trainer

    b = _batch(cuda)
    eager, graphed = Trainer(_model(cuda, conv_beta=True)), Trainer(_model(cuda, conv_beta=True))
    for _ in range(3):
        eager.forward_backward(b)
    graphed.capture(b, warm=3)
    le, lg = [], []
    for _ in range(3):
        le.append(eager.step(b).detach().clone())
        lg.append(graphed.step(b).detach().clone())
    torch.cuda.synchronize()
    assert all(torch.equal(a, c) for a, c in zip(le, lg))
    assert len({float(v) for v in le}) == 3
    assert torch.equal(eager.opt.flat, graphed.opt.flat)
    assert torch.equal(eager.opt.ema, graphed.opt.ema)


def test_model_state_dict_round_trips(cuda):
    b = _batch(cuda)
    a, c = _model(cuda, conv_beta=True), _model(cuda, conv_beta=True)
    with torch.no_grad():
        for p in a.parameters():
            p.add_(0.01 * torch.randn_like(p))
    sd = a.state_dict()
    assert sum(k.endswith("lin_beta.weight") for k in sd) == 2
    assert all(tuple(v.shape) == (1, 384) for k, v in sd.items() if k.endswith("lin_beta.weight"))
    res = c.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    a.eval(), c.eval()
    with torch.no_grad():
        assert torch.equal(a(b), c(b))
    with pytest.raises(RuntimeError, match="lin_beta"):
        _model(cuda).load_state_dict(sd)


def test_default_model_never_calls_the_combine_pass(cuda, monkeypatch):
    b, m = _batch(cuda), _model(cuda, conv_beta=False)
    calls = record_calls(monkeypatch)
    _fwd_bwd(m, b)
    names = [n for n, _ in calls]
    assert names and not any(n.startswith("x2g_conv_combine") for n in names)
    assert not any(k.endswith("lin_beta.weight") for k in m.state_dict())
