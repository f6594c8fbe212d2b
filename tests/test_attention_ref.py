"""The fp64 attention reference (tests/attention_ref.py) made trustworthy on the CPU: equal to the oracle's
SBFTransformerConv in float64 and to the reference implementation's stored fp32 outputs (conv1.npz), its
derived backward quantities equal to autograd, and a destination without triplets handled."""
import math

import numpy as np
import pytest
import torch

from attention_ref import (attention_ref, edge_case_graph, fold_g, make_inputs, p_rows, project, rows_sum,
                           s_from_p, sbf_from_factors, wgrad_from_g)
from conftest import golden
from helpers import rel_err

from oracle import ref_cpu, triplets


def test_reference_equals_oracle_conv_fp64_and_golden():
    """On conv1.npz (D=128, H=16, C=8, per-triplet edge term) the reference fed the oracle's own q / k / v /
    skip / e / S projections gives the oracle's float64 output within 1e-12 of scale, and its autograd
    gradients dq, dk, dv, dskip, dS, de_t pushed through those projections give the oracle's parameter
    gradients, grad_x and grad_edge_attr; and all of it equals the stored fp32 golden at the tolerances of
    test_conv_layer_vs_reference (1e-5 forward, 1e-4 gradients)."""
    from weights import load_seeded

    z = golden("conv1.npz")
    conv = ref_cpu.SBFTransformerConv(128, 16, 42, 6, 128)
    load_seeded(conv, int(z["weight_seed"]))
    conv = conv.double()
    f64 = lambda name: torch.from_numpy(z[name]).double()  # noqa: E731
    x, ea = f64("conv_x").requires_grad_(True), f64("conv_edge_attr").requires_grad_(True)
    sbf, rbf, up = f64("sbf"), f64("rbf"), f64("upstream")
    trip = torch.from_numpy(z["trip"].astype(np.int64))
    # the oracle itself, float64
    out_o = conv(sbf, rbf, x, trip, ea)
    params = dict(conv.named_parameters())
    leaves = [x, ea] + list(params.values())
    grads_o = torch.autograd.grad(out_o, leaves, up, allow_unused=True)
    # the reference on the oracle's projections
    x_src = x * conv.lin_rbf(rbf)
    proj = dict(q=conv.lin_query(x), k=conv.lin_key(x_src), v=conv.lin_value(x_src), skip=conv.lin_skip(x),
                e=conv.lin_edge(ea), S=conv.lin_sbf(sbf))
    r = attention_ref(proj["q"], proj["k"], proj["v"], proj["skip"], proj["S"], trip[0], trip[1], 16, 8,
                      e_t=proj["e"], dout=up)
    assert r["out"].dtype == torch.float64
    assert rel_err(r["out"].numpy(), out_o.detach().numpy()) < 1e-12
    order = ("q", "k", "v", "skip", "e", "S")
    up_grads = [r["dq"], r["dk"], r["dv"], r["dskip"], r["de_t"], r["dS"]]
    grads_r = torch.autograd.grad([proj[n] for n in order], leaves, up_grads, allow_unused=True)
    names = ["grad_x", "grad_edge_attr"] + ["grad." + n for n in params]
    # lin_key.bias has no gradient analytically (the softmax is shift invariant): rounding noise on both
    # sides, so the absolute slack is 1e-12 of the largest gradient, as test_model_vs_reference scales it
    gmax = max(float(b.abs().max()) for b in grads_o if b is not None)
    for name, a, b in zip(names, grads_r, grads_o):
        assert (a is None) == (b is None), name
        if a is not None:
            assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()) + 1e-12 * gmax, name
    # and the reference implementation's own fp32 results
    assert rel_err(r["out"].numpy(), z["out"]) < 1e-5
    assert rel_err(grads_r[0].numpy(), z["grad_x"]) < 1e-4
    assert rel_err(grads_r[1].numpy(), z["grad_edge_attr"]) < 1e-4


def _edge_graph_case(heads, channels, seed):
    ei, n = edge_case_graph(hub=12)
    trip = triplets.vertex_to_edge(ei, n)[0]
    E, T, D = ei.shape[1], trip.shape[1], heads * channels
    x = {k: v.double() for k, v in make_inputs("unit", E, T, D, seed).items()}
    return ei, n, trip, E, T, D, x


@pytest.mark.parametrize("heads,channels", [(16, 8), (8, 16), (32, 4), (4, 8)])
def test_derived_quantities_equal_autograd(heads, channels):
    """With sbf = radial[src] (x) Y: the weight gradient folded from G (sum_s radial[s, 6l+n] G[s, l, c]) and
    sum_s G[s, 7, :] equal the autograd gradients of a torch.nn.Linear(42, HC) applied to that sbf; dlogit =
    a (g - rho); S rebuilt from the P rows equals W sbf + b; the per-destination / per-atom / per-row edge
    gradients are sums of the per-triplet one and agree with the gradient of the table itself."""
    ei, n, trip, E, T, D, x = _edge_graph_case(heads, channels, 7 + heads)
    src, dst = torch.from_numpy(trip[0]), torch.from_numpy(trip[1])
    z = torch.randint(0, 10, (n,), generator=torch.Generator().manual_seed(1))
    row_dst = z[torch.from_numpy(ei[1])]  # the element of each destination's middle atom
    sbf = sbf_from_factors(x["radial"], x["y"], src)
    lin = torch.nn.Linear(42, D).double()
    with torch.no_grad():
        lin.weight.copy_(x["W"])
        lin.bias.copy_(x["b"])
    table = x["table"].clone().requires_grad_(True)
    e_t = table[row_dst[dst]]
    S = lin(sbf)
    r = attention_ref(x["q"], x["k"], x["v"], x["skip"], S, src, dst, heads, channels, e_t=e_t, dout=x["dout"])
    # autograd through lin_sbf and the table lookup, from the reference's dS and de_t
    dW, db, dtable = torch.autograd.grad([S, e_t], [lin.weight, lin.bias, table], [r["dS"], r["de_t"]])
    G = fold_g(r["dS"], x["y"], src, E)
    assert G.shape == (E, 8, D)
    dW_g, db_g = wgrad_from_g(G, x["radial"])
    assert rel_err(dW_g.numpy(), dW.numpy()) < 1e-12 and rel_err(db_g.numpy(), db.numpy()) < 1e-12
    # the same through the reference's own lin form
    r2 = attention_ref(x["q"], x["k"], x["v"], x["skip"], None, src, dst, heads, channels, e_t=e_t.detach(),
                       dout=x["dout"], lin=(sbf, x["W"], x["b"]))
    assert rel_err(r2["out"].numpy(), r["out"].numpy()) < 1e-13
    assert rel_err(r2["dW"].numpy(), dW.numpy()) < 1e-12 and rel_err(r2["db"].numpy(), db.numpy()) < 1e-12
    # dlogit = a (g - rho), rho per destination
    want = r["prob"] * (r["g"] - r["seg_rho"][dst])
    assert rel_err(r["dlogit"].numpy(), want.numpy()) < 1e-12
    # S from the P rows
    P = p_rows(x["W"], x["radial"])
    assert P.shape == (E, 7, D)
    assert rel_err(s_from_p(P, x["b"], x["y"], src).numpy(), project(sbf, x["W"], x["b"]).numpy()) < 1e-13
    # edge gradients: per destination -> per table row == per center atom -> per element == autograd's
    center = torch.from_numpy(ei[1])[dst]
    assert torch.equal(center, torch.from_numpy(ei[0])[src])  # the triplets through atom b: src leaves b, dst enters b
    d_dst = rows_sum(r["de_t"], dst, E)
    d_atom = rows_sum(r["de_t"], center, n)
    assert rel_err(rows_sum(d_dst, row_dst, 10).numpy(), dtable.numpy()) < 1e-12
    assert rel_err(rows_sum(d_atom, z, 10).numpy(), dtable.numpy()) < 1e-12
    # probabilities and row statistics are what they say
    assert rel_err(rows_sum(r["prob"], dst, E)[r["seg_den"][:, 0] > 0].numpy(), 1.0) < 1e-12
    assert rel_err(r["row_stats"][:, 0].numpy(), r["out"].mean(1).numpy()) < 1e-13
    assert rel_err(r["row_stats"][:, 1].numpy(), (r["out"].var(1, unbiased=False) * D).numpy()) < 1e-12


@pytest.mark.parametrize("regime", ["peaked", "offset"])
def test_large_logits_are_finite_and_well_conditioned(regime):
    """The regimes the kernels are run in: logits beyond the fp32 exp range without the max shift, and the
    float32 evaluation of the reference stays within 1.25e-5 of every output's scale (so 8 x that is below
    the 1e-4 the GPU tests allow a bound to reach)."""
    ei, n, trip, E, T, D, _ = _edge_graph_case(16, 8, 0)
    x = make_inputs(regime, E, T, D, 3)
    src, dst = trip[0], trip[1]
    r64, r32 = (attention_ref(x["q"], x["k"], x["v"], x["skip"], x["S"], src, dst, 16, 8, e_t=x["e_trip"],
                              dout=x["dout"], dtype=dt) for dt in (torch.float64, torch.float32))
    assert float(r64["logits"].abs().max()) > 100.0
    if regime == "offset":
        assert float(r64["seg_max"][r64["seg_den"] > 0].min()) < -88.0  # whole segments far negative
    for name in ("out", "dq", "dk", "dv", "dS", "de_t"):
        assert torch.isfinite(r64[name]).all() and r32[name].dtype == torch.float32
        assert rel_err(r32[name].numpy(), r64[name].numpy()) < 1.25e-5, name


def test_destination_without_triplets():
    """A destination no triplet enters: out = skip, max -inf, denominator 0, zero gradients, nothing NaN."""
    E, H, C = 4, 4, 8
    x = make_inputs("unit", E, 3, H * C, 5)
    src, dst = torch.tensor([0, 1, 3]), torch.tensor([1, 1, 3])  # destinations 0 and 2 are empty
    r = attention_ref(x["q"], x["k"], x["v"], x["skip"], x["S"], src, dst, H, C, e_t=x["e_trip"], dout=x["dout"])
    for name, t in r.items():
        if name != "seg_max":
            assert not torch.isnan(t).any(), name
    for d in (0, 2):
        assert torch.equal(r["out"][d], x["skip"][d].double())
        assert bool((r["seg_max"][d] == -math.inf).all()) and float(r["seg_den"][d].abs().max()) == 0.0
        assert float(r["dq"][d].abs().max()) == 0.0
        assert float(r["seg_rho"][d].abs().max()) == 0.0
    assert float(r["dk"][2].abs().max()) == 0.0 and float(r["dv"][2].abs().max()) == 0.0  # not a source either
    assert torch.equal(r["dskip"], x["dout"].double())
    assert torch.isfinite(r["seg_max"][[1, 3]]).all()
    # a destination with a single triplet: probability 1 / (1 + 1e-16), dlogit 0
    assert float((r["prob"][2] - 1.0).abs().max()) < 1e-15 and float(r["dlogit"][2].abs().max()) < 1e-12
