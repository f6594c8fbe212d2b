"""x2gnn.init.reference_init_: the reference's reset_parameters rules on every model class (CPU)."""
import math

import pytest
import torch
import torch.nn as nn

SMALL = dict(conv_layers=2, in_channels=32, heads=4, embedding_size=32, rbf_dim=6, sbf_dim=7)


def build(kind):
    import x2gnn

    torch.manual_seed(0)
    if kind == "poly":
        return x2gnn.xgnn_poly(**SMALL)
    if kind == "poly_beta":
        return x2gnn.xgnn_poly(conv_beta=True, **SMALL)
    if kind == "global":
        return x2gnn.xgnn_poly_global(**SMALL)
    if kind == "multi":
        return x2gnn.xgnn_poly_multi(atom_targets=2, mol_targets=2, **SMALL)
    if kind == "v2":
        return x2gnn.xgnn_poly_v2(**SMALL)
    if kind == "trunk":
        return x2gnn.SBFTransformer(conv_layers=2, emb_size=32, sbf_dim=7, rbf_dim=6, in_channels=32, heads=4)
    if kind == "conv":
        return x2gnn.SBFTransformerConv(in_channels=32, out_channels=8, heads=4, sbf_dim=42, rbf_dim=6, edge_dim=32,
                                        beta=True)
    raise AssertionError(kind)


KINDS = ["poly", "poly_beta", "global", "multi", "v2", "trunk", "conv"]


def expected_rule(name):
    """The issue's table, restated from the parameter's name alone."""
    leaf = name.rsplit(".", 1)[1]
    if name.endswith("frequencies"):
        return "untouched"
    if "embedding." in name:
        return "embedding"
    conv_default = ("lin_key.", "lin_query.", "lin_value.", "lin_edge.", "lin_skip.", "lin_beta.")
    if any(k in name for k in conv_default):
        return "default"
    if "mol_readouts." in name and ".mlp." in name:
        return "default"
    return "glorot" if leaf == "weight" else "zero"


@pytest.mark.parametrize("kind", KINDS)
def test_every_parameter_gets_its_rule(kind):
    from x2gnn.init import reference_init_, reference_init_rules

    model = build(kind)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    rules = reference_init_rules(model)
    assert set(rules) == set(before)  # the rules visit every parameter, and nothing else
    is_global = kind == "global"
    for n, rule in rules.items():
        want = expected_rule(n)
        if is_global and ".readouts." in n and ".mlp." in n:
            want = "default"  # xgnn_poly_global's readouts are MolWise
        assert rule == want, n
    assert reference_init_(model, torch.Generator().manual_seed(1)) is model
    seen = {r: 0 for r in ("glorot", "zero", "default", "embedding", "untouched")}
    for n, p in model.named_parameters():
        rule, w = rules[n], p.detach()
        seen[rule] += 1
        if rule == "glorot":
            o, i = w.shape
            gram = (w @ w.T if o <= i else w.T @ w).double()
            diag = float(gram.diagonal().mean())
            assert float((gram - diag * torch.eye(gram.shape[0], dtype=torch.float64)).abs().max()) <= 1e-5 * diag, n
            assert abs(float(w.double().var()) * (o + i) / 2 - 1) <= 1e-5, n
        elif rule == "zero":
            assert bool((w == 0).all()), n
        elif rule == "default":
            fan_in = w.shape[1] if w.dim() == 2 else dict(model.named_parameters())[n[:-4] + "weight"].shape[1]
            assert float(w.abs().max()) <= 1 / math.sqrt(fan_in), n
            assert not torch.equal(w, before[n]), n
        elif rule == "embedding":
            assert bool((w[0] == 0).all()) and not torch.equal(w, before[n])
            assert 0.8 < float(w[1:].std()) < 1.2
        else:
            assert torch.equal(w, before[n]) and n.endswith("frequencies")
            assert torch.equal(w, math.pi * torch.arange(1, w.numel() + 1, dtype=torch.float32))
    assert seen["glorot"] and seen["zero"] and seen["default"]
    if kind not in ("trunk", "conv"):
        assert seen["untouched"] == 1
    if kind not in ("trunk", "conv", "v2"):
        assert seen["embedding"] == 1


def test_the_conv_rows_of_the_table():
    from x2gnn.init import reference_init_rules

    rules = reference_init_rules(build("conv"))
    assert rules == {"lin_key.weight": "default", "lin_key.bias": "default", "lin_query.weight": "default",
                     "lin_query.bias": "default", "lin_value.weight": "default", "lin_value.bias": "default",
                     "lin_edge.weight": "default", "lin_skip.weight": "default", "lin_skip.bias": "default",
                     "lin_beta.weight": "default", "lin_sbf.weight": "glorot", "lin_sbf.bias": "zero",
                     "lin_rbf.weight": "glorot"}


def test_a_parameter_no_rule_names_raises_naming_it():
    from x2gnn.init import reference_init_

    model = build("poly")
    model.fin_model.extra_head = nn.Linear(4, 4)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    with pytest.raises(ValueError, match=r"fin_model\.extra_head\.weight"):
        reference_init_(model)
    for n, p in model.named_parameters():  # raised before anything was written
        assert torch.equal(p, before[n]), n


def test_equal_generator_seeds_give_equal_bits():
    from x2gnn.init import reference_init_

    def state(model, seed):
        m = reference_init_(model, torch.Generator().manual_seed(seed))
        return {k: v.clone() for k, v in m.state_dict().items()}

    models = [build("multi") for _ in range(3)]
    kept = torch.get_rng_state()
    a, b, c = state(models[0], 3), state(models[1], 3), state(models[2], 4)
    assert torch.equal(torch.get_rng_state(), kept)  # every draw came from the generator given
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert any(not torch.equal(a[k], c[k]) for k in a)


def test_without_a_generator_the_draws_are_the_global_generators():
    from x2gnn.init import reference_init_

    torch.manual_seed(11)
    a = reference_init_(build("poly")).state_dict()
    torch.manual_seed(11)
    b = reference_init_(build("poly")).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_exports():
    import x2gnn

    for name in ("reference_init_", "Plateau", "fit"):
        assert name in x2gnn.__all__ and callable(getattr(x2gnn, name))
