"""Attention dropout through the modules and the trainer (xgnn_poly(attn_dropout=...), Trainer): eval is the
undropped model, training draws a new mask per forward from the trunk's (seed, step) state and reproduces it
from the same state, only the staged drop entries run, a captured step advances the state on every replay
and equals the eager step bit for bit, and a checkpoint resumes the mask sequence."""
import pytest
import torch

from test_gpu_model import record_calls

pytestmark = pytest.mark.gpu

CFG = dict(conv_layers=4, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)
P = 0.25
CENTER = ["x2g_sbf_attention_fwd_center_sf", "x2g_sbf_attention_fwd_center_sf_tiled", "x2g_sbf_attention_bwd_center"]


def _batch(cuda, n=4, seed=77):
    from x2gnn.data import collate
    from x2gnn.synth import synthetic_molecules

    return collate(synthetic_molecules(n, "S160", seed=seed)).to(cuda)


def _model(cuda, **kw):
    import x2gnn

    torch.manual_seed(0)
    return x2gnn.xgnn_poly(device="cuda", **CFG, **kw).to(cuda)


def test_eval_is_the_model_without_dropout(cuda):
    b = _batch(cuda)
    plain, drop = _model(cuda), _model(cuda, attn_dropout=P, dropout_seed=3)
    drop.load_state_dict(plain.state_dict())
    plain.eval()
    drop.eval()
    with torch.no_grad():
        e0, e1 = plain(b), drop(b)
    assert torch.equal(e0, e1)
    assert drop.fin_model.attn_dropout_state.tolist() == [3, 0]  # eval never touches the state


def test_training_forwards_draw_new_masks_and_reproduce_from_the_state(cuda, monkeypatch):
    b = _batch(cuda)
    m = _model(cuda, attn_dropout=P, dropout_seed=3)
    m.train()
    with torch.no_grad():
        m(b)  # (the first forward applies the embedding's max_norm renorm)
    st = m.fin_model.attn_dropout_state
    held = st.clone()
    seen = record_calls(monkeypatch)
    e1 = m(b)
    torch.nn.functional.smooth_l1_loss(e1, b.y).backward()
    g1 = [p.grad.clone() for p in m.parameters() if p.grad is not None]
    names = [n for n, _ in seen]
    # the three drop entries and none of their parents (4 layers: one untiled forward and one backward each)
    assert names.count("x2g_sbf_attention_fwd_center_sf_drop") == 4
    assert names.count("x2g_sbf_attention_bwd_center_drop") == 4
    assert not any(n in CENTER for n in names)
    assert all(n.endswith("_drop") for n in names if "attention" in n)
    salts = [a[-1] for n, a in seen if n == "x2g_sbf_attention_fwd_center_sf_drop"]
    assert salts == [0, 1, 2, 3]
    assert [a[-1] for n, a in seen if n == "x2g_sbf_attention_bwd_center_drop"] == [3, 2, 1, 0]
    assert st.tolist() == [3, int(held[1]) + 1]
    e2 = m(b).detach()
    assert not torch.equal(e1.detach(), e2)
    assert st.tolist() == [3, int(held[1]) + 2]
    st.copy_(held)
    m.zero_grad(set_to_none=True)
    e3 = m(b)
    torch.nn.functional.smooth_l1_loss(e3, b.y).backward()
    assert torch.equal(e3.detach(), e1.detach())
    g3 = [p.grad for p in m.parameters() if p.grad is not None]
    assert len(g1) == len(g3) and all(torch.equal(a, c) for a, c in zip(g1, g3))
    # and the dropped model is not the undropped one
    plain = _model(cuda)
    plain.load_state_dict(m.state_dict())
    plain.train()
    assert not torch.equal(plain(b).detach(), e1.detach())


def test_training_under_no_grad_runs_the_drop_forward_only(cuda, monkeypatch):
    b = _batch(cuda)
    m = _model(cuda, attn_dropout=P)
    m.train()
    seen = record_calls(monkeypatch)
    with torch.no_grad():
        m(b)
    names = [n for n, _ in seen]
    assert names.count("x2g_sbf_attention_fwd_center_sf_drop") == 4 and not any(n in CENTER for n in names)
    fwd = [a for n, a in seen if n == "x2g_sbf_attention_fwd_center_sf_drop"]
    assert all(a[-5] is None and a[-6] is None for a in fwd)  # no P rows, no S rows kept


def _trainer(cuda, **kw):
    from x2gnn.train import Trainer

    return Trainer(_model(cuda, attn_dropout=P, dropout_seed=11, **kw))


def _warm(tr, batch, n=3):
    """The forwards a capture's warm-up makes (each applies the max_norm renorm), the mask state left alone."""
    st = tr.model.fin_model.attn_dropout_state
    held = st.clone()
    for _ in range(n):
        tr.forward_backward(batch)
    st.copy_(held)


def test_captured_steps_equal_eager_steps_and_a_checkpoint_resumes(cuda):
    batch = _batch(cuda)
    eager, graphed = _trainer(cuda), _trainer(cuda)
    _warm(eager, batch)
    graphed.capture(batch, warm=3)
    assert graphed.model.fin_model.attn_dropout_state.tolist() == [11, 0]  # the warm-up's masks are not steps
    le, lg, saved = [], [], None
    for i in range(3):
        le.append(eager.step(batch).detach().clone())
        lg.append(graphed.step(batch).detach().clone())
        if i == 1:
            saved = eager.state_dict()
    torch.cuda.synchronize()
    assert eager.model.fin_model.attn_dropout_state.tolist() == [11, 3]
    assert graphed.model.fin_model.attn_dropout_state.tolist() == [11, 3]  # every replay advanced it
    assert all(torch.equal(a, b) for a, b in zip(le, lg))
    assert len({float(v) for v in le}) == 3
    assert torch.equal(eager.opt.flat, graphed.opt.flat)
    assert torch.equal(eager.opt.ema, graphed.opt.ema)
    # save after step 2, load into a fresh trainer: its step 3 is the uninterrupted run's
    assert saved["attn_dropout_state"].tolist() == [11, 2]
    fresh = _trainer(cuda)
    _warm(fresh, batch)
    addr = fresh.model.fin_model.attn_dropout_state.data_ptr()
    fresh.load_state_dict(saved)
    assert fresh.model.fin_model.attn_dropout_state.data_ptr() == addr  # copied into the existing buffer
    l3 = fresh.step(batch).detach()
    assert torch.equal(l3, le[2])
    assert torch.equal(fresh.opt.flat, eager.opt.flat)
    # a model without dropout neither writes nor wants the key
    from x2gnn.train import Trainer

    plain = Trainer(_model(cuda))
    assert "attn_dropout_state" not in plain.state_dict()
    with pytest.raises(KeyError, match="attn_dropout_state"):
        fresh.load_state_dict(plain.state_dict())


def test_drop_in_conv_with_per_triplet_edge_attr_raises_in_training_only(cuda):
    """SBFTransformerConv through the reference's forward(sbf, rbf, x, edge_index, edge_attr) with per-triplet
    edge attributes: no dropout kernel covers that route, so training raises and eval runs."""
    import numpy as np

    from oracle import triplets
    from x2gnn.sbftransformer_conv import SBFTransformerConv

    import attention_ref as ar

    ei, n = ar.edge_case_graph(6)
    trip = triplets.vertex_to_edge(ei, n)[0]
    E, T = ei.shape[1], trip.shape[1]
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    conv = SBFTransformerConv(128, 8, heads=16, sbf_dim=42, rbf_dim=6, dropout=0.2, edge_dim=32).to(cuda)
    sbf, rbf, x, ea = (torch.randn(*s, generator=g).to(cuda) for s in ((T, 42), (E, 6), (E, 128), (T, 32)))
    edge_index = torch.from_numpy(np.ascontiguousarray(trip)).to(cuda)
    conv.train()
    with pytest.raises(NotImplementedError, match="per-triplet"):
        conv(sbf, rbf, x, edge_index, ea)
    conv.eval()
    out = conv(sbf, rbf, x, edge_index, ea)
    assert out.shape == (E, 128) and bool(torch.isfinite(out).all())
