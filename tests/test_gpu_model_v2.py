"""xgnn_poly_v2 / SBFTransformerV2 on the GPU against the reference's own SBFTransformerV2 (tests/golden/model_v2.npz,
written by running it: tests/golden/make_v2_golden.py): energies and gradients through the shipped route (the atom
context fused, one table row per center atom in the center attention kernels) and through the destination-major
route, every slower path against the same bounds, the in-place gradient fan-in, the captured training step, and a
batch with an atom that has no neighbour.

Tolerances are the project's own, imported from test_gpu_model: ENERGY_RTOL and the gradient rule of
check_vs_fixture (its embedding check compares nothing here: V2 has no embedding)."""
import types

import numpy as np
import pytest
import torch

from conftest import golden
from helpers import batch_from_fixture, energy_rel_err, model_cfg
from test_gpu_model import ENERGY_RTOL, check_vs_fixture, record_calls
from weights import load_seeded

pytestmark = pytest.mark.gpu

EDGE_PER_TRIPLET, EDGE_PER_DST = 1, 2


class _NoEmbedding:
    """check_vs_fixture's model and fixture arguments for a model without ``emb_block``: its embedding check then
    compares one constant with itself, and everything else is the model's and the fixture's own."""

    def __init__(self, inner):
        self._inner = inner
        self.emb_block = types.SimpleNamespace(embedding=types.SimpleNamespace(weight=torch.zeros(1)))
        self.files = getattr(inner, "files", None)

    def named_parameters(self):
        return self._inner.named_parameters()

    def __getitem__(self, key):
        return np.zeros(1, np.float32) if key == "emb_after" else self._inner[key]


def _check(m, z, res, y):
    checked = check_vs_fixture(_NoEmbedding(m), _NoEmbedding(z), res, y)
    assert checked == sum(k.startswith("grad.") for k in z.files) >= 5
    for n in ("fin_model.edgenn.1.0.weight", "fin_model.convs.1.lin_edge.weight", "fin_model.convs.0.lin_sbf.bias"):
        assert "grad." + n in z.files


def _model(z, cuda):
    import x2gnn

    m = x2gnn.xgnn_poly_v2(device="cuda", **model_cfg(z))
    load_seeded(m, int(z["weight_seed"]))
    return m.to(cuda)


@pytest.mark.parametrize("path", ["shipped", "dst_major"])
def test_fixture_through_both_routes(cuda, monkeypatch, path):
    z = golden("model_v2.npz")
    m = _model(z, cuda)
    b = batch_from_fixture(z, shipped=path == "shipped").to(cuda)
    seen = record_calls(monkeypatch)
    res = m(b)
    _check(m, z, res, b.y)
    names = [n for n, _ in seen]
    layers = model_cfg(z)["conv_layers"]
    assert not any(n.startswith("x2g_keyed_row_sum") or n.startswith("x2g_table_chain") for n in names)
    attn = [(n, a) for n, a in seen if n.startswith("x2g_sbf_attention_")]
    # no T-row gather of the edge term on either route: every attention call reads one row per destination
    modes = [a[6] for n, a in attn if n.startswith("x2g_sbf_attention_fwd")]
    modes += [a[5] for n, a in attn if n in ("x2g_sbf_attention_bwd_center", "x2g_sbf_attention_bwd_dst")]
    assert len(modes) == 2 * layers and modes == [EDGE_PER_DST] * len(modes) and EDGE_PER_TRIPLET not in modes
    if path == "shipped":
        assert names.count("x2g_atom_context_fwd") == layers and names.count("x2g_atom_context_bwd") == layers
        fwd = [a for n, a in attn if n == "x2g_sbf_attention_fwd_center_sf"]
        bwd = [a for n, a in attn if n == "x2g_sbf_attention_bwd_center"]
        assert len(fwd) == len(bwd) == layers and len(attn) == 2 * layers
        assert all(a[4] and a[5] and a[15] and a[16] for a in fwd)  # the table, src_row, packs, the atom info
        assert all(a[28] for a in bwd)  # d_edge_atom: the table's gradient itself
        n_atoms = int(b.x.shape[0])
        assert all(a[18] == n_atoms for a in bwd)
    else:
        assert not any(n.startswith("x2g_sbf_attention_fwd_center") or n == "x2g_sbf_attention_bwd_center"
                       for n in names)
        assert names.count("x2g_sbf_attention_bwd_dst") == layers  # the plain two-pass backward, not the fold passes
        assert "x2g_sbf_attention_bwd_src_fold" not in names and "x2g_sbf_attention_bwd_dst_g" not in names
        assert names.count("x2g_segment_reduce_perm") >= layers  # d_edge [E, HC] summed by target atom
        assert names.count("x2g_atom_context_fwd") == layers


@pytest.mark.parametrize("variant", ["_ATOM_CTX", "_CENTER", "literal"])
def test_slower_paths_within_the_same_bounds(cuda, monkeypatch, variant):
    """The composition segment_sum -> row_chain (ops._ATOM_CTX = False), the destination-major attention
    (ops._CENTER = False) and the literal form (no ``edge_atom_row``: pool, gather, edgenn and lin_edge on T rows,
    EDGE_PER_TRIPLET) against the fixture, with the bounds of the fast path."""
    from x2gnn import ops

    z = golden("model_v2.npz")
    m = _model(z, cuda)
    b = batch_from_fixture(z).to(cuda)
    if variant != "literal":
        monkeypatch.setattr(ops, variant, False)
    seen = record_calls(monkeypatch)
    if variant == "literal":
        line, plan = m.line_graph_data(b, lazy_sbf=ops.LAZY_SBF)
        del line._store["edge_atom_row"]
        res = m.fin_model(line, edge_index_0=plan.lg.edge_src, atom_batch=b.batch)
    else:
        res = m(b)
    _check(m, z, res, b.y)
    names = [n for n, _ in seen]
    layers = model_cfg(z)["conv_layers"]
    if variant == "_ATOM_CTX":
        assert "x2g_atom_context_fwd" not in names and "x2g_atom_context_bwd" not in names
        assert names.count("x2g_segment_sum") >= layers and names.count("x2g_segment_broadcast") >= layers
        assert names.count("x2g_sbf_attention_fwd_center_sf") == layers
    elif variant == "_CENTER":
        assert names.count("x2g_atom_context_fwd") == layers
        assert not any(n.startswith("x2g_sbf_attention_fwd_center") for n in names)
    else:
        assert "x2g_atom_context_fwd" not in names
        modes = [a[6] for n, a in seen if n.startswith("x2g_sbf_attention_fwd")]
        assert modes == [EDGE_PER_TRIPLET] * layers


def test_fan_in_gradients_match_autograd_adds(cuda):
    """The layer input has one more consumer than in SBFTransformer, the atom context, which joins the in-place
    fan-in through the backward kernel's accumulate flag: the same parameter gradients as autograd's own adds
    (test_gpu_model.test_fan_in_gradients_match_autograd_adds' criterion)."""
    import x2gnn
    from x2gnn import ops
    from x2gnn.data import collate
    from x2gnn.synth import synthetic_molecules

    cfg = dict(conv_layers=3, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)
    b = collate(synthetic_molecules(4, "S160", seed=3)).to(cuda)
    m = x2gnn.xgnn_poly_v2(device="cuda", **cfg)
    load_seeded(m, 11)
    m = m.to(cuda)
    grads = []
    for fan in (True, False):
        ops._FAN_IN = fan
        try:
            m.zero_grad(set_to_none=True)
            line, plan = m.line_graph_data(b)
            assert m.fin_model._fan_in_ok(line, line.x) == fan
            e = m(b)
            (e * torch.linspace(0.5, 1.5, e.numel(), device=cuda)).sum().backward()
            grads.append({n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None})
        finally:
            ops._FAN_IN = True
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 20
    top = max(float(g.abs().max()) for g in grads[1].values())
    for n in grads[0]:
        a, r = grads[0][n], grads[1][n]
        assert float((a - r).abs().max()) <= 1e-5 * float(r.abs().max()) + 1e-6 * top, n
    ops._ATOM_CTX = False  # the composition is not fan-aware: the trunk leaves the fan-in to autograd
    try:
        line, plan = m.line_graph_data(b)
        assert not m.fin_model._fan_in_ok(line, line.x)
    finally:
        ops._ATOM_CTX = True


def test_graphed_training_steps_equal_eager_steps(cuda):
    """Three full steps (forward, loss, backward, clip + Adam + EMA) on 8 molecules replayed from the captured graphs
    leave parameters, optimizer state and EMA bitwise equal to three eager steps
    (test_gpu_model.test_graphed_training_steps_equal_eager_steps' criterion)."""
    import x2gnn
    from x2gnn.data import collate
    from x2gnn.synth import synthetic_molecules
    from x2gnn.train import Trainer

    cfg = dict(conv_layers=2, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)
    res = []
    for graphed in (False, True):
        torch.manual_seed(0)
        model = x2gnn.xgnn_poly_v2(device="cuda", **cfg).to(cuda)
        batch = collate(synthetic_molecules(8, "S160", seed=77)).to(cuda)
        tr = Trainer(model)
        if graphed:
            tr.capture(batch, warm=3)
        else:
            for _ in range(3):
                tr.forward_backward(batch)
        losses = [float(tr.step(batch).detach()) for _ in range(3)]
        torch.cuda.synchronize()
        res.append((losses, tr.opt.flat.clone(), tr.opt.exp_avg_sq.clone(), tr.opt.ema.clone()))
    assert res[0][0] == res[1][0] and all(np.isfinite(res[0][0]))
    for a, b in zip(res[0][1:], res[1][1:]):
        assert torch.equal(a, b)


def test_atom_without_neighbours(cuda):
    """A molecule with an atom beyond the cutoff of every other (no line node starts or ends at it: a zero row of
    atoms_rep, a bias-only table row nobody reads) between two ordinary molecules: finite energies equal to the
    float64 statement (tests/model_v2_ref.py), on the shipped route."""
    import model_v2_ref
    import x2gnn
    from x2gnn.data import collate
    from x2gnn.synth import molecule_from_geometry, random_geometry, synthetic_molecules

    rng = np.random.default_rng(5)
    zs, pos = random_geometry(rng, 1.8)
    k = len(zs) // 2  # an interior atom of the batch, 100 Angstrom away from its molecule
    zs, pos = np.insert(zs, k, 8), np.insert(pos, k, pos[0] + 100.0, axis=0)
    lone = molecule_from_geometry(zs, pos, feat_rng=np.random.default_rng(6))
    assert k not in lone["edge_index"][0] and k not in lone["edge_index"][1]
    ordinary = synthetic_molecules(2, "S160", seed=9)
    mols = [ordinary[0], lone, ordinary[1]]
    cfg = dict(conv_layers=2, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)
    host = collate(mols)
    _, want = model_v2_ref.statement(cfg, 23, host)
    m = x2gnn.xgnn_poly_v2(device="cuda", **cfg)
    load_seeded(m, 23)
    m = m.to(cuda)
    b = collate(mols).to(cuda)
    got = m(b)
    got.sum().backward()
    got = got.detach().cpu().numpy()
    assert got.shape == (3,) and np.isfinite(got).all()
    assert energy_rel_err(got, want.detach().numpy()) < ENERGY_RTOL
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def test_device_dataset_trainer_and_evaluator_take_it(cuda):
    """A batch assembled on the device (DeviceDataset) gives xgnn_poly_v2 the energies of the host-collated batch bit
    for bit, a Trainer steps on it and Trainer.evaluate reports a finite MAE on the averaged weights."""
    import x2gnn
    from x2gnn.data import collate
    from x2gnn.synth import synthetic_molecules
    from x2gnn.train import Trainer

    cfg = dict(conv_layers=2, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)
    mols = synthetic_molecules(6, "S160", seed=21)
    ds = x2gnn.DeviceDataset(mols, cuda)
    torch.manual_seed(0)
    model = x2gnn.xgnn_poly_v2(device="cuda", **cfg).to(cuda)
    idx = [4, 0, 3]
    with torch.no_grad():
        on_device = model(ds.batch(idx))
        on_host = model(collate([mols[i] for i in idx]).to(cuda))
    assert torch.equal(on_device, on_host) and bool(torch.isfinite(on_device).all())
    tr = Trainer(model)
    loss = tr.step(ds.batch(idx))
    mae = tr.evaluate(ds.loader(3, shuffle=False), std=2.0)
    assert np.isfinite(float(loss.detach())) and np.isfinite(np.asarray(mae, dtype=np.float64)).all()
