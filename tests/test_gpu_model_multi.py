"""Multi-target models through the public interface on the GPU: xgnn_poly / xgnn_poly_global with num_target = 3 and
xgnn_poly_multi against the oracle with K-wide readouts and against the reference's own K = 3 run
(tests/golden/model_multi.npz), the ABI calls of num_target = 1 against today's model, and Trainer, Evaluator and
DeviceDataset on [B, K] labels.  Two conv layers, D = 128, weights from weights.load_seeded."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import energy_rel_err, model_cfg
from model_multi_cases import MODELS, batch_k, copy_shared, fixture, oracle_k, oracle_of, small_batch
from test_gpu_model import ENERGY_RTOL, _grads_vs_oracle, check_vs_fixture, record_calls
from weights import load_seeded

from oracle import ref_cpu

pytestmark = pytest.mark.gpu

CFG = dict(conv_layers=2, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)
K = 3


def product(kind, pool_option, cuda, seed, **kw):
    import x2gnn

    if kind == "poly":
        m = x2gnn.xgnn_poly(device="cuda", **CFG, **kw)
    else:
        m = x2gnn.xgnn_poly_global(device="cuda", pool_option=pool_option, **CFG, **kw)
    load_seeded(m, seed)
    return m.to(cuda)


def columns_close(res, ref):
    """Per molecule and per column: helpers.energy_rel_err of every column under ENERGY_RTOL; returns the worst."""
    res, ref = np.asarray(res, np.float64), np.asarray(ref, np.float64)
    assert res.shape == ref.shape and res.ndim == 2
    worst = max(energy_rel_err(res[:, k], ref[:, k]) for k in range(ref.shape[1]))
    print("worst per-column energy error:", worst)
    assert worst < ENERGY_RTOL
    return worst


# ------------------------------------------------------------------------------ K = 3 against oracle and reference
@pytest.fixture(scope="module")
def oracles():
    """Per model of the fixture: the widened oracle after one forward + backward (computed once, left unchanged)."""
    out = {}
    for model in MODELS:
        z = fixture(model)
        orc = oracle_of(z)
        b = batch_k(z)
        res = ref_cpu.run_batch(orc, b)
        torch.nn.functional.smooth_l1_loss(res, b.y.view(-1)).backward()
        out[model] = (orc, res.detach().view(b.y.shape).numpy())
    return out


@pytest.mark.parametrize("shipped", [True, False], ids=["shipped", "dst_major"])
@pytest.mark.parametrize("model", MODELS)
def test_three_targets_vs_oracle_and_reference(cuda, monkeypatch, oracles, model, shipped):
    z = fixture(model)
    assert model_cfg(z) == CFG and int(z["num_target"]) == K
    m = product(str(z["kind"]), str(z["pool_option"]), cuda, int(z["weight_seed"]), num_target=K)
    b = batch_k(z, shipped=shipped).to(cuda)
    seen = record_calls(monkeypatch)
    res = m(b)
    assert tuple(res.shape) == (b.num_graphs, K) and m.num_target == K
    orc, ref = oracles[model]
    columns_close(res.detach().cpu().numpy(), ref)
    # the reference's flattened tensor is this one's row-major flattening: check_vs_fixture's rule on it
    assert check_vs_fixture(m, z, res.view(-1), b.y.view(-1)) >= 5
    _grads_vs_oracle(m, orc)
    names = [n for n, _ in seen]
    assert names.count("x2g_readout_heads_k_fwd") == 1 and names.count("x2g_readout_heads_k_bwd") == 1
    assert not any(n.startswith("x2g_readout_head_") for n in names)


@pytest.mark.parametrize("model", ["poly", "global_add"])
def test_columns_equal_the_one_target_models(cuda, model):
    """Column k of the K = 3 model is the K = 1 model that has row k of each last layer."""
    z = fixture(model)
    kind, pool = str(z["kind"]), str(z["pool_option"])
    m3 = product(kind, pool, cuda, int(z["weight_seed"]), num_target=K)
    b = batch_k(z).to(cuda)
    with torch.no_grad():
        wide = m3(b).cpu().numpy()
        for k in range(K):
            m1 = product(kind, pool, cuda, 1)
            left = copy_shared(m1, m3)
            assert left and all("mlp.4." in n for n in left)
            for r1, r3 in zip(m1.fin_model.readouts, m3.fin_model.readouts):
                r1.mlp[4].weight.copy_(r3.mlp[4].weight[k:k + 1])
                r1.mlp[4].bias.copy_(r3.mlp[4].bias[k:k + 1])
            one = m1(b)
            assert tuple(one.shape) == (b.num_graphs,)
            assert energy_rel_err(wide[:, k], one.cpu().numpy()) < ENERGY_RTOL


# ------------------------------------------------------------------------------ the two-family model
def _multi(cuda, ka, km, pool_option="mean", seed=401):
    import x2gnn

    m = x2gnn.xgnn_poly_multi(device="cuda", atom_targets=ka, mol_targets=km, pool_option=pool_option, **CFG)
    load_seeded(m, seed)
    return m.to(cuda)


def _family_oracle(multi, family, k, pool_option):
    """The oracle of one family alone, with the multi model's trunk and that family's readout weights."""
    orc = oracle_k("poly" if family == "readouts" else "global", pool_option, k, 0, CFG)
    sd = {n: v.detach().cpu() for n, v in multi.state_dict().items()}
    own = dict(orc.named_parameters())
    with torch.no_grad():
        for n, p in own.items():
            src = n.replace("fin_model.readouts.", f"fin_model.{family}.") if "fin_model.readouts." in n else n
            p.copy_(sd[src])
    return orc


@pytest.mark.parametrize("pool_option", ["mean", "add"])
def test_multi_model_vs_its_families_and_the_oracle(cuda, pool_option):
    z = fixture("poly")
    m = _multi(cuda, 2, 2, pool_option)
    b = batch_k(z).to(cuda)
    y = torch.from_numpy(np.random.default_rng(3).standard_normal((b.num_graphs, 4)).astype(np.float32)).to(cuda)
    with torch.no_grad():
        m(b)  # (the first forward applies the embedding's max_norm renorm: the weights copied below are settled)
    res = m(b)
    assert tuple(res.shape) == (b.num_graphs, 4) and m.num_target == 4
    # the families alone, sharing the trunk's weights: the same columns (the same kernels on the same values)
    atoms = product("poly", None, cuda, 1, num_target=2)
    mols = product("global", pool_option, cuda, 1, num_target=2)
    assert not copy_shared(atoms, m, skip=())
    left = copy_shared(mols, m, skip=("readouts.",))
    assert left and all("readouts." in n for n in left)
    for r, src in zip(mols.fin_model.readouts, m.fin_model.mol_readouts):
        r.load_state_dict(src.state_dict())
    ea, em = atoms(b).detach(), mols(b).detach()
    assert torch.equal(res.detach()[:, 2:], ea) and torch.equal(res.detach()[:, :2], em)
    # the oracle, family by family
    hb = batch_k(z)
    oa, om = _family_oracle(m, "readouts", 2, pool_option), _family_oracle(m, "mol_readouts", 2, pool_option)
    ra, rm = ref_cpu.run_batch(oa, hb).view(-1, 2), ref_cpu.run_batch(om, hb).view(-1, 2)
    columns_close(res.detach().cpu().numpy(), torch.cat([rm, ra], dim=1).detach().numpy())
    # the joint loss is the mean over all four columns: half the sum of the two families' own mean losses
    from x2gnn import ops

    ops.smooth_l1_loss(res, y).backward()
    yc = y.cpu()
    (0.5 * torch.nn.functional.smooth_l1_loss(ra, yc[:, 2:])).backward()
    (0.5 * torch.nn.functional.smooth_l1_loss(rm, yc[:, :2])).backward()
    ga, gm = dict(oa.named_parameters()), dict(om.named_parameters())
    ref = {}
    for n, p in m.named_parameters():
        if "fin_model.mol_readouts." in n:
            ref[n] = gm[n.replace("mol_readouts", "readouts")].grad
        elif "fin_model.readouts." in n:
            ref[n] = ga[n].grad
        else:  # the shared trunk and featurisation: the sum of the two
            g1, g2 = ga[n].grad, gm[n].grad
            ref[n] = None if g1 is None and g2 is None else (0 if g1 is None else g1) + (0 if g2 is None else g2)
    scale = max(float(g.abs().max()) for g in ref.values() if g is not None)
    for n, p in m.named_parameters():
        if ref[n] is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        err = float((p.grad.detach().cpu() - ref[n]).abs().max())
        assert err <= 2e-3 * float(ref[n].abs().max()) + 1e-6 * scale, (n, err)


# ------------------------------------------------------------------------------ K = 1 is today's path
def _calls(m, b, monkeypatch):
    """(name, the scalar arguments) of every ABI call of a forward and a backward."""
    with torch.no_grad():
        m(b)  # (the first forward applies the embedding's max_norm renorm)
    seen = record_calls(monkeypatch)
    res = m(b)
    torch.nn.functional.smooth_l1_loss(res.view(-1), b.y.view(-1)).backward()
    out = [(n, tuple(a for a in args if isinstance(a, (int, float)) and not isinstance(a, bool))) for n, args in seen]
    monkeypatch.undo()
    return out


@pytest.mark.parametrize("kind", ["poly", "global"])
def test_one_target_makes_todays_calls(cuda, monkeypatch, kind):
    from x2gnn.data import collate

    b = collate(small_batch(1)).to(cuda)
    today = _calls(product(kind, "mean", cuda, 7), b, monkeypatch)
    names = [n for n, _ in today]
    assert "x2g_readout_head_pool_fwd" in names or "x2g_readout_head_fwd" in names
    assert not any("heads_k" in n or n == "x2g_error_accum_cols" for n in names)
    assert _calls(product(kind, "mean", cuda, 7, num_target=1), b, monkeypatch) == today
    ka, km = (1, 0) if kind == "poly" else (0, 1)
    assert _calls(_multi(cuda, ka, km, seed=7), b, monkeypatch) == today


# ------------------------------------------------------------------------------ training and evaluation
def _trainer(cuda):
    import x2gnn

    return x2gnn.Trainer(product("poly", None, cuda, 11, num_target=K))


def _train_batch(cuda):
    from x2gnn.data import collate

    return collate(small_batch(K)).to(cuda)


def test_eager_steps_decrease_the_loss(cuda):
    tr, b = _trainer(cuda), _train_batch(cuda)
    losses = [float(tr.step(b).detach()) for _ in range(3)]
    print("losses:", losses)
    assert all(np.isfinite(losses)) and losses[2] < losses[0]
    assert all(bool(torch.isfinite(p).all()) for p in tr.model.parameters())


def test_captured_steps_equal_eager_steps_and_a_checkpoint_round_trips(cuda):
    b = _train_batch(cuda)
    eager, graphed = _trainer(cuda), _trainer(cuda)
    for _ in range(3):  # the forwards a capture's warm-up makes (each applies the max_norm renorm)
        eager.forward_backward(b)
    graphed.capture(b, warm=3)
    le, lg = [], []
    for i in range(3):
        le.append(eager.step(b).detach().clone())
        lg.append(graphed.step(b).detach().clone())
        if i == 1:
            saved = eager.state_dict()
    torch.cuda.synchronize()
    assert all(torch.equal(a, c) for a, c in zip(le, lg)) and len({float(v) for v in le}) == 3
    assert torch.equal(eager.opt.flat, graphed.opt.flat) and torch.equal(eager.opt.ema, graphed.opt.ema)
    assert tuple(saved["model"]["fin_model.readouts.0.mlp.4.weight"].shape) == (K, 128)
    fresh = _trainer(cuda)
    for _ in range(3):
        fresh.forward_backward(b)
    fresh.load_state_dict(saved)
    assert torch.equal(fresh.step(b).detach(), le[2]) and torch.equal(fresh.opt.flat, eager.opt.flat)
    again = fresh.state_dict()
    fresh.load_state_dict(again)
    for k, v in again["model"].items():
        assert torch.equal(fresh.state_dict()["model"][k], v), k


def test_evaluate_per_target(cuda):
    import x2gnn

    tr, b = _trainer(cuda), _train_batch(cuda)
    tr.step(b)
    ev = x2gnn.Evaluator(tr.model)
    assert tuple(ev.acc.shape) == (K, 4)
    e = ev.update(b)
    ev.update(b)
    std = [1.0, 2.0, 0.5]
    got = ev.result(std)
    d = np.abs(e.detach().cpu().numpy() - b.y.cpu().numpy()).astype(np.float64)  # (d formed in fp32, then widened)
    assert got["count"] == 2 * b.num_graphs and [len(got[k]) for k in ("mae", "rmse", "max_abs")] == [K, K, K]
    np.testing.assert_allclose(got["mae"], np.array(std) * d.mean(0), rtol=1e-14)
    np.testing.assert_allclose(got["rmse"], np.array(std) * np.sqrt((d * d).mean(0)), rtol=1e-14)
    np.testing.assert_array_equal(got["max_abs"], np.array(std) * d.max(0))
    np.testing.assert_allclose(ev.result(2.0)["mae"], 2.0 * d.mean(0), rtol=1e-14)
    with pytest.raises(ValueError):
        ev.result([1.0, 2.0])
    # Trainer.evaluate: the averaged weights, per target
    mae = tr.evaluate([b, b], std=std)
    avg = product("poly", None, cuda, 11, num_target=K)
    avg.load_state_dict(tr.state_dict()["ema"])
    avg.eval()
    with torch.no_grad():
        ea = avg(b)
    da = np.abs(ea.cpu().numpy() - b.y.cpu().numpy()).astype(np.float64)
    assert isinstance(mae, list) and len(mae) == K
    np.testing.assert_allclose(mae, np.array(std) * da.mean(0), rtol=1e-5)
    # a captured evaluation adds into the same [K, 4] accumulator
    ev2 = x2gnn.Evaluator(tr.model)
    ev2.capture(b)
    ev2.reset()
    ev2.update(b)
    ev2.update(b)
    assert torch.equal(ev2.acc, ev.acc)


# ------------------------------------------------------------------------------ the device dataset
@pytest.mark.parametrize("idx", [[0, 1, 2], [2, 0], [1, 1, 2, 1]], ids=["all", "subset", "repeats"])
def test_device_dataset_with_wide_labels(cuda, monkeypatch, idx):
    import x2gnn
    from device_dataset_cases import mixed_molecules
    from test_gpu_device_dataset import assert_same_batch, collated

    ys = np.random.default_rng(5).standard_normal((10, K)).astype(np.float32)
    mols = [dict(m, y=ys[i]) for i, m in enumerate(mixed_molecules())]
    ds = x2gnn.DeviceDataset(mols, cuda)
    assert tuple(ds.y.shape) == (10, K)
    seen = record_calls(monkeypatch)
    got = ds.batch([3 * i for i in idx])
    asm = [a for n, a in seen if n == "x2g_batch_assemble"]
    assert len(asm) == 1 and asm[0][6] is None and asm[0][19] is None  # both y pointers NULL
    monkeypatch.undo()
    assert tuple(got.y.shape) == (len(idx), K) and torch.equal(got.y.cpu(), torch.from_numpy(ys[[3 * i for i in idx]]))
    assert_same_batch(got, collated(mols, [3 * i for i in idx], cuda, monkeypatch))
    order = [9, 3, 3, 0, 6]
    new = ds.reordered(order)
    assert tuple(new.y.shape) == (5, K)
    assert_same_batch(new.batch([1, 4, 0]), collated(mols, [order[i] for i in (1, 4, 0)], cuda, monkeypatch))


def test_from_collated_takes_wide_labels_only_when_asked(cuda):
    import x2gnn
    from x2gnn import datasets as xds

    cds = xds.CollatedDataset.load(os.path.join(GOLDEN, "pyg_inmemory_v21.pt"))
    with pytest.raises(ValueError, match="prepare_target"):
        x2gnn.DeviceDataset.from_collated(cds, cuda)  # y is [M, 12]: the default still refuses it
    scales = xds.prepare_targets(cds, list(range(12)))
    with pytest.raises(ValueError, match="prepare_target"):
        x2gnn.DeviceDataset.from_collated(cds, cuda)
    with pytest.raises(ValueError, match="prepare_targets"):
        x2gnn.DeviceDataset.from_collated(cds, cuda, num_target=3)
    ds = x2gnn.DeviceDataset.from_collated(cds, cuda, num_target=12)
    got = ds.batch([2, 0, 2])
    assert len(scales) == 12 and tuple(got.y.shape) == (3, 12)
    assert torch.equal(got.y.cpu(), cds.data.y[[2, 0, 2]].to(torch.float32))
