"""Evaluation on the averaged weights (x2gnn.train.Evaluator, Trainer.evaluate / run_epoch / state_dict) on the
GPU: the average is what is evaluated, in place and without disturbing training; captured equals eager; the
epoch loss and the MAE equal their host restatements; a saved trainer resumes bit for bit.

Every forward renormalises the embedding rows of the weights it runs on, in place (nn.Embedding's max_norm),
and a second renormalisation of a row already at the bound may move it by an ulp.  So wherever two evaluations
are compared bit for bit, both start from the same bytes of ``FlatAdam.ema``: a clone taken before the first
is copied back (in place) before the second, as test_gpu_model.py does for the live table."""
import io

import numpy as np
import pytest
import torch

from device_dataset_cases import mixed_molecules
from helpers import batch_from_fixture, energy_rel_err, golden, model_cfg, oracle_model
from weights import load_seeded

pytestmark = pytest.mark.gpu

CFG = dict(conv_layers=4, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)  # test_gpu_device_dataset.py
EPS = 2.0 ** -52

# positions in mixed_molecules(): 0-5 S160, 6 S5A, 7 the 2-atom molecule, 8 the 3-atom non-symmetric one, 9 S160
TRAIN_LISTS = [[0, 1, 2, 3], [5, 4, 9, 0], [3, 6, 1, 2, 5], [9, 7, 4]]
EVAL_LIST = [4, 0, 8, 2]


@pytest.fixture(scope="module")
def dataset(cuda):
    import x2gnn

    return x2gnn.DeviceDataset(mixed_molecules(), cuda)


def make_trainer(cuda, seed=0, **kw):
    import x2gnn

    torch.manual_seed(seed)
    return x2gnn.Trainer(x2gnn.xgnn_poly(device="cuda", **CFG).to(cuda), **kw)


def trained(cuda, dataset, steps, **kw):
    tr = make_trainer(cuda, **kw)
    for idx in TRAIN_LISTS[:steps]:
        tr.step(dataset.batch(idx))
    return tr


def model_like(tr, cuda, trainable=None):
    """A fresh xgnn_poly with the trainer's model state, its trainable parameters replaced by ``trainable``."""
    import x2gnn

    m = x2gnn.xgnn_poly(device="cuda", **CFG).to(cuda)
    m.load_state_dict(tr.model.state_dict())
    if trainable is not None:
        mine = [p for p in m.parameters() if p.requires_grad]
        assert len(mine) == len(trainable)
        with torch.no_grad():
            for p, v in zip(mine, trainable):
                p.copy_(v)
    return m.eval()


def host_abs_errors(e, y):
    """|e - y| per molecule in fp64, from the difference formed in fp32 (as the kernel and torch form it)."""
    d = e.detach().cpu().numpy().reshape(-1) - y.detach().cpu().numpy().reshape(-1)
    assert d.dtype == np.float32
    return np.abs(d).astype(np.float64)


def test_the_average_is_what_is_evaluated(cuda, dataset):
    tr = trained(cuda, dataset, 3)
    opt, b = tr.opt, dataset.batch(EVAL_LIST)
    ema_before = [t.clone() for t in opt.ema_params()]
    fresh = model_like(tr, cuda, ema_before)
    live = model_like(tr, cuda)
    with torch.no_grad():
        e_ref, e_live = fresh(b), live(b)
    kept = [t.clone() for t in (opt.flat, opt.exp_avg, opt.exp_avg_sq, tr.bucket.flat)]
    assert tr.model.training
    ev = tr.evaluator("ema")
    e = ev.update(b)
    assert torch.isfinite(e).all() and e.shape == (len(EVAL_LIST),)
    assert torch.equal(e, e_ref)  # the plain eval forward of a model that HOLDS the average
    assert not torch.equal(e, e_live)  # and not the live weights'
    assert tr.model.training  # the caller's mode is back
    # the average after the call = the fresh model's parameters after its forward: the rows of the averaged
    # embedding table for the batch's elements were renormalised in place, nothing else moved
    for got, want in zip(opt.ema_params(), [p for p in fresh.parameters() if p.requires_grad]):
        assert torch.equal(got, want)
    k = next(i for i, p in enumerate(opt.params) if p is tr.model.emb_block.embedding.weight)
    assert not torch.equal(opt.ema_params()[k], ema_before[k])
    # the live weights, both moments and the gradient bucket are untouched, bit for bit
    for was, now in zip(kept, (opt.flat, opt.exp_avg, opt.exp_avg_sq, tr.bucket.flat)):
        assert torch.equal(was, now)
    # the Parameters are the training views again, their .grad still the bucket's views, the marks in place
    for p, off in zip(opt.params, opt.offsets):
        assert p.data_ptr() == opt.flat.data_ptr() + 4 * off
        assert p.grad.data_ptr() == tr.bucket.flat.data_ptr() + 4 * off
        assert p._x2g_grad_sink is True
    # evaluating the live weights is the other choice
    opt_flat = opt.flat.clone()
    assert torch.equal(tr.evaluator("model").update(b), e_live)
    opt.flat.copy_(opt_flat)
    with pytest.raises(ValueError):
        tr.evaluator("best")


def test_averaged_context_restores_after_an_exception(cuda, dataset):
    tr = make_trainer(cuda)
    opt = tr.opt
    tr.model.eval()
    with pytest.raises(RuntimeError, match="inside"):
        with tr.averaged():
            for p, off in zip(opt.params, opt.offsets):
                assert p.data_ptr() == opt.ema.data_ptr() + 4 * off
            tr.model.train()
            raise RuntimeError("inside")
    assert not tr.model.training
    for p, off in zip(opt.params, opt.offsets):
        assert p.data_ptr() == opt.flat.data_ptr() + 4 * off
        assert p.grad.data_ptr() == tr.bucket.flat.data_ptr() + 4 * off


def test_averaged_energies_against_the_oracle(cuda):
    import x2gnn
    from oracle import ref_cpu

    z = golden("model_small.npz")
    m = x2gnn.xgnn_poly(device="cuda", **model_cfg(z))
    load_seeded(m, int(z["weight_seed"]))
    tr = x2gnn.Trainer(m.to(cuda))
    host = batch_from_fixture(z)
    b = host.to(cuda)
    for _ in range(2):
        tr.step(b)
    sd = tr.state_dict()
    orc = oracle_model(z)
    orc.load_state_dict({k: v.cpu() for k, v in sd["ema"].items()})
    with torch.no_grad():
        ref = ref_cpu.run_batch(orc.eval(), host).numpy()
    ev = tr.evaluator("ema")
    e = ev.update(b)
    err = energy_rel_err(e.cpu().numpy(), ref)
    print(f"averaged energies vs oracle: rel err {err:.3e}")
    assert err <= 1e-4
    res = ev.result()
    a = host_abs_errors(e, b.y)
    B = len(a)
    want = float(a.sum()) / B
    print(f"mae {res['mae']!r} host {want!r}")
    assert abs(res["mae"] - want) <= B * EPS * want
    assert res["count"] == B and res["max_abs"] == float(a.max())
    # (the sum's bound, plus the division and the square root on either side: two roundings each)
    assert abs(res["rmse"] - float(np.sqrt((a * a).sum() / B))) <= (B + 2) * EPS * res["rmse"]


def test_evaluate_over_a_loader(cuda, dataset):
    """Trainer.evaluate over ten molecules in batches of 4, 4 and 2 (a change of shape between calls)."""
    tr = trained(cuda, dataset, 2)
    opt = tr.opt
    start = opt.ema.clone()
    loader = dataset.loader(4, shuffle=False, indices=range(10))
    assert [len(i) for i in loader.index_lists()] == [4, 4, 2]
    mae = tr.evaluate(loader, std=23.06)
    opt.ema.copy_(start)
    ev = tr.evaluator("ema")
    ev.reset()
    errs = np.concatenate([host_abs_errors(ev.update(b), b.y) for b in loader])
    assert errs.shape == (10,)
    want = 23.06 * float(errs.sum()) / 10
    print(f"mae {mae!r} host {want!r}")
    assert abs(mae - want) <= 10 * EPS * want
    res = ev.result(std=23.06)
    assert res["count"] == 10 and res["mae"] == mae and res["max_abs"] == 23.06 * float(errs.max())


def test_captured_equals_eager_and_follows_the_average(cuda, dataset):
    tr = trained(cuda, dataset, 2)
    opt, b = tr.opt, dataset.batch(EVAL_LIST)
    start = opt.ema.clone()
    ev = tr.evaluator("ema")
    ev.acc.fill_(7.0)
    ev.capture(b)  # (recording update() in a graph at all: it reads nothing back)
    assert (ev.acc.cpu() == 7.0).all()  # the warm-up passes are not counted

    def replay():
        ev.reset()
        return ev.update(b).clone(), ev.acc.clone()

    def eager():
        fresh = tr.evaluator("ema")
        return fresh.update(b).clone(), fresh.acc.clone()

    opt.ema.copy_(start)
    e_g, acc_g = replay()
    opt.ema.copy_(start)
    e_e, acc_e = eager()
    assert torch.isfinite(e_g).all() and float(acc_g[3]) == len(EVAL_LIST)
    assert torch.equal(e_g, e_e) and torch.equal(acc_g, acc_e)
    for idx in TRAIN_LISTS[2:4]:
        tr.step(dataset.batch(idx))
    later = opt.ema.clone()
    e_g2, acc_g2 = replay()  # the graph reads FlatAdam.ema: the average as it is now
    opt.ema.copy_(later)
    e_e2, acc_e2 = eager()
    assert torch.equal(e_g2, e_e2) and torch.equal(acc_g2, acc_e2)
    assert not torch.equal(e_g2, e_g)


def test_capture_refuses_a_tiled_batch_and_eager_keeps_working(cuda, dataset, monkeypatch):
    from x2gnn import ops

    tr = trained(cuda, dataset, 1)
    opt, b = tr.opt, dataset.batch(EVAL_LIST)
    start = opt.ema.clone()
    whole = tr.evaluator("ema").update(b).clone()
    opt.ema.copy_(start)
    monkeypatch.setattr(ops, "INFER_TILE", 4096)
    assert int(b.host_meta()["triplets"].sum()) > 4096
    ev = tr.evaluator("ema")
    with pytest.raises(ValueError, match="INFER_TILE"):
        ev.capture(b)
    assert ev.graph is None
    assert torch.equal(ev.update(b), whole)


def test_training_is_not_disturbed_by_an_evaluation(cuda, dataset):
    runs = []
    for evaluate in (False, True):
        tr = make_trainer(cuda)
        losses = []
        for k, idx in enumerate(TRAIN_LISTS):
            if evaluate and k == 2:
                mae = tr.evaluate(dataset.loader(5, shuffle=False, indices=[8, 1, 6, 7, 3, 2]), std=2.0)
                assert np.isfinite(mae) and mae > 0
            losses.append(tr.step(dataset.batch(idx)).detach().clone())
        runs.append((torch.stack(losses), tr.opt.flat.clone(), tr.opt.exp_avg.clone(), tr.opt.exp_avg_sq.clone()))
    assert torch.isfinite(runs[0][0]).all()
    for a, b in zip(*runs):  # (opt.ema is not compared: the evaluation renormalised it, as the reference's would)
        assert torch.equal(a, b)


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_run_epoch(cuda, dataset, captured):
    """The epoch loss equals sum float(loss_b) * n_b / sum n_b in Python floats exactly (an fp32 loss times a
    small integer is exact in fp64, and the device adds in the same order)."""
    lists = [[0, 1, 2, 3], [5, 4, 9, 0], [8, 6]]
    if captured:
        lists = [lists[0]] * 3
    a, b = make_trainer(cuda), make_trainer(cuda)
    if captured:
        fixed = dataset.batch(lists[0])
        a.capture(fixed)
        b.capture(fixed)
        batches = [fixed] * 3
        graphs = a.graphs
    else:
        batches = [dataset.batch(i) for i in lists]
    got = a.run_epoch(iter(batches))
    s = c = 0.0
    for batch in batches:
        n = batch.num_graphs
        s += n * float(b.step(batch).detach())
        c += n
    assert c == sum(len(i) for i in lists) and np.isfinite(s)
    assert got == s / c
    if captured:
        assert a.graphs is graphs  # the graphs are replayed as they were: the accumulation is outside them
    assert torch.equal(a.opt.flat, b.opt.flat) and torch.equal(a.opt.ema, b.opt.ema)
    assert torch.equal(a.step(batches[0]), b.step(batches[0]))  # step() itself is what it was


SCHEDULE = dict(warmup_steps=2, decay_steps=4, decay_rate=0.5)


def test_resume_from_a_saved_state(cuda, dataset):
    import x2gnn

    a = trained(cuda, dataset, 2, lr_schedule=SCHEDULE)
    buf = io.BytesIO()
    torch.save(a.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf)
    third = dataset.batch(TRAIN_LISTS[2])
    loss_a = a.step(third).clone()

    def state(tr):
        o = tr.opt
        return o.flat, o.ema, o.exp_avg, o.exp_avg_sq, o.scalars

    for captured in (False, True):
        b = make_trainer(cuda, seed=1, lr_schedule=SCHEDULE)
        assert not torch.equal(b.opt.flat, a.opt.flat)
        if captured:
            b.capture(third)
        held = [t.data_ptr() for t in state(b)]
        b.load_state_dict(sd)
        assert held == [t.data_ptr() for t in state(b)]  # copied into the buffers, nothing rebound
        loss_b = b.step(third)
        assert torch.equal(loss_b, loss_a), captured
        for x, y in zip(state(a), state(b)):
            assert torch.equal(x, y), captured

    b = make_trainer(cuda, seed=1, lr_schedule=SCHEDULE)
    name = next(iter(sd["model"]))
    with pytest.raises(KeyError):
        b.load_state_dict({**sd, "model": {k: v for k, v in sd["model"].items() if k != name}})
    with pytest.raises(KeyError):
        b.load_state_dict({**sd, "ema": {**sd["ema"], "no.such.weight": sd["ema"][name]}})
    bad = {**sd["optimizer"], "exp_avg": {k: v.reshape(-1)[:1] for k, v in sd["optimizer"]["exp_avg"].items()}}
    with pytest.raises(ValueError):
        b.load_state_dict({**sd, "optimizer": bad})
    # the averaged model, out of the state: a fresh model takes "ema" strictly
    fresh = x2gnn.xgnn_poly(device="cuda", **CFG)
    fresh.load_state_dict(sd["ema"], strict=True)
    assert set(sd["ema"]) == set(a.model.state_dict())
    w = "emb_trans.weight"
    assert torch.equal(dict(fresh.named_parameters())[w].detach().to(cuda), sd["ema"][w])
    assert not torch.equal(sd["ema"][w], sd["model"][w])
