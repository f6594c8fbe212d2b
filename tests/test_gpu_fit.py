"""x2gnn.fit on the GPU: the epoch loop equals the same loop written by hand, checkpoints hold what they should, a
resumed run continues bit for bit, a plateau reduction reaches a captured update graph, and a model initialised by
reference_init_ (orthogonal weights: another input distribution than the seeded ones of the parity tests) still
matches the oracle."""
import os

import numpy as np
import pytest
import torch

from device_dataset_cases import mixed_molecules
from helpers import energy_rel_err

from oracle import ref_cpu

pytestmark = pytest.mark.gpu

CFG = dict(conv_layers=2, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)
ENERGY_RTOL = 1e-4  # tests/test_gpu_model.py
BATCH = 3


@pytest.fixture(scope="module")
def dataset(cuda):
    import x2gnn

    return x2gnn.DeviceDataset(mixed_molecules(), cuda)


@pytest.fixture(scope="module")
def split():
    from x2gnn.datasets import split_indices

    s = split_indices(10, (2, 5), 41)
    assert [len(p) for p in s] == [2, 3, 5]
    return s


def make_model(cuda, seed=3):
    import x2gnn

    torch.manual_seed(0)
    return x2gnn.reference_init_(x2gnn.xgnn_poly(device="cuda", **CFG), torch.Generator().manual_seed(seed)).to(cuda)


def make_trainer(cuda, **kw):
    import x2gnn

    return x2gnn.Trainer(make_model(cuda), **kw)


def plateau(tr):
    import x2gnn

    return x2gnn.Plateau(tr.opt, factor=0.5, patience=0, min_lr=1e-5)


def assert_same_state(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], dict):
            assert_same_state(a[k], b[k])
        elif torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_fit_equals_the_loop_written_by_hand(cuda, dataset, split, tmp_path):
    import x2gnn

    test_idx, val_idx, train_idx = split
    tr, twin = make_trainer(cuda), make_trainer(cuda)
    best_path = str(tmp_path / "best.pt")
    hist = x2gnn.fit(tr, dataset, split, epochs=3, batch_size=BATCH, schedule=plateau(tr), save_after=0,
                     best_path=best_path)
    sched, best, want, saved = plateau(twin), None, [], None
    for e in range(3):
        loss = twin.run_epoch(dataset.loader(BATCH, shuffle=False, seed=e, indices=train_idx))
        val = twin.evaluate(dataset.loader(BATCH, shuffle=False, indices=val_idx), 1.0)
        sched.step(val)
        if best is None or val <= best:
            best = val
            if e > 0:
                twin.evaluate(dataset.loader(BATCH, shuffle=False, indices=test_idx), 1.0)
                saved = (e, best, sched.state_dict())
        want.append({"epoch": e, "lr": float(twin.opt.lr), "loss": loss, "val": val, "best": best})
    print("history", hist)
    for h, w in zip(hist, want):
        assert {k: h[k] for k in w} == w
        assert h["skipped"] == 0
    assert len(hist) == 3 and hist[0]["test"] is None
    assert all(np.isfinite(h["loss"]) and np.isfinite(h["val"]) for h in hist)
    assert_same_state(tr.state_dict(), twin.state_dict())
    # the checkpoint: the last epoch past save_after that was the best so far
    if saved is None:
        assert not os.path.exists(best_path)
    else:
        ckpt = torch.load(best_path, weights_only=True)
        assert (ckpt["epoch"], ckpt["best"], ckpt["schedule"]) == saved and ckpt["seed"] == 0
        assert hist[saved[0]]["test"] is not None
        fresh = x2gnn.xgnn_poly(device="cuda", **CFG)
        fresh.load_state_dict(ckpt["ema"])
    assert not os.path.exists(best_path + ".tmp")


def test_a_resumed_run_continues_bit_for_bit(cuda, dataset, split, tmp_path):
    import x2gnn

    kw = dict(batch_size=BATCH, shuffle=True, seed=5, save_after=0)
    straight = make_trainer(cuda)
    s4 = plateau(straight)
    h4 = x2gnn.fit(straight, dataset, split, epochs=4, schedule=s4, **kw)
    last = str(tmp_path / "last.pt")
    first = make_trainer(cuda)
    h2 = x2gnn.fit(first, dataset, split, epochs=2, schedule=plateau(first), last_path=last, **kw)
    assert h2 == h4[:2]
    ckpt = torch.load(last, weights_only=True)
    assert ckpt["epoch"] == 1 and ckpt["best"] == h2[-1]["best"] and ckpt["seed"] == 5
    second = make_trainer(cuda, lr=3e-3)  # (another rate: the loaded state must replace it)
    sched = x2gnn.Plateau(second.opt, factor=0.5, patience=0, min_lr=1e-5)
    tail = x2gnn.fit(second, dataset, split, epochs=4, schedule=sched, resume=last, **kw)
    assert [h["epoch"] for h in tail] == [2, 3]
    assert tail == h4[2:]
    assert_same_state(second.state_dict(), straight.state_dict())
    assert sched.state_dict() == s4.state_dict() and sched.last_epoch == 4


def test_a_plateau_reduction_reaches_the_captured_update(cuda, dataset):
    import x2gnn

    b = dataset.batch([0, 1, 2, 8])
    eager, graphed = make_trainer(cuda), make_trainer(cuda)
    graphed.capture(b, warm=3)
    scheds = [x2gnn.Plateau(t.opt, factor=0.5, patience=0, min_lr=1e-5, lr=1e-3) for t in (eager, graphed)]
    for t in (eager, graphed):
        t.step(b)
    for s in scheds:
        assert s.step(1.0) == 1e-3
        assert s.step(2.0) == 5e-4  # a worse epoch: reduced, written into the scalar block
    for t in (eager, graphed):
        t.step(b)
    torch.cuda.synchronize()
    assert float(graphed.opt.lr) == float(torch.tensor(5e-4, dtype=torch.float32))
    assert torch.equal(eager.opt.flat, graphed.opt.flat) and torch.equal(eager.opt.ema, graphed.opt.ema)
    assert torch.equal(eager.opt.scalars, graphed.opt.scalars)


def test_reference_init_weights_match_the_oracle(cuda):
    from x2gnn.data import collate
    from x2gnn.synth import synthetic_molecules

    m = make_model(cuda, seed=11)
    orc = ref_cpu.XGNN(**CFG)
    orc.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    b = collate(synthetic_molecules(4, "S160", seed=21))
    ref = ref_cpu.run_batch(orc, b)
    torch.nn.functional.smooth_l1_loss(ref, b.y).backward()
    bd = b.to(cuda)
    res = m(bd)
    torch.nn.functional.smooth_l1_loss(res, bd.y).backward()
    err = energy_rel_err(res.detach().cpu().numpy(), ref.detach().numpy())
    print("energy rel err", err)
    assert err < ENERGY_RTOL
    ref_grads = {n: p.grad for n, p in orc.named_parameters()}
    scale = max(float(g.abs().max()) for g in ref_grads.values() if g is not None)
    for n, p in m.named_parameters():  # the 2e-3 rule of tests/test_gpu_model.py
        rg = ref_grads.get(n)
        if rg is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        got = p.grad.detach().cpu()
        assert float((got - rg).abs().max()) <= 2e-3 * float(rg.abs().max()) + 1e-6 * scale, n
