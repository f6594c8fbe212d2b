"""Trainer(skip_nonfinite=True): a non-finite gradient bucket costs one skipped step and nothing else; the default
makes the call it always made (and is poisoned by the same bucket).

The poison goes into the bucket, not through the model's kernels: forward_backward, one bucket element set to inf,
update."""
import pytest
import torch

from device_dataset_cases import mixed_molecules

pytestmark = pytest.mark.gpu

CFG = dict(conv_layers=2, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)
BATCHES = [[0, 1, 7, 2], [3, 8, 4], [5, 6, 9]]


@pytest.fixture(scope="module")
def dataset(cuda):
    import x2gnn

    return x2gnn.DeviceDataset(mixed_molecules(), cuda)


def make_trainer(cuda, **kw):
    import x2gnn

    torch.manual_seed(0)
    return x2gnn.Trainer(x2gnn.xgnn_poly(device="cuda", **CFG).to(cuda), **kw)


def record_optim_calls(monkeypatch):
    """The names of the C-ABI entries x2gnn.optim calls from here on."""
    from x2gnn import optim

    seen, inner = [], optim.call

    def rec(name, *args):
        seen.append(name)
        return inner(name, *args)

    monkeypatch.setattr(optim, "call", rec)
    return seen


def snapshot(tr):
    opt = tr.opt
    return ({k: v.clone() for k, v in tr.model.state_dict().items()}, opt.ema.clone(), opt.exp_avg.clone(),
            opt.exp_avg_sq.clone(), opt.steps.clone())


def assert_same_state(tr, snap):
    model, ema, m, v, steps = snap
    now = tr.model.state_dict()
    assert set(now) == set(model)
    for k in model:
        assert torch.equal(now[k], model[k]), k
    assert torch.equal(tr.opt.ema, ema) and torch.equal(tr.opt.exp_avg, m) and torch.equal(tr.opt.exp_avg_sq, v)
    assert torch.equal(tr.opt.steps, steps)


def test_a_poisoned_bucket_is_one_skipped_step(cuda, dataset):
    tr = make_trainer(cuda, skip_nonfinite=True)
    twin = make_trainer(cuda)  # unguarded: the same forward_backward calls, never poisoned, never updated on b1
    b0, b1, b2 = (dataset.batch(i) for i in BATCHES)
    for t in (tr, twin):
        t.step(b0)
    tr.forward_backward(b1)
    twin.forward_backward(b1)
    snap = snapshot(tr)
    tr.bucket.flat[17] = float("inf")
    tr.update()
    assert_same_state(tr, snap)
    assert bool((tr.bucket.flat == 0).all())
    assert int(tr.opt.skipped) == 1 and int(tr.opt.last_skipped) == 1
    assert float(tr.opt.grad_norm) == float("inf")
    # the twin drops b1's gradients unapplied (its next forward_backward zeroes the bucket): both then make the
    # same clean step
    la, lb = tr.step(b2), twin.step(b2)
    assert torch.equal(la, lb)
    assert int(tr.opt.skipped) == 1 and int(tr.opt.last_skipped) == 0
    for a, b in ((tr.opt.flat, twin.opt.flat), (tr.opt.ema, twin.opt.ema), (tr.opt.exp_avg, twin.opt.exp_avg),
                 (tr.opt.exp_avg_sq, twin.opt.exp_avg_sq), (tr.opt.scalars, twin.opt.scalars)):
        assert torch.equal(a, b)
    assert float(tr.opt.steps) == 2.0
    sd = tr.state_dict()
    assert sd["format"] == 1 and set(sd) == {"format", "model", "ema", "optimizer"}  # the count is not saved


def test_the_default_makes_the_unguarded_call_and_is_poisoned(cuda, dataset, monkeypatch):
    tr = make_trainer(cuda)
    assert tr.opt.guard is None and tr.opt.skip_nonfinite is False
    with pytest.raises(ValueError):
        tr.opt.skipped
    seen = record_optim_calls(monkeypatch)
    tr.step(dataset.batch(BATCHES[0]))
    assert seen == ["x2g_clip_adam_ema_ex"]
    tr.forward_backward(dataset.batch(BATCHES[1]))
    tr.bucket.flat[17] = float("inf")
    tr.update()
    assert not bool(torch.isfinite(tr.opt.flat).all())  # what the guard is for


def test_the_guarded_trainer_calls_the_guard_entry_only(cuda, dataset, monkeypatch):
    tr = make_trainer(cuda, skip_nonfinite=True)
    seen = record_optim_calls(monkeypatch)
    tr.step(dataset.batch(BATCHES[0]))
    assert seen == ["x2g_clip_adam_ema_guard"]
    assert tr.opt.guard.tolist() == [0, 0]
    assert bool(torch.isfinite(tr.opt.flat).all())
