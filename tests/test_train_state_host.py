"""Host-side halves of the evaluation support, no GPU: the parameter swap (optim.swap_params /
FlatAdam.averaged) and the trainer's state round trip, on a small CPU-resident model (nothing is launched: the
flat buffers, the views and the name-keyed state are plain tensor bookkeeping)."""
import io

import pytest
import torch

CFG = dict(conv_layers=1, sbf_dim=7, rbf_dim=6, in_channels=32, heads=4, embedding_size=32)
SCHEDULE = dict(warmup_steps=2, decay_steps=4, decay_rate=0.5)


def make_trainer(seed):
    import x2gnn

    torch.manual_seed(seed)
    return x2gnn.Trainer(x2gnn.xgnn_poly(**CFG), lr_schedule=SCHEDULE)


def scramble(tr, seed):
    """Distinct values in every optimizer buffer (as after some steps); the alignment padding between the
    parameters stays zero, as the update kernel leaves it."""
    g = torch.Generator().manual_seed(seed)
    for t in (tr.opt.ema, tr.opt.exp_avg, tr.opt.exp_avg_sq):
        for p, off in zip(tr.opt.params, tr.opt.offsets):
            t[off:off + p.numel()].copy_(torch.rand(p.numel(), generator=g))
    tr.opt.scalars[6] = 5.0  # the step count


def test_swap_reads_the_average_in_place_and_restores():
    tr = make_trainer(0)
    opt = tr.opt
    scramble(tr, 1)
    grads = [p.grad.data_ptr() for p in opt.params]
    tr.model.eval()
    with pytest.raises(RuntimeError, match="inside"):
        with tr.averaged():
            for p, off, v in zip(opt.params, opt.offsets, opt.ema_params()):
                assert p.data_ptr() == opt.ema.data_ptr() + 4 * off and torch.equal(p, v)
                assert p.requires_grad and p._x2g_grad_sink is True
            tr.model.train()
            raise RuntimeError("inside")
    assert not tr.model.training
    for p, off, g in zip(opt.params, opt.offsets, grads):
        assert p.data_ptr() == opt.flat.data_ptr() + 4 * off
        assert p.grad.data_ptr() == g == tr.bucket.flat.data_ptr() + 4 * off
        assert p._x2g_grad_sink is True


def test_swap_refuses_other_shapes():
    from x2gnn.optim import swap_params

    tr = make_trainer(0)
    vals = tr.opt.ema_params()
    with pytest.raises(ValueError):
        with swap_params(tr.opt.params, vals[:-1]):
            pass
    vals[0] = vals[0].reshape(-1)[:1]
    with pytest.raises(ValueError):
        with swap_params(tr.opt.params, vals):
            pass
    assert tr.opt.params[0].data_ptr() == tr.opt.flat.data_ptr()


def test_state_round_trip_by_name():
    import x2gnn

    a, b = make_trainer(0), make_trainer(1)
    scramble(a, 2)
    buf = io.BytesIO()
    torch.save(a.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf)
    assert sd["format"] == 1 and set(sd) == {"format", "model", "ema", "optimizer"}
    assert set(sd["model"]) == set(sd["ema"]) == set(a.model.state_dict())
    names = {n for n, p in a.model.named_parameters() if p.requires_grad}
    assert set(sd["optimizer"]["exp_avg"]) == set(sd["optimizer"]["exp_avg_sq"]) == names
    # clones: the state does not alias the live buffers
    live, ema = a.state_dict(), a.opt.ema.clone()
    a.opt.ema.add_(1.0)
    name = next(iter(names))
    assert not torch.equal(live["ema"][name], a.state_dict()["ema"][name])
    a.opt.ema.copy_(ema)

    def buffers(tr):
        o = tr.opt
        return o.flat, o.ema, o.exp_avg, o.exp_avg_sq, o.scalars

    assert not torch.equal(a.opt.flat, b.opt.flat)
    held = [t.data_ptr() for t in buffers(b)]
    b.load_state_dict(sd)
    assert held == [t.data_ptr() for t in buffers(b)]  # copied into the buffers: nothing is rebound
    for x, y in zip(buffers(a), buffers(b)):
        assert torch.equal(x, y)
    for p, off in zip(b.opt.params, b.opt.offsets):
        assert p.data_ptr() == b.opt.flat.data_ptr() + 4 * off

    before = [t.clone() for t in buffers(b)]
    with pytest.raises(KeyError):
        b.load_state_dict({**sd, "model": {k: v for k, v in sd["model"].items() if k != name}})
    with pytest.raises(KeyError):
        b.load_state_dict({**sd, "ema": {**sd["ema"], "no.such.weight": sd["ema"][name]}})
    bad = {**sd["optimizer"], "exp_avg_sq": {k: v.reshape(-1)[:1] for k, v in sd["optimizer"]["exp_avg_sq"].items()}}
    with pytest.raises(ValueError):
        b.load_state_dict({**sd, "optimizer": bad})
    with pytest.raises(ValueError):
        b.load_state_dict({**sd, "format": 2})
    for x, y in zip(before, buffers(b)):  # a refused state changes nothing
        assert torch.equal(x, y)

    fresh = x2gnn.xgnn_poly(**CFG)
    fresh.load_state_dict(sd["ema"], strict=True)
    got = dict(fresh.named_parameters())
    for n, v in zip([n for n, p in a.model.named_parameters() if p.requires_grad], a.opt.ema_params()):
        assert torch.equal(got[n], v)
