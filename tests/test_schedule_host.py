"""schedule.Plateau against torch.optim.lr_scheduler.ReduceLROnPlateau(mode='min', threshold_mode='rel') on a dummy
SGD: the learning-rate sequences must be ==."""
import numpy as np
import pytest
import torch


class StubOpt:
    """What Plateau needs of a FlatAdam: ``lr`` and ``set_lr``."""

    def __init__(self, lr):
        self.lr = lr
        self.calls = []

    def set_lr(self, lr):
        self.lr = lr
        self.calls.append(lr)


def torch_sequence(values, lr, **kw):
    p = torch.nn.Parameter(torch.zeros(1))
    sgd = torch.optim.SGD([p], lr=lr)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(sgd, mode="min", threshold_mode="rel", **kw)
    out = []
    for v in values:
        sched.step(v)
        out.append(sgd.param_groups[0]["lr"])
    return out


def plateau_sequence(values, lr, **kw):
    from x2gnn.schedule import Plateau

    opt = StubOpt(lr)
    sched = Plateau(opt, **kw)
    out = []
    for v in values:
        got = sched.step(v)
        assert got == sched.lr == opt.lr  # every reduction went through set_lr
        out.append(opt.lr)
    return out, opt


def test_the_fixed_sequence():
    values = [1.0, .9, .9, .90005, .9, .9, .8, .8, .8, .8, .8, .8, .8]
    kw = dict(factor=0.5, patience=2, min_lr=1e-5)
    want = [1e-3] * 4 + [5e-4] * 5 + [2.5e-4] * 3 + [1.25e-4]
    assert torch_sequence(values, 1e-3, **kw) == want
    got, opt = plateau_sequence(values, 1e-3, **kw)
    assert got == want
    assert opt.calls == [5e-4, 2.5e-4, 1.25e-4]


def random_values(seed=7, n=200):
    rng = np.random.default_rng(seed)
    v = np.round(1.0 - 0.002 * np.arange(n) + 0.05 * rng.standard_normal(n), 2)  # two decimals: many exact ties
    assert len(set(v.tolist())) < n
    return [float(x) for x in v]


@pytest.mark.parametrize("cooldown", [0, 3])
@pytest.mark.parametrize("patience", [0, 2, 10])
@pytest.mark.parametrize("factor", [0.5, 0.1])
def test_a_random_sequence_with_ties(factor, patience, cooldown):
    values = random_values()
    kw = dict(factor=factor, patience=patience, min_lr=1e-5, cooldown=cooldown)
    want = torch_sequence(values, 1e-3, **kw)
    got, _ = plateau_sequence(values, 1e-3, **kw)
    assert got == want
    if patience == 0:
        assert want[-1] == 1e-5  # the floor is reached
        assert len(set(want)) > 2


def test_a_state_dict_round_trip_mid_sequence_continues_identically():
    from x2gnn.schedule import Plateau

    values = random_values(seed=9)
    kw = dict(factor=0.5, patience=2, min_lr=1e-5, cooldown=1)
    want, _ = plateau_sequence(values, 1e-3, **kw)
    opt = StubOpt(1e-3)
    first = Plateau(opt, **kw)
    for v in values[:77]:
        first.step(v)
    sd = first.state_dict()
    assert all(isinstance(x, (int, float)) for x in sd.values())
    opt2 = StubOpt(opt.lr)  # (the optimizer's own rate comes back with the trainer's state)
    second = Plateau(opt2, lr=123.0, **kw)
    second.load_state_dict(sd)
    got = []
    for v in values[77:]:
        second.step(v)
        got.append(opt2.lr)
    assert got == want[77:]
    with pytest.raises(KeyError):
        second.load_state_dict({"lr": 1.0})


def test_the_reference_call_without_a_metric_cannot_run():
    """trainer.py:47 calls scheduler.step() per batch with no metric: for ReduceLROnPlateau that is a TypeError, so
    the reference's plateau branch never ran as written (why Plateau steps per epoch on the validation error)."""
    p = torch.nn.Parameter(torch.zeros(1))
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(torch.optim.SGD([p], lr=1e-3))
    with pytest.raises(TypeError):
        sched.step()
