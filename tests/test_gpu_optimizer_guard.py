"""The guarded parameter update (x2g_clip_adam_ema_guard, include/x2g_train.h) on flat buffers, through the raw ABI.

A finite norm: bit for bit the unguarded entry's outputs.  A non-finite norm (an inf element, a NaN element, finite
elements whose squares overflow fp32): parameters, moments, average, step count and schedule untouched, the norm
published, clip 0, the gradients still zeroed when asked, the guard words set.  Eager and captured.

The sizes: 1 and 3 (the n % 4 tail alone, summed by block 0), 5 (a tail and one float4), 1024 and 1027 (fewer
float4s than the 256 norm blocks: ``per`` = 1, most blocks empty), 262147 (``per`` = 256 exactly, every thread of
every block one float4, plus a tail of 3; 1025 update blocks)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 5, 1024, 1027, 262147]
POISONS = ["inf", "nan", "overflow"]


def consts():
    from x2gnn import _lib

    return _lib.CONSTS


class Buffers:
    """params, grads, both moments, the average and the scalar block of one optimizer, seeded."""

    def __init__(self, n, max_norm, cuda, seed=0):
        c = consts()
        g = torch.Generator().manual_seed(seed)
        self.n = n
        self.params = torch.randn(n, generator=g).to(cuda)
        self.grads = torch.zeros(n, device=cuda)
        self.exp_avg = torch.zeros(n, device=cuda)
        self.exp_avg_sq = torch.zeros(n, device=cuda)
        self.ema = self.params.clone()
        sc = torch.zeros(16)
        for k, v in (("LR", 1e-3), ("BETA1", 0.9), ("BETA2", 0.999), ("EPS", 1e-8), ("MAX_NORM", max_norm),
                     ("EMA_DECAY", 0.95), ("WARMUP", 3.0), ("DECAY_STEPS", 10.0), ("DECAY_RATE", 0.5),
                     ("BASE_LR", 1e-3), ("STAIRCASE", 0.0)):
            sc[c["OPT_" + k]] = v
        self.scalars = sc.to(cuda)
        self.guard = torch.zeros(2, dtype=torch.int64, device=cuda)
        self.ws = torch.empty(2048, dtype=torch.uint8, device=cuda)

    def tensors(self):
        return (self.params, self.grads, self.exp_avg, self.exp_avg_sq, self.ema, self.scalars)

    def clone(self):
        new = object.__new__(Buffers)
        new.n = self.n
        for k in ("params", "grads", "exp_avg", "exp_avg_sq", "ema", "scalars", "guard", "ws"):
            setattr(new, k, getattr(self, k).clone())
        return new

    def step(self, grads, guarded, zero):
        from x2gnn import _lib
        from x2gnn._lib import call, ptr, stream_ptr

        self.grads.copy_(grads)
        flags = consts()["OPT_ZERO_GRADS"] if zero else 0
        lib = _lib.load()
        head = (ptr(self.params), ptr(self.grads), ptr(self.exp_avg), ptr(self.exp_avg_sq), ptr(self.ema), self.n,
                ptr(self.scalars), flags)
        if guarded:
            call("x2g_clip_adam_ema_guard", *head, ptr(self.guard), ptr(self.ws),
                 int(lib.x2g_optimizer_guard_workspace(self.n)), stream_ptr())
        else:
            call("x2g_clip_adam_ema_ex", *head, ptr(self.ws), int(lib.x2g_optimizer_workspace(self.n)), stream_ptr())


def bits(t):
    return t.view(torch.int32)


def same(a, b):
    """Every buffer and all 16 scalars, bit for bit (NaN-proof)."""
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a.tensors(), b.tensors()))


def finite_grads(n, cuda, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(100 + seed)).to(cuda)


def poisoned(g, kind, pos):
    g = g.clone()
    if kind == "inf":
        g[pos] = float("inf")
    elif kind == "nan":
        g[pos] = float("nan")
    else:  # finite, and the sum of squares overflows fp32 (3e19^2 = 9e38 > 3.4e38)
        g[pos] = 3e19
        g[(pos + 1) % g.numel()] = 3e19
    return g


def positions(n):
    return sorted({0, n // 2, n - 1})


@pytest.mark.parametrize("zero", [False, True])
@pytest.mark.parametrize("max_norm", [100.0, 0.05])
@pytest.mark.parametrize("n", SIZES)
def test_finite_steps_equal_the_unguarded_entry(cuda, n, max_norm, zero):
    a = Buffers(n, max_norm, cuda)
    b = a.clone()
    for s in range(3):
        g = finite_grads(n, cuda, s)
        a.step(g, guarded=True, zero=zero)
        b.step(g, guarded=False, zero=zero)
        assert same(a, b), s
        assert a.guard.tolist() == [0, 0]
    c = consts()
    assert float(a.scalars[c["OPT_STEP"]]) == 3.0
    assert bool((a.grads == 0).all()) == zero


@pytest.mark.parametrize("zero", [False, True])
@pytest.mark.parametrize("max_norm", [100.0, 0.05])
@pytest.mark.parametrize("n", SIZES)
def test_a_poisoned_step_is_skipped(cuda, n, max_norm, zero):
    c = consts()
    kept_slots = [c["OPT_" + k] for k in ("STEP", "LR", "STEP_SIZE", "BC2_SQRT")]
    base = Buffers(n, max_norm, cuda)
    base.step(finite_grads(n, cuda, 0), guarded=True, zero=zero)  # moments, average and schedule under way
    g_next = finite_grads(n, cuda, 2)
    want = base.clone()
    want.step(g_next, guarded=False, zero=zero)  # the unguarded step from the pre-poison state
    for kind in POISONS:
        for pos in positions(n):
            a = base.clone()
            bad = poisoned(finite_grads(n, cuda, 1), kind, pos)
            a.step(bad, guarded=True, zero=zero)
            for got, was in ((a.params, base.params), (a.exp_avg, base.exp_avg), (a.exp_avg_sq, base.exp_avg_sq),
                             (a.ema, base.ema)):
                assert torch.equal(bits(got), bits(was)), (kind, pos)
            assert torch.equal(bits(a.scalars[kept_slots]), bits(base.scalars[kept_slots])), (kind, pos)
            norm = float(a.scalars[c["OPT_NORM"]])
            assert norm != norm if kind == "nan" else norm == float("inf"), (kind, pos, norm)
            assert float(a.scalars[c["OPT_CLIP"]]) == 0.0
            hyper = [c["OPT_" + k] for k in ("BETA1", "BETA2", "EPS", "MAX_NORM", "EMA_DECAY", "WARMUP", "DECAY_STEPS",
                                             "DECAY_RATE", "BASE_LR", "STAIRCASE")]
            assert torch.equal(a.scalars[hyper], base.scalars[hyper])
            if zero:
                assert bool((a.grads == 0).all()), (kind, pos)
            else:
                assert torch.equal(bits(a.grads), bits(bad)), (kind, pos)
            assert a.guard.tolist() == [1, 1], (kind, pos)
            # the next, finite step is the unguarded step from the pre-poison state
            a.step(g_next, guarded=True, zero=zero)
            assert same(a, want), (kind, pos)
            assert a.guard.tolist() == [1, 0], (kind, pos)


@pytest.mark.parametrize("n", [3, 1027])
def test_a_skipped_first_step_leaves_the_first_update_copy_to_the_next(cuda, n):
    c = consts()
    a = Buffers(n, 100.0, cuda)
    a.ema.fill_(7.0)  # (not the parameters: the first counted step must overwrite it with them)
    a.step(poisoned(finite_grads(n, cuda, 0), "inf", n - 1), guarded=True, zero=True)
    assert a.guard.tolist() == [1, 1] and float(a.scalars[c["OPT_STEP"]]) == 0.0
    assert bool((a.ema == 7.0).all())
    a.step(finite_grads(n, cuda, 1), guarded=True, zero=True)
    assert float(a.scalars[c["OPT_STEP"]]) == 1.0 and a.guard.tolist() == [1, 0]
    assert torch.equal(bits(a.ema), bits(a.params))
    a.step(finite_grads(n, cuda, 2), guarded=True, zero=True)
    assert not torch.equal(a.ema, a.params)  # from the second counted step on it is the average


@pytest.mark.parametrize("n", [5, 262147])
def test_one_captured_graph_replayed_finite_poisoned_finite(cuda, n):
    c = consts()
    seq = [finite_grads(n, cuda, 0), poisoned(finite_grads(n, cuda, 1), "nan", n // 2), finite_grads(n, cuda, 2)]
    eager = Buffers(n, 0.05, cuda)
    a = eager.clone()
    for g in seq:  # (also loads the kernels before the capture)
        eager.step(g, guarded=True, zero=True)
    stage = torch.zeros(n, device=cuda)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a.step(stage, guarded=True, zero=True)
    for g in seq:
        stage.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    assert same(a, eager)
    assert a.guard.tolist() == eager.guard.tolist() == [1, 0]
    # two steps counted: the schedule's rate is the one of t = 1 (warmup 3: base * 2 / 3, decay 0.5^(1 / 10))
    assert float(a.scalars[c["OPT_STEP"]]) == 2.0
    want_lr = torch.tensor(1e-3, dtype=torch.float32).double().item() * (2.0 / 3.0) * 0.5 ** 0.1
    assert abs(float(a.scalars[c["OPT_LR"]]) - want_lr) <= 2.0 ** -23 * want_lr
