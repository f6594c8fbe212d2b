"""x2g_error_accum / x2g_weighted_accum through the raw C ABI against fp64 numpy.

The error kernel is one 256-thread workgroup: per-thread strided sums, a wave butterfly, the waves in index
order.  It can go wrong at one lane, at the wave edges, with fewer elements than threads and in the strided
loop's tail, so those are the sizes.  Bound on the two sums: every term is non-negative, each of the at most n
fp64 additions rounds once by at most 2^-53 of a running sum that never exceeds the total, and numpy's own
summation carries the same bound, so |got - ref| <= n * 2^-52 * ref; d^2 is exact in fp64 (a 24-bit significand
squared).  The maximum and the count are exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000]
SENTINEL = -12345.678
EPS = 2.0 ** -52


def draw(n, seed):
    """pred / target (fp32) with magnitudes and differences spread over about 1e-3 .. 1e3, and exact ties
    (d = 0) at every index = 3 mod 7."""
    rng = np.random.default_rng(seed)
    pred = (10.0 ** rng.uniform(-3, 3, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    target = (pred + 10.0 ** rng.uniform(-3, 3, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    target[3::7] = pred[3::7]
    return pred, target


def reference(pred, target):
    """fp64 statistics of d = pred - target ROUNDED TO FLOAT32 FIRST (as torch forms it)."""
    d = pred - target
    assert d.dtype == np.float32
    a = np.abs(d).astype(np.float64)
    return float(a.sum()), float((a * a).sum()), float(a.max()), float(len(a))


def accumulate(cuda, calls, seed_acc=(0.0, 0.0, 0.0, 0.0)):
    """x2g_error_accum per (pred, target) of ``calls`` into the first 4 of 8 doubles; returns all 8 (host)."""
    from x2gnn._lib import call, ptr, stream_ptr

    buf = torch.tensor(list(seed_acc) + [SENTINEL] * 4, dtype=torch.float64, device=cuda)
    keep = []
    for pred, target in calls:
        p, t = torch.from_numpy(pred).to(cuda), torch.from_numpy(target).to(cuda)
        keep.append((p, t))
        call("x2g_error_accum", ptr(p), ptr(t), p.numel(), ptr(buf), stream_ptr())
    return buf.cpu().numpy()


@pytest.mark.parametrize("n", SIZES)
def test_error_accum_against_fp64(cuda, n):
    pred, target = draw(n, seed=100 + n)
    if n >= 7:
        assert (pred == target).any() and (pred != target).any()
    r_abs, r_sq, r_max, r_n = reference(pred, target)
    got = accumulate(cuda, [(pred, target)])
    print(f"n={n}: sum|d| {got[0]!r} ref {r_abs!r}; sum d^2 {got[1]!r} ref {r_sq!r}; max {got[2]!r}; n {got[3]!r}")
    assert abs(got[0] - r_abs) <= n * EPS * r_abs
    assert abs(got[1] - r_sq) <= n * EPS * r_sq
    assert got[2] == r_max and got[3] == r_n
    assert (got[4:] == SENTINEL).all()  # the doubles behind the accumulator are not touched
    again = accumulate(cuda, [(pred, target)])
    assert got.tobytes() == again.tobytes()  # fixed summation order: identical bits


def test_error_accum_adds_to_a_running_accumulator(cuda):
    """Three calls of different n into one accumulator that starts non-zero: the seeds plus the three
    references, under the sums' bound with n = all elements (each call's last addition, into the accumulator,
    takes the place of the one a lone sum of n terms does not make); the maximum is the maximum of all."""
    seed_acc = (1.5, 2.25, 0.125, 3.0)
    calls = [draw(n, seed=7 + n) for n in (65, 1000, 2)]
    refs = [reference(p, t) for p, t in calls]
    n = sum(len(p) for p, _ in calls)
    got = accumulate(cuda, calls, seed_acc)
    want_abs = seed_acc[0] + sum(r[0] for r in refs)
    want_sq = seed_acc[1] + sum(r[1] for r in refs)
    print(f"sum|d| {got[0]!r} ref {want_abs!r}; sum d^2 {got[1]!r} ref {want_sq!r}")
    assert abs(got[0] - want_abs) <= n * EPS * want_abs
    assert abs(got[1] - want_sq) <= n * EPS * want_sq
    assert got[2] == max([seed_acc[2]] + [r[2] for r in refs])
    assert got[3] == seed_acc[3] + n
    assert (got[4:] == SENTINEL).all()
    # a running maximum larger than every batch's is kept
    big = accumulate(cuda, calls[:1], (0.0, 0.0, 1e9, 0.0))
    assert big[2] == 1e9


def test_weighted_accum_equals_the_python_float_loop_exactly(cuda):
    """acc[0] += w * value, acc[1] += w over five fp32 values with integer weights up to 2^20 equals the Python
    ``float`` loop bit for bit: an fp32 value (24-bit significand) times an integer below 2^29 is exact in fp64,
    so a fused multiply-add and a multiply followed by an add round the same single time."""
    from x2gnn._lib import call, ptr, stream_ptr

    rng = np.random.default_rng(5)
    values = (10.0 ** rng.uniform(-3, 3, 5) * rng.choice([-1.0, 1.0], 5)).astype(np.float32)
    weights = [1, 128, 4097, 2 ** 20, 37]
    v = torch.from_numpy(values).to(cuda)
    buf = torch.tensor([0.0, 0.0, SENTINEL, SENTINEL], dtype=torch.float64, device=cuda)
    a = c = 0.0
    for i, w in enumerate(weights):
        call("x2g_weighted_accum", ptr(v[i:i + 1]), float(w), ptr(buf), stream_ptr())
        a += w * float(values[i])
        c += w
    got = buf.cpu().numpy()
    assert got[0] == a and got[1] == c
    assert (got[2:] == SENTINEL).all()


def test_ops_wrappers(cuda):
    """ops.error_accum treats [B] and [B, 1] alike and checks its arguments; ops.weighted_accum likewise."""
    from x2gnn import ops

    pred, target = draw(65, seed=3)
    r = reference(pred, target)
    p, t = torch.from_numpy(pred).to(cuda), torch.from_numpy(target).to(cuda)
    acc = torch.zeros(4, dtype=torch.float64, device=cuda)
    ops.error_accum(p, t.reshape(-1, 1), acc)
    got = acc.cpu().numpy()
    assert abs(got[0] - r[0]) <= 65 * EPS * r[0] and got[2] == r[2] and got[3] == 65.0
    assert got.tobytes() == accumulate(cuda, [(pred, target)])[:4].tobytes()
    with pytest.raises(ValueError):
        ops.error_accum(p, t, acc.float())
    with pytest.raises(ValueError):
        ops.error_accum(p, t, acc[:3])
    with pytest.raises(ValueError):
        ops.error_accum(p, t[:64], acc)
    with pytest.raises(ValueError):
        ops.error_accum(p.double(), t, acc)
    w = torch.zeros(2, dtype=torch.float64, device=cuda)
    ops.weighted_accum(p[0], 3, w)
    assert w.cpu().tolist() == [3 * float(pred[0]), 3.0]
    with pytest.raises(ValueError):
        ops.weighted_accum(p[:2], 3, w)
    with pytest.raises(ValueError):
        ops.weighted_accum(p[0], 3, w[:1])
