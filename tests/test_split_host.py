"""datasets.split_indices: the reference's permutation and cuts (trainer.py:22-27) without numpy's global state."""
import numpy as np
import pytest


@pytest.mark.parametrize("seed", [0, 41])
@pytest.mark.parametrize("n,division", [(10, (2, 5)), (1000, (100, 200))])
def test_equals_the_global_state_form(n, division, seed):
    from x2gnn.datasets import split_indices

    state = np.random.get_state()
    try:
        np.random.seed(seed)
        perm = np.random.permutation(n)  # trainer.py:22-23
    finally:
        np.random.set_state(state)
    test, val, train = split_indices(n, division, seed)
    assert all(p.dtype == np.int64 for p in (test, val, train))
    np.testing.assert_array_equal(test, perm[:division[0]])
    np.testing.assert_array_equal(val, perm[division[0]:division[1]])
    np.testing.assert_array_equal(train, perm[division[1]:])
    parts = np.concatenate([test, val, train])
    assert len(parts) == n and sorted(parts.tolist()) == list(range(n))  # disjoint, and they cover range(n)


def test_numpys_global_generator_is_not_touched():
    from x2gnn.datasets import split_indices

    state = np.random.get_state()
    try:
        np.random.seed(123)
        want = np.random.random(4), np.random.random(4)
        np.random.seed(123)
        first = np.random.random(4)
        split_indices(1000, (100, 200), 41)
        second = np.random.random(4)
    finally:
        np.random.set_state(state)
    np.testing.assert_array_equal(first, want[0])
    np.testing.assert_array_equal(second, want[1])


def test_a_division_that_does_not_fit_raises():
    from x2gnn.datasets import split_indices

    with pytest.raises(ValueError):
        split_indices(10, (5, 2), 0)
    with pytest.raises(ValueError):
        split_indices(10, (2, 11), 0)
