"""x2g_error_accum / x2g_weighted_accum refuse bad arguments on the host, before any launch (no GPU needed)."""
import ctypes

import pytest

EINVAL = 1001
P = ctypes.c_void_p(16)  # a plausible pointer, never dereferenced: every case below fails a host check first
MISALIGNED = ctypes.c_void_p(12)  # not 8-byte aligned


@pytest.fixture(scope="module")
def lib():
    from x2gnn import _lib

    return _lib.load()


@pytest.mark.parametrize("n", [0, -1])
def test_error_accum_refuses_no_elements(lib, n):
    assert lib.x2g_error_accum(P, P, n, P, None) == EINVAL


@pytest.mark.parametrize("args", [(None, P, 4, P), (P, None, 4, P), (P, P, 4, None), (P, P, 4, MISALIGNED)],
                         ids=["pred", "target", "acc", "acc_misaligned"])
def test_error_accum_refuses_bad_pointers(lib, args):
    assert lib.x2g_error_accum(*args, None) == EINVAL


@pytest.mark.parametrize("args", [(None, 2.0, P), (P, 2.0, None), (P, 2.0, MISALIGNED)],
                         ids=["value", "acc", "acc_misaligned"])
def test_weighted_accum_refuses_bad_pointers(lib, args):
    assert lib.x2g_weighted_accum(*args, None) == EINVAL
