"""The edge features from AO matrices (include/x2g_features.h, csrc/ao_features.hip) stated in float64 with plain numpy
loops, written from the operation's definition and not from the kernel: the oracle of tests/test_ao_features_ref.py
(against what the reference itself recorded, tests/golden/ao_features.npz) and of tests/test_gpu_ao_features.py.

For the edge (i, j) and each matrix M of (S, H / nelectron):
  1. B = M[ao_i0:ao_i1, ao_j0:ao_j1], shape (r, c); r or c above 39 raises, as the reference does.
  2. Every element is rounded to float32 (after the float64 division for H).
  3. B goes into a zero 39 x 39 pad P at (0, 2) when (r, c) == (39, 9), at (2, 2) when (r, c) == (9, 9), and at (0, 0)
     for every other shape, (9, 39) included (the reference's branch for that shape is never taken).
  4. 13 index groups of 0..38, for rows and columns alike (GROUPS).
  5. f[a, b] = P[a, b] where both groups are one index, else the Frobenius norm of P[rows(a), cols(b)]: squares summed
     in float64, row-major inside the sub-block, then a float64 square root.
  6. row = concat(f_S.reshape(169), f_H.reshape(169)).

``edge_features`` returns the rows in float64 WITHOUT the final rounding to float32, so that a float32 result can be
held to one rounding of it.  ``variant`` names one deliberate error a kernel could make (WRONG); the tests show that
each misses the reference's recorded rows by far more than the bound.
"""
import numpy as np

PAD = 39
GROUPS = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 8), (8, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 32),
          (32, 39)]
G = len(GROUPS)
CELLS = G * G
ROW = 2 * CELLS

WRONG = ("quirk_repaired", "cells_transposed", "halves_swapped", "single_as_norm", "no_division", "f_group_short")


def single_mask():
    """bool [338]: the cells that are one signed element (both groups a single index)."""
    one = np.array([hi - lo == 1 for lo, hi in GROUPS])
    m = one[:, None] & one[None, :]
    return np.concatenate([m.reshape(-1), m.reshape(-1)])


def placement(r, c, variant=None):
    if (r, c) == (39, 9):
        return 0, 2
    if (r, c) == (9, 9):
        return 2, 2
    if variant == "quirk_repaired" and (r, c) == (9, 39):
        return 2, 0
    return 0, 0


def matrix_cells(M, ri, rj, div, variant=None):
    """float64 [13, 13] of one matrix and one edge (AO ranges ``ri``, ``rj``)."""
    B = np.asarray(M, np.float64)[ri[0]:ri[1], rj[0]:rj[1]]
    r, c = B.shape
    if r > PAD or c > PAD:
        raise ValueError(f"a block of {r} x {c} does not fit the {PAD} x {PAD} pad")
    if div is not None and variant != "no_division":
        B = B / np.float64(div)
    P = np.zeros((PAD, PAD), np.float64)
    r0, c0 = placement(r, c, variant)
    P[r0:r0 + r, c0:c0 + c] = B.astype(np.float32).astype(np.float64)
    groups = list(GROUPS)
    if variant == "f_group_short":
        groups[-1] = (32, 38)
    f = np.zeros((G, G), np.float64)
    for a, (a0, a1) in enumerate(groups):
        for b, (b0, b1) in enumerate(groups):
            if a1 - a0 == 1 and b1 - b0 == 1 and variant != "single_as_norm":
                f[a, b] = P[a0, b0]
                continue
            s = np.float64(0.0)
            for p in range(a0, a1):
                for q in range(b0, b1):
                    s += P[p, q] * P[p, q]
            f[a, b] = np.sqrt(s)
    return f.T if variant == "cells_transposed" else f


def edge_features(S, H, aoslice, edge_index, nelectron=None, variant=None):
    """float64 [E, 338].  ``aoslice`` [n_atoms, 4] (columns 2, 3: AO begin, end); ``edge_index`` [2, E];
    ``nelectron``: H is divided by it in float64 first (None: H is taken as it is)."""
    aoslice, edge_index = np.asarray(aoslice), np.asarray(edge_index)
    out = np.zeros((edge_index.shape[1], ROW), np.float64)
    for e, (i, j) in enumerate(edge_index.T):
        ri, rj = aoslice[i, 2:4], aoslice[j, 2:4]
        fs = matrix_cells(S, ri, rj, None, variant).reshape(-1)
        fh = matrix_cells(H, ri, rj, nelectron, variant).reshape(-1)
        out[e] = np.concatenate([fh, fs] if variant == "halves_swapped" else [fs, fh])
    return out


# ------------------------------------------------------------------------------------------------- seeded inputs
def aoslice_of(counts):
    """[n, 4] int64 like pyscf's ``aoslice_by_atom()`` for atoms of ``counts`` functions each (the shell columns 0
    and 1 are not used by the operation: atom indices stand in)."""
    ends = np.cumsum(counts)
    begins = ends - np.asarray(counts)
    idx = np.arange(len(counts))
    return np.stack([idx, idx + 1, begins, ends], axis=1).astype(np.int64)


def random_symmetric(rng, n, lo=-6.0, hi=1.0):
    """Symmetric float64 [n, n] with signed entries whose magnitudes are log-uniform over [10^lo, 10^hi]."""
    A = rng.choice([-1.0, 1.0], size=(n, n)) * 10.0 ** rng.uniform(lo, hi, size=(n, n))
    return np.triu(A) + np.triu(A, 1).T


def all_directed_edges(n, self_loops=False):
    return np.array([[i, j] for i in range(n) for j in range(n) if self_loops or i != j], np.int64).T.reshape(2, -1)
