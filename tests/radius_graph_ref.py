"""The radius graph (include/x2g_graph.h, csrc/radius_graph.hip) stated in float64, written from the operation's
definition and not from the kernel: the oracle of tests/test_radius_graph_ref.py (against the host's float32 form,
``datasets.bonds(datasets.distance_matrix(R))``) and of tests/test_gpu_radius_graph.py.

Statement.  With R the float64 copies of the float32 positions of one molecule, d(i, j) = |R_i - R_j|; the ordered
pair (i, j), i != j, is an edge iff 0 < d < cutoff; an atom with a non-finite coordinate has no edge; the edges are
listed in argwhere (row-major) order with molecule-local ids, the molecules end to end.

Band.  The float32 Gram form the reference and the kernel evaluate is d2 = (g_ii + g_jj) - 2 g_ij with g a three-term
dot product.  With u = 2^-24 each product and each partial sum is rounded once, so a dot product of vectors a, b is
off by at most about 3 u |a| |b|; g_ii, g_jj and 2 g_ij together by 3 u (|R_i|^2 + |R_j|^2 + 2 |R_i| |R_j|) =
3 u (|R_i| + |R_j|)^2, the sum g_ii + g_jj adds u (|R_i|^2 + |R_j|^2) <= u (|R_i| + |R_j|)^2, and the final
subtraction u d^2:
    |d2_f32 - d^2| <= 4 u (|R_i| + |R_j|)^2 + u d^2.
The square root turns an error e in d^2 into e / (2 d); at d ~ cutoff = 5 that is
    (4 u (|R_i| + |R_j|)^2 + 25 u) / 10 = 0.4 u (|R_i| + |R_j|)^2 + 2.5 u,
and the rounding of the root itself adds 5 u.  The band below, u (|R_i| + |R_j|)^2 + 2^-20 = u (|R_i| + |R_j|)^2 +
16 u, covers both with a factor of two to spare.  A pair is *decided* when |d - cutoff| > band: there every correct
float32 evaluation of the Gram form has to agree with float64.  Undecided pairs may go either way (the result has to
stay symmetric); how many of them a fixture may hold is capped in FIXTURES, and the tests assert the cap.

``variant`` names one deliberate error an implementation could make (WRONG); tests/test_radius_graph_ref.py shows
that each differs from the statement on the exact lattice fixture.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24
CUTOFF = 5.0

WRONG = ("less_or_equal", "self_loops", "coincident_bonded", "column_major", "global_ids")


def distances(R):
    """float64 [n, n] of float32 (or exact) positions [n, 3]."""
    R = np.asarray(R).astype(np.float64).reshape(-1, 3)
    diff = R[:, None, :] - R[None, :, :]
    return np.sqrt((diff * diff).sum(-1))


def band(R):
    """float64 [n, n]: band_ij = 2^-24 (|R_i| + |R_j|)^2 + 2^-20."""
    norm = np.sqrt((np.asarray(R).astype(np.float64).reshape(-1, 3) ** 2).sum(-1))
    return U * (norm[:, None] + norm[None, :]) ** 2 + 2.0 ** -20


def adjacency(R, cutoff=CUTOFF, variant=None):
    """bool [n, n]: the statement's edges of one molecule."""
    R = np.asarray(R).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        d = distances(R)
        adj = (d <= cutoff) if variant == "less_or_equal" else (d < cutoff)
        if variant != "coincident_bonded":
            adj &= d > 0
    off = ~np.eye(len(R), dtype=bool)
    if variant != "self_loops":
        adj &= off
    else:
        adj |= ~off
    finite = np.isfinite(R.astype(np.float64)).all(-1)
    return adj & finite[:, None] & finite[None, :]


def decided(R, cutoff=CUTOFF):
    """bool [n, n]: the ordered pairs i != j whose distance is further from the cutoff than the band."""
    with np.errstate(invalid="ignore"):
        far = np.abs(distances(R) - cutoff) > band(R)
    return far & ~np.eye(len(np.asarray(R).reshape(-1, 3)), dtype=bool)


def edges_of(adj, variant=None):
    """int64 [2, E] of a bool adjacency, argwhere order."""
    if variant == "column_major":
        return np.argwhere(adj.T).T[::-1].astype(np.int64).reshape(2, -1)
    return np.argwhere(adj).T.astype(np.int64).reshape(2, -1)


def graph(mols, cutoff=CUTOFF, variant=None):
    """(edge_index int64 [2, E] molecule-local, atom_start int64 [M + 1]) of a list of position arrays."""
    start = np.concatenate([[0], np.cumsum([len(np.asarray(R).reshape(-1, 3)) for R in mols])]).astype(np.int64)
    parts = [edges_of(adjacency(R, cutoff, variant), variant) + (int(s) if variant == "global_ids" else 0)
             for R, s in zip(mols, start[:-1])]
    ei = np.concatenate(parts, axis=1) if parts else np.zeros((2, 0), np.int64)
    return ei, start


def flat(mols):
    """(pos float32 [N, 3], atom_start int64 [M + 1]) of a list of position arrays."""
    start = np.concatenate([[0], np.cumsum([len(np.asarray(R).reshape(-1, 3)) for R in mols])]).astype(np.int64)
    parts = [np.asarray(R, np.float32).reshape(-1, 3) for R in mols]
    return (np.concatenate(parts) if parts else np.zeros((0, 3), np.float32)), start


def adjacency_from_edges(ei, n):
    adj = np.zeros((n, n), bool)
    adj[ei[0], ei[1]] = True
    return adj


def compare(mols, adj_of, cutoff=CUTOFF):
    """Against the statement: ``adj_of(k)`` is the bool adjacency under test of molecule k.  Returns (pairs decided
    wrongly, undecided ordered pairs, all ordered pairs i != j, molecules whose adjacency is not symmetric)."""
    wrong = undecided = pairs = asym = 0
    for k, R in enumerate(mols):
        got, want, dec = adj_of(k), adjacency(R, cutoff), decided(R, cutoff)
        n = len(R)
        wrong += int(((got != want) & dec).sum()) + int(got[np.eye(n, dtype=bool)].sum())
        undecided += n * (n - 1) - int(dec.sum())
        pairs += n * (n - 1)
        asym += int(not np.array_equal(got, got.T))
    return wrong, undecided, pairs, asym


# ------------------------------------------------------------------------------------------------- fixtures
def aid_molecules(indices=None, shift=0.0):
    """The AID geometries (tests/golden/aid_geom.npz) as float32 [n, 3] arrays, optionally moved by ``shift`` A along
    every axis (rounded to float32 again: what a kernel is given)."""
    with np.load(os.path.join(GOLDEN, "aid_geom.npz"), allow_pickle=False) as z:
        counts, pos = z["counts"].astype(np.int64), z["pos"].astype(np.float32)
    off = np.concatenate([[0], np.cumsum(counts)])
    idx = range(len(counts)) if indices is None else indices
    return [(pos[off[m]:off[m + 1]] + np.float32(shift)).astype(np.float32) for m in idx]


def s160_molecules(n=128, seed=0):
    """The positions of ``synth.synthetic_molecules(n, "S160", seed)`` (the same generator stream), float32."""
    from x2gnn.synth import SHAPES, random_geometry

    rng = np.random.default_rng(seed)
    return [random_geometry(rng, SHAPES["S160"])[1].astype(np.float32) for _ in range(n)]


def uniform_molecules():
    """Six molecules of 300 atoms, uniform in a cube of 18 A: rows of more than four 64-lane steps."""
    return list(np.random.default_rng(5).uniform(-9, 9, size=(6, 300, 3)).astype(np.float32))


# name -> (molecules, the largest share of ordered pairs that may be undecided)
FIXTURES = {
    "aid": (lambda: aid_molecules(), 1e-5),
    "aid16": (lambda: aid_molecules(range(16)), 0.0),
    "aid21": (lambda: aid_molecules([21]), 0.0),
    "s160": (lambda: s160_molecules(), 0.0),
    "uniform300": (lambda: uniform_molecules(), 0.0),
    "aid_plus_100": (lambda: aid_molecules(shift=100.0), 1e-2),
}


# the exact fixture: integer coordinates, so that both float32 forms and float64 are exact, d^2 = 25 sits on the
# cutoff (no edge: the test is strict) and d^2 = 24 inside it
LATTICE = [
    # 0-1 and 0-2 at d^2 = 25, 0-3 at 24, atom 4 coincident with atom 0
    [(0, 0, 0), (3, 4, 0), (0, 0, 5), (2, 2, 4), (0, 0, 0), (1, 0, 0)],
    [(7, 7, 7)],                           # one atom
    [],                                    # an empty molecule in the middle
    [(0, 0, 0), (6, 0, 0)],                # two atoms out of each other's reach
    [(0, 0, 0), (1, 0, 0), (9, 9, 9)],     # the last atom out of reach: last_bonded 1 of 3 atoms
]


def lattice_molecules():
    return [np.asarray(m, np.float32).reshape(-1, 3) for m in LATTICE]


def lattice_expected(cutoff_sq=25):
    """From integer arithmetic alone: (edge_index [2, E] local, degree [N], edges, triplets, max_degree, last_bonded
    per molecule)."""
    cols, degree, edges, trips, top, last = [], [], [], [], [], []
    for mol in LATTICE:
        deg = [0] * len(mol)
        for i, a in enumerate(mol):
            for j, b in enumerate(mol):
                d2 = sum((p - q) ** 2 for p, q in zip(a, b))
                if i != j and 0 < d2 < cutoff_sq:
                    cols.append((i, j))
                    deg[i] += 1
        degree += deg
        edges.append(sum(deg))
        trips.append(sum(d * (d - 1) for d in deg))
        top.append(max(deg, default=0))
        last.append(max((i for i, d in enumerate(deg) if d), default=-1))
    ei = np.array(cols, np.int64).T.reshape(2, -1)
    return (ei, np.array(degree, np.int32), np.array(edges, np.int64), np.array(trips, np.int64),
            np.array(top, np.int64), np.array(last, np.int32))
