"""Fixed-shape padding, the host half: the filler molecules that bring every batch of an epoch to one shape
(N_cap, E_cap, T_cap, B_real + F), so that a step captured on one batch could replay on all of them (numpy only;
the device half, which assembles such a batch and steps on it, is not in the tree: DESIGN.md section 5).

A HIP graph bakes in every host number of the batch it was recorded on: the row counts, the degree and
molecule-size bounds, every address.  The scheme keeps the batch at one shape instead: ``F`` filler molecules
with exactly ``dn = N_cap - N`` atoms, ``de = E_cap - E`` directed edges and ``dt = T_cap - T`` triplets follow
the real ones, and the loss leaves them out.  The batch stays an ordinary molecular batch (symmetric, every
edge inside its molecule), so no kernel of the step changes.

The arithmetic.  A symmetric graph with out-degrees d_i has E = sum d_i directed edges and
T = sum d_i (d_i - 1) triplets, so a filler is a degree sequence in [0, C] over ``dn`` atoms with
sum d = de and sum d (d - 1) = dt (both even), realised as a simple graph.  ``C`` is the pool's own largest
degree: a filler never raises the batch's degree bound.  Atoms the sequence does not need stay without edges
(x2g_center_schedule packs them into units of their own, x2g_vertex_to_edge_sym_mol gives them empty rows, the
center kernels skip them).  With F > 1 the molecules after the first are two bonded atoms each (2 edges, no
triplet) and share the edgeless atoms, so every filler molecule has an edge and ``plan.out_graphs`` counts them
all.

The graph (``filler_plan``): the bulk as complete graphs K_k with k - 2 near dt / de (vectorised), as many as
leave a rest inside the region; the rest (``degree_sequences``) as the even spread of its edge ends over m atoms
(degrees q and q + 1: the fewest triplets m atoms can hold), m the fewest atoms that do not overshoot dt, then
single moves of one edge end from an atom of degree a to one of degree b >= a, each adding 2 (b - a + 1)
triplets; realised by Havel-Hakimi, a sequence that is no graph skipped for the next candidate.

The region (``in_region`` / ``region_bounds``): with n = dn - 2 (F - 1) and S = de - 2 (F - 1) (the first filler
molecule's share), S and dt even,
    spread(S, min(n, S)) <= dt <= spread(S, m_min)
where spread(S, m) is the triplet count of S edge ends spread evenly over m atoms and m_min the fewest atoms
with q1 = ceil(S / m), q1 + REGION_HEADROOM <= C and q1 + q1 // 2 + REGION_ROOM <= m.  ``DeviceDataset.capacity``
sizes an epoch's slack so that every one of its batches lies inside; ``filler_plan`` still answers outside of it
when it finds a graph, and returns None when it does not: it never returns a graph with other counts (it
recounts before returning).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

CUTOFF = 5.0  # the model's radius cutoff (xgnn.py:30-33): every filler edge is shorter


@dataclass(frozen=True)
class Capacity:
    """The one shape of an epoch's padded batches: ``real_graphs`` real molecules and ``fillers`` filler
    molecules of together ``nodes`` atoms, ``edges`` directed edges and ``triplets`` triplets;
    ``max_degree`` / ``max_mol_atoms`` bound every batch of the epoch, fillers included."""
    real_graphs: int
    fillers: int
    nodes: int
    edges: int
    triplets: int
    max_degree: int
    max_mol_atoms: int

    @property
    def graphs(self):
        return self.real_graphs + self.fillers


@dataclass(frozen=True)
class Filler:
    """An explicit filler graph: ``x`` int64 [dn] (atomic number 0: the embedding's padding row, which no rule
    of the embedding counts), ``atom_pos`` f32 [dn, 3], ``edge_index`` int64 [2, de] with batch-local atom ids
    0 .. dn - 1 sorted by (src, dst), and per filler molecule ``nodes`` / ``edges`` / ``triplets`` int64 [F]
    (the molecules' atoms and edges are consecutive)."""
    x: np.ndarray
    atom_pos: np.ndarray
    edge_index: np.ndarray
    nodes: np.ndarray
    edges: np.ndarray
    triplets: np.ndarray


# ----------------------------------------------------------------------------------------- positions
def _position_table(count=4096, spacing=0.28, radius=2.45):
    """Distinct lattice points inside a ball of diameter < CUTOFF (every pair 0 < d < 4.9), nearest the
    centre first."""
    k = int(radius / spacing) + 1
    g = np.arange(-k, k + 1, dtype=np.float64) * spacing
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    r = np.sqrt((p * p).sum(1))
    p, r = p[r <= radius], r[r <= radius]
    return np.ascontiguousarray(p[np.argsort(r, kind="stable")][:count].astype(np.float32))


POSITIONS = _position_table()  # [P, 3]: a filler molecule's atom i sits at POSITIONS[i]


# ----------------------------------------------------------------------------------------- degree sequence
def _spread_triplets(S, m):
    """Triplets of S edge ends spread evenly over m atoms (vectorised over m >= 1)."""
    q, r = S // m, S % m
    return r * (q + 1) * q + (m - r) * q * (q - 1)


def degree_sequences(n, S, T, C):
    """Candidate degree sequences (int64, descending, zeros left out) of at most ``n`` atoms in [1, C] with sum
    ``S`` and sum d (d - 1) = ``T``, the likeliest to be a graph first; nothing where there is none."""
    n, S, T, C = int(n), int(S), int(T), int(C)
    if S < 0 or T < 0 or n < 0 or S % 2 or T % 2:
        return
    if S == 0:
        if T == 0:
            yield np.zeros(0, np.int64)
        return
    if C < 1 or n < 1 or T > (C - 1) * S or S > C * n:
        return
    m = np.arange(-(-S // C), min(n, S) + 1, dtype=np.int64)
    fits = np.nonzero(_spread_triplets(S, m) <= T)[0]
    # the spread's triplets fall as m grows: the fewest atoms that do not overshoot leave the smallest rest; a few
    # more atoms where that rest is out of the moves' reach or the sequence is no graph; the narrowest moves first
    for mi in fits[:6]:
        mm = int(m[mi])
        seen = []
        for width in (1, 2, 4, C):
            seq = _spread_and_move(S, T, mm, C, width)
            if seq is not None and not any(np.array_equal(seq, o) for o in seen):
                seen.append(seq)
                yield seq


def _spread_and_move(S, T, m, C, width):
    """The even spread of S over m atoms, then moves among the degrees within ``width`` of the spread's."""
    q, r = S // m, S % m
    cnt = np.zeros(C + 2, np.int64)  # atoms per degree
    cnt[q] += m - r
    cnt[q + 1] += r
    g = T - int(_spread_triplets(S, m))
    lo, hi = max(q - width, 1), min(q + 1 + width, C)
    while g > 0:
        want = g // 2  # b - a + 1: exactly where two levels have it, else the largest below
        lv = np.nonzero(cnt[lo + 1:hi])[0] + lo + 1  # a - 1 >= lo, b + 1 <= hi
        best = None
        for a in lv:
            cand = lv[(lv >= a) & (lv <= a + want - 1)]
            if cnt[a] < 2:
                cand = cand[cand != a]
            if cand.size == 0:
                continue
            b = int(cand[-1])
            if best is None or b - a + 1 > best[0]:
                best = (b - a + 1, int(a), b)
                if b - a + 1 == want:
                    break
        if best is None:
            return None
        gain, a, b = best
        k = max(min(want // gain, cnt[a] // 2 if a == b else min(cnt[a], cnt[b])), 1)
        cnt[a] -= k
        cnt[a - 1] += k
        cnt[b] -= k
        cnt[b + 1] += k
        g -= 2 * gain * k
    if g != 0 or cnt[C + 1] or (cnt < 0).any():
        return None
    deg = np.repeat(np.arange(C + 2, dtype=np.int64), cnt)[::-1]
    return np.ascontiguousarray(deg[deg > 0])


def havel_hakimi(deg):
    """A simple undirected graph with the degrees ``deg`` (descending or not): int64 [2, sum deg] directed
    edges (both directions) sorted by (src, dst), or None when the sequence is not graphical."""
    deg = np.asarray(deg, dtype=np.int64)
    m = int(deg.shape[0])
    rem = deg.copy()
    src, dst = [], []
    ids = np.arange(m)
    for _ in range(m):
        v = int(np.argmax(rem))
        d = int(rem[v])
        if d == 0:
            break
        rem[v] = -1  # out of the running
        if d > m - 1:
            return None
        nb = np.argpartition(-rem, d - 1)[:d] if d < m else ids
        # ties at the boundary must not matter for correctness: any d largest do (Havel-Hakimi)
        if (rem[nb] <= 0).any():
            return None
        rem[nb] -= 1
        rem[v] = 0
        src.append(np.full(d, v, np.int64))
        dst.append(nb.astype(np.int64))
    if (rem != 0).any():
        return None
    if not src:
        return np.zeros((2, 0), np.int64)
    a, b = np.concatenate(src), np.concatenate(dst)
    s, t = np.concatenate([a, b]), np.concatenate([b, a])
    order = np.argsort(s * m + t, kind="stable")
    return np.stack([s[order], t[order]])


# ----------------------------------------------------------------------------------------- the region
REGION_HEADROOM = 1  # the densest spread of the region leaves its degrees q + 1 + REGION_HEADROOM <= C
REGION_ROOM = 3      # ... and has at least 1.5 (q + 1) + REGION_ROOM atoms (the moves' sequences are then graphs)


def region_bounds(n, S, C):
    """(T_lo, T_hi) of the region for ``n`` atoms and ``S`` directed edges, or None where it is empty: from the
    even spread over min(n, S) atoms (the fewest triplets there are) up to the even spread over the fewest
    atoms m with q1 = ceil(S / m), q1 + REGION_HEADROOM <= C and q1 + q1 // 2 + REGION_ROOM <= m."""
    n, S, C = int(n), int(S), int(C)
    if S < 2 or S % 2 or n < 2:
        return None
    m = np.arange(1, min(n, S) + 1, dtype=np.int64)
    q1 = -(-S // m)
    ok = np.nonzero((q1 + REGION_HEADROOM <= C) & (q1 + q1 // 2 + REGION_ROOM <= m))[0]
    if ok.size == 0:
        return None
    return int(_spread_triplets(S, min(n, S))), int(_spread_triplets(S, int(m[ok[0]])))


def _in_main_region(n, S, T, C):
    b = region_bounds(n, S, C)
    return b is not None and b[0] <= T <= b[1] and T % 2 == 0


def in_region(dn, de, dt, C, F=1):
    """Whether ``filler_plan(dn, de, dt, C, F)`` is promised to return a graph: with n = dn - 2 (F - 1) and
    S = de - 2 (F - 1) (the first filler molecule's share), S and dt even and ``region_bounds(n, S, C)[0] <= dt <=
    region_bounds(n, S, C)[1]`` (tests/test_padding.py checks the promise, exhaustively for small sizes)."""
    dn, de, dt, C, F = int(dn), int(de), int(dt), int(C), int(F)
    if F < 1 or dt < 0 or dt % 2:
        return False
    n, S = dn - 2 * (F - 1), de - 2 * (F - 1)
    if n > POSITIONS.shape[0]:
        return False
    b = region_bounds(n, S, C)
    return b is not None and b[0] <= dt <= b[1]


# ----------------------------------------------------------------------------------------- the filler
def filler_plan(dn, de, dt, C, F=1):
    """The filler graph of exactly ``dn`` atoms, ``de`` directed edges and ``dt`` triplets in ``F`` molecules, no
    degree above ``C``, or None when none is found (always a graph inside ``in_region``)."""
    dn, de, dt, C, F = int(dn), int(de), int(dt), int(C), int(F)
    if F < 1 or dn < 2 * F or de < 2 * F or dt < 0 or C < 1:
        return None
    n, S = dn - 2 * (F - 1), de - 2 * (F - 1)
    # the bulk as c complete graphs K_k, k - 2 near the triplets per edge asked for (vectorised: Havel-Hakimi is a
    # Python loop over the atoms), as many as leave a rest that is still inside the region; the rest by sequence
    T = dt
    k = min(C + 1, max(3, T // max(S, 1) + 2))
    ke, kt = k * (k - 1), k * (k - 1) * (k - 2)
    c = 0
    if _in_main_region(n, S, T, C):
        top = min(n // k, S // ke, T // kt if kt else S // ke)
        step = 0
        while top - step > 0 and not _in_main_region(n - (top - step) * k, S - (top - step) * ke,
                                                     T - (top - step) * kt, C):
            step = max(1, 2 * step)
        c = max(top - step, 0)
    n, S, T = n - c * k, S - c * ke, T - c * kt
    deg = ei0 = None
    for deg in degree_sequences(n, S, T, C):
        ei0 = havel_hakimi(deg) if deg.shape[0] >= 2 else None
        if ei0 is not None:
            break
    if ei0 is None:
        return None
    if c:
        a, b = np.nonzero(~np.eye(k, dtype=bool))  # K_k's edges in (src, dst) order
        base = (np.arange(c, dtype=np.int64) * k)[:, None]
        ei0 = np.concatenate([np.stack([(base + a).reshape(-1), (base + b).reshape(-1)]), ei0 + c * k], axis=1)
        deg = np.concatenate([np.full(c * k, k - 1, np.int64), deg])
    used = int(deg.shape[0])
    # the edgeless atoms levelled over the molecules (the first has `used` bonded atoms, the others two)
    nodes = np.full(F, 2, np.int64)
    nodes[0] = used
    spare = dn - used - 2 * (F - 1)
    while spare > 0:  # (F is a handful)
        i = int(np.argmin(nodes))
        second = np.partition(nodes, 1)[1] if F > 1 else nodes[i] + spare
        add = int(min(spare, max(second - nodes[i], 1)))
        nodes[i] += add
        spare -= add
    if int(nodes.max()) > POSITIONS.shape[0]:
        return None
    start = np.concatenate([[0], np.cumsum(nodes)])
    parts = [ei0]
    for f in range(1, F):
        a = int(start[f])
        parts.append(np.array([[a, a + 1], [a + 1, a]], np.int64))
    ei = np.concatenate(parts, axis=1)
    edges = np.full(F, 2, np.int64)
    edges[0] = ei0.shape[1]
    trips = np.zeros(F, np.int64)
    trips[0] = int((deg * (deg - 1)).sum())
    pos = np.concatenate([POSITIONS[:k] for k in nodes])
    fl = Filler(np.zeros(dn, np.int64), pos, ei, nodes, edges, trips)
    # recount: never a graph with other counts
    if ei.shape[1] != de or int(trips.sum()) != dt or int(nodes.sum()) != dn:
        return None
    if ei.shape[1] and int(np.bincount(ei[0], minlength=dn).max()) > C:
        return None
    return fl


# ----------------------------------------------------------------------------------------- the capacity
# what a padded edge row and a padded atom cost in triplet rows when candidates are ranked (an edge row runs
# the featurisation and every layer's dense chain, a triplet row one attention term): rough, only an order
COST_EDGE = 8
COST_ATOM = 1


def _fewest_atoms_table(s_max, C):
    """m_min[S] for S = 0 .. s_max: the fewest atoms of the region's densest spread (``region_bounds``), 0 where
    there is none."""
    S = np.arange(s_max + 1, dtype=np.int64)[:, None]
    m = np.arange(1, int(1.5 * C + REGION_ROOM + 3) + int(np.sqrt(2 * s_max)) + 2, dtype=np.int64)[None, :]
    q1 = -(-S // m)
    ok = (q1 + REGION_HEADROOM <= C) & (q1 + q1 // 2 + REGION_ROOM <= m) & (m <= S)
    first = np.argmax(ok, axis=1)
    return np.where(ok.any(axis=1), m[0][first], 0)


def solve_capacity(nodes, edges, triplets, C, F, real_graphs, pool_max_atoms, max_mol_atoms):
    """The cheapest fixed shape found that puts every batch of an epoch inside the region: ``nodes`` / ``edges`` /
    ``triplets`` are the batches' real totals (one entry per index list), ``C`` the pool's largest degree.

    The gaps of one epoch vary independently (a batch can sit at the largest N and the smallest T), so the shape
    needs base slack over the largest N and E: for each candidate (dn0, de0) every list's triplet window
    [T + T_lo, T + T_hi] (``region_bounds`` of its own gaps) is taken, vectorised over the lists, and where the
    windows meet their lowest common point is T_cap; the candidate of the least weighted padding (COST_EDGE,
    COST_ATOM) wins.  Raises ValueError where no slack within the filler's reach does it."""
    N, E, T = (np.asarray(a, dtype=np.int64) for a in (nodes, edges, triplets))
    C, F = int(C), int(F)
    if F < 1:
        raise ValueError("fillers must be at least 1")
    if (E % 2).any() or (T % 2).any():
        raise ValueError("a symmetric batch has even edge and triplet counts")
    Nmax, Nmin, Emax, Emin = int(N.max()), int(N.min()), int(E.max()), int(E.min())
    room = min(int(POSITIONS.shape[0]), int(max_mol_atoms))
    de_top = 8 * (C + 4) ** 2 + 2 * F
    fewest = _fewest_atoms_table(de_top + Emax - Emin, C) if C >= 2 else None
    best = None
    de0 = 2 * F
    while fewest is not None and de0 <= de_top:
        S = Emax + de0 - E - 2 * (F - 1)
        m_hi = fewest[S]
        dn0 = 2 * F
        while m_hi.all() and dn0 + (Nmax - Nmin) - 2 * (F - 1) <= room:
            n = Nmax + dn0 - N - 2 * (F - 1)
            if (m_hi <= n).all():
                t_lo = int((T + _spread_triplets(S, np.minimum(n, S))).max())
                t_hi = int((T + _spread_triplets(S, m_hi)).min())
                if t_lo <= t_hi:
                    cost = t_lo + COST_EDGE * de0 + COST_ATOM * dn0
                    if best is None or cost < best[0]:
                        best = (cost, Nmax + dn0, Emax + de0, t_lo)
            dn0 += max(1, dn0 // 8)
        de0 += max(2, (de0 // 32) * 2)
    if best is not None:
        _, n_cap, e_cap, t_cap = best
        if all(in_region(n_cap - n, e_cap - e, t_cap - t, C, F) for n, e, t in zip(N, E, T)):
            filler_atoms = n_cap - Nmin - 2 * (F - 1)  # (a bound: the edgeless atoms are levelled over the fillers)
            return Capacity(int(real_graphs), F, n_cap, e_cap, t_cap, C, max(int(pool_max_atoms), filler_atoms))
    raise ValueError(f"no fixed shape within the fillers' reach for these {len(N)} batches (largest degree {C}, "
                     f"{F} filler molecule(s)): atoms {Nmin}-{Nmax}, edges {Emin}-{Emax}, triplets "
                     f"{int(T.min())}-{int(T.max())}")
