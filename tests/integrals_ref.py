"""The overlap matrix and the core Hamiltonian (include/x2g_integrals.h, csrc/integrals.hip) stated in float64 with plain
numpy / scipy, written from the formulas and not from the kernel: the oracle of tests/test_integrals_ref.py (which
grounds it on a textbook table and on quadrature) and of tests/test_gpu_integrals.py.

  S[a, b] = <a|b>,   H[a, b] = <a| -1/2 nabla^2 |b> - sum_C Z_C <a| 1/|r - R_C| |b>

over contracted real-spherical Gaussians.  A shell (l, exponents, coefficients) is  sum_k c_k N(e_k, l) r^l Y_lm
exp(-e_k r^2), N the primitive's radial normalisation, the whole rescaled to unit self-overlap; an atom's shells are
sorted stably by l; p functions are (x, y, z), d and f run m = -l .. l.

Primitive Cartesian integrals are McMurchie-Davidson (Helgaker, Jorgensen, Olsen, ch. 9): Hermite coefficients
E^{ij}_t by their two-term recursions, the kinetic integral from overlaps at j - 2, j, j + 2, the nuclear attraction
from R^n_tuv built by its recursion from the Boys function.  The Boys function is
F_n(x) = Gamma(n + 1/2) P(n + 1/2, x) / (2 x^{n + 1/2}) with scipy's regularised incomplete gamma P, and its Taylor
series  sum_k (-x)^k / (k! (2n + 2k + 1))  below x = 0.1.

The test bases are data, in pyscf's internal format {symbol: [[l, [exp, c1, ...], ...], ...]}.
"""
import functools
import math

import numpy as np
from scipy import special

BOHR = 0.52917721092
Z_OF = {"H": 1, "Li": 3, "C": 6, "N": 7, "O": 8, "F": 9}

# ------------------------------------------------------------------------------------------------- the test bases
STO3G_H = {"H": [[0, [3.42525091, 0.15432897], [0.62391373, 0.53532814], [0.16885540, 0.44463454]]]}


def _heavy(scale):
    """5 s / 4 p / 3 d / 1 f = 39 functions; not in l order (the constructors sort)."""
    s = scale
    return [
        [0, [4200.0 * s, 0.002], [630.0 * s, 0.015], [145.0 * s, 0.075], [41.0 * s, 0.26], [12.5 * s, 0.6],
         [1.9 * s, 0.24]],
        [1, [21.0 * s, 0.03], [4.9 * s, 0.15], [1.5 * s, 0.45]],
        [0, [21.0 * s, 0.12], [4.9 * s, 0.9], [1.5 * s, -0.05]],
        [0, [0.48 * s, 1.0]], [1, [0.48 * s, 1.0]],
        [0, [0.15 * s, 1.0]], [1, [0.15 * s, 1.0]],
        [2, [2.5 * s, 1.0]], [2, [0.63 * s, 1.0]], [2, [0.16 * s, 1.0]],
        [3, [0.8 * s, 1.0]],
        [0, [0.045 * s, 1.0]], [1, [0.045 * s, 1.0]],
    ]


SYNTH = {
    "C": _heavy(1.0), "N": _heavy(1.3), "O": _heavy(1.7), "F": _heavy(2.1),
    # 3 s / 2 p = 9 functions
    "H": [[0, [33.9, 0.025], [5.1, 0.19], [1.16, 0.85]], [0, [0.33, 1.0]], [1, [1.5, 1.0]], [0, [0.10, 1.0]],
          [1, [0.375, 1.0]]],
    # a two-column general contraction (2 s), an SP block (s + p), a d shell and two s: 13 functions, the features'
    # "every other shape"
    "Li": [[0, [120.0, 0.02, -0.005], [18.0, 0.14, -0.03], [4.0, 0.5, -0.12], [1.1, 0.45, 0.3]],
           [0, [0.6, -0.2], [0.14, 1.1]], [1, [0.6, 0.1], [0.14, 0.95]],
           [2, [0.3, 1.0]], [0, [0.07, 1.0]], [0, [0.028, 1.0]]],
}

# the same basis as NWChem text (Fortran exponents, comments, an SP block, a general contraction)
SYNTH_LI_NWCHEM = """
# a made-up element entry
BASIS "ao basis" SPHERICAL PRINT
Li    S
    1.2D+02   0.02  -0.005     # two columns: two shells
    18.0      0.14  -0.03
    4.0       0.5   -0.12
    1.1       0.45   0.3
Li    SP
    0.6      -0.2    0.1
    0.14      1.1    0.95
Li    D
    3.0d-01   1.0
Li    S
    0.07      1.0
Li    S
    2.8E-02   1.0
END
"""


def to_nwchem(basis):
    """NWChem text of a pyscf-format basis, one block per entry."""
    kinds = "SPDF"
    out = ["BASIS \"ao basis\" SPHERICAL"]
    for sym, entries in basis.items():
        for entry in entries:
            out.append(f"{sym}    {kinds[entry[0]]}")
            out += ["    " + "  ".join(repr(float(v)) for v in row) for row in entry[1:]]
    return "\n".join(out + ["END", ""])


# ------------------------------------------------------------------------------------------------- shells
def atom_shells(basis, sym):
    """[(l, exponents, coefficients with the normalisation folded in)] of one element, sorted stably by l."""
    shells = []
    for entry in basis[sym]:
        l, tab = entry[0], np.asarray(entry[1:], np.float64)
        for k in range(1, tab.shape[1]):
            shells.append((l, tab[:, 0], tab[:, k]))
    out = []
    for l, e, c in sorted(shells, key=lambda s: s[0]):
        n = np.sqrt(2.0 * (2.0 * e) ** (l + 1.5) / math.gamma(l + 1.5))  # int (N r^l exp(-e r^2))^2 r^2 dr = 1
        d = c * n
        # <chi|chi> over the radial functions: int r^(2l+2) exp(-(e_i + e_j) r^2) dr
        pair = math.gamma(l + 1.5) / (2.0 * np.add.outer(e, e) ** (l + 1.5))
        out.append((l, e, d / np.sqrt(d @ pair @ d)))
    return out


def nao_of(basis, sym):
    return sum(2 * l + 1 for l, _, _ in atom_shells(basis, sym))


def aoslice(basis, symbols):
    """int64 [n, 4] like pyscf's aoslice_by_atom(): shell range, AO range."""
    rows, sh, ao = [], 0, 0
    for s in symbols:
        shells = atom_shells(basis, s)
        n = sum(2 * l + 1 for l, _, _ in shells)
        rows.append([sh, sh + len(shells), ao, ao + n])
        sh, ao = sh + len(shells), ao + n
    return np.asarray(rows, np.int64)


# ------------------------------------------------------------------------------------------------- real solid harmonics
def cart_components(l):
    """Exponent triples (a, b, c) with a + b + c = l, lexicographic."""
    return [(a, b, l - a - b) for a in range(l, -1, -1) for b in range(l - a, -1, -1)]


def solid_harmonics(l):
    """[{(a, b, c): coefficient}] for the 2l + 1 functions: r^l Y_lm normalised over the sphere; p as (x, y, z), d and
    f as m = -l .. l."""
    pi, q = math.pi, math.sqrt
    if l == 0:
        return [{(0, 0, 0): q(1 / (4 * pi))}]
    if l == 1:
        c = q(3 / (4 * pi))
        return [{(1, 0, 0): c}, {(0, 1, 0): c}, {(0, 0, 1): c}]
    if l == 2:
        a, b, c = q(15 / (4 * pi)), q(5 / (16 * pi)), q(15 / (16 * pi))
        return [{(1, 1, 0): a}, {(0, 1, 1): a}, {(0, 0, 2): 2 * b, (2, 0, 0): -b, (0, 2, 0): -b}, {(1, 0, 1): a},
                {(2, 0, 0): c, (0, 2, 0): -c}]
    if l == 3:
        a, b, c, d, e = (q(35 / (32 * pi)), q(105 / (4 * pi)), q(21 / (32 * pi)), q(7 / (16 * pi)),
                         q(105 / (16 * pi)))
        return [{(2, 1, 0): 3 * a, (0, 3, 0): -a},
                {(1, 1, 1): b},
                {(0, 1, 2): 4 * c, (2, 1, 0): -c, (0, 3, 0): -c},
                {(0, 0, 3): 2 * d, (2, 0, 1): -3 * d, (0, 2, 1): -3 * d},
                {(1, 0, 2): 4 * c, (3, 0, 0): -c, (1, 2, 0): -c},
                {(2, 0, 1): e, (0, 2, 1): -e},
                {(3, 0, 0): a, (1, 2, 0): -3 * a}]
    raise ValueError(f"l = {l}")


@functools.lru_cache(maxsize=None)
def c2s(l):
    """[2l + 1, ncart] matrix of solid_harmonics over cart_components."""
    comps = cart_components(l)
    out = np.zeros((2 * l + 1, len(comps)))
    for m, poly in enumerate(solid_harmonics(l)):
        for key, v in poly.items():
            out[m, comps.index(key)] = v
    return out


# ------------------------------------------------------------------------------------------------- Boys
def boys(n, x):
    """F_n(x) = int_0^1 t^(2n) exp(-x t^2) dt for x >= 0 (array)."""
    x = np.asarray(x, np.float64)
    out = np.empty_like(x)
    small = x < 0.1
    xs = x[small]
    acc, term = np.zeros_like(xs), np.ones_like(xs)
    for k in range(40):
        acc += term / (2 * n + 2 * k + 1)
        term = term * (-xs) / (k + 1)
    out[small] = acc
    xl = x[~small]
    out[~small] = special.gamma(n + 0.5) * special.gammainc(n + 0.5, xl) / (2.0 * xl ** (n + 0.5))
    return out


# ------------------------------------------------------------------------------------------------- primitive integrals
def hermite_e(la, lb, a, b, ab):
    """E[i, j, t] for i <= la, j <= lb: the expansion of x_A^i x_B^j exp(-a x_A^2 - b x_B^2) in Hermite Gaussians at
    P; ``ab`` = A - B (one dimension)."""
    p, mu = a + b, a * b / (a + b)
    pa, pb = -b / p * ab, a / p * ab
    E = np.zeros((la + 1, lb + 1, la + lb + 2))
    E[0, 0, 0] = math.exp(-mu * ab * ab)
    for j in range(lb):
        for t in range(j + 2):
            E[0, j + 1, t] = (E[0, j, t - 1] / (2 * p) if t else 0.0) + pb * E[0, j, t] + (t + 1) * E[0, j, t + 1]
    for i in range(la):
        for j in range(lb + 1):
            for t in range(i + j + 2):
                E[i + 1, j, t] = (E[i, j, t - 1] / (2 * p) if t else 0.0) + pa * E[i, j, t] + (t + 1) * E[i, j, t + 1]
    return E


def hermite_r(L, p, PC, x_boys=None):
    """R[t, u, v] (t + u + v <= L) summed over nothing: [L+1, L+1, L+1, n_nuclei], from
    R^n_000 = (-2p)^n F_n(p |PC|^2),  R^n_{t+1,u,v} = t R^{n+1}_{t-1,u,v} + X R^{n+1}_{t,u,v}  (and alike for u, v)."""
    PC = np.asarray(PC, np.float64).reshape(-1, 3)
    x = p * (PC ** 2).sum(axis=1)
    R = np.zeros((L + 1, L + 1, L + 1, L + 1, len(PC)))  # [n, t, u, v, C]
    for n in range(L + 1):
        R[n, 0, 0, 0] = (-2.0 * p) ** n * boys(n, x)
    X, Y, Z = PC[:, 0], PC[:, 1], PC[:, 2]
    for total in range(1, L + 1):
        for t in range(total + 1):
            for u in range(total - t + 1):
                v = total - t - u
                for n in range(L + 1 - total):
                    if t:
                        val = X * R[n + 1, t - 1, u, v] + ((t - 1) * R[n + 1, t - 2, u, v] if t > 1 else 0.0)
                    elif u:
                        val = Y * R[n + 1, t, u - 1, v] + ((u - 1) * R[n + 1, t, u - 2, v] if u > 1 else 0.0)
                    else:
                        val = Z * R[n + 1, t, u, v - 1] + ((v - 1) * R[n + 1, t, u, v - 2] if v > 1 else 0.0)
                    R[n, t, u, v] = val
    return R[0]


def primitive_block(la, a, A, lb, b, B, nuclei, charges):
    """(S, T, V) [ncart(la), ncart(lb)] between the unnormalised Cartesian primitives x_A^i y_A^j z_A^k exp(-a r_A^2)
    and the like at B; V = -sum_C Z_C <.|1/r_C|.>."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    p = a + b
    P = (a * A + b * B) / p
    E = [hermite_e(la, lb + 2, a, b, A[d] - B[d]) for d in range(3)]
    pref = (math.pi / p) ** 1.5

    def s1(d, i, j):
        return E[d][i, j, 0] if j >= 0 else 0.0

    def t1(d, i, j):
        return -0.5 * (j * (j - 1) * s1(d, i, j - 2) - 2.0 * b * (2 * j + 1) * s1(d, i, j) + 4.0 * b * b * s1(d, i, j + 2))

    L = la + lb
    G = (hermite_r(L, p, P[None, :] - np.asarray(nuclei, np.float64).reshape(-1, 3)) *
         np.asarray(charges, np.float64)).sum(axis=-1)
    ca, cb = cart_components(la), cart_components(lb)
    S, T, V = (np.zeros((len(ca), len(cb))) for _ in range(3))
    for ia, (ax, ay, az) in enumerate(ca):
        for ib, (bx, by, bz) in enumerate(cb):
            sx, sy, sz = s1(0, ax, bx), s1(1, ay, by), s1(2, az, bz)
            S[ia, ib] = pref * sx * sy * sz
            T[ia, ib] = pref * (t1(0, ax, bx) * sy * sz + sx * t1(1, ay, by) * sz + sx * sy * t1(2, az, bz))
            ex, ey, ez = E[0][ax, bx, :ax + bx + 1], E[1][ay, by, :ay + by + 1], E[2][az, bz, :az + bz + 1]
            V[ia, ib] = -2.0 * math.pi / p * np.einsum("t,u,v,tuv->", ex, ey, ez,
                                                        G[:ax + bx + 1, :ay + by + 1, :az + bz + 1])
    return S, T, V


# ------------------------------------------------------------------------------------------------- matrices
def one_electron(basis, symbols, pos_bohr, parts=False, nuclei=None):
    """(S, H) [nao, nao] of one molecule; ``parts``: (S, T, V).  ``nuclei``: the atoms that attract (default: all)."""
    pos = np.asarray(pos_bohr, np.float64).reshape(-1, 3)
    charges = [Z_OF[s] if nuclei is None or k in nuclei else 0 for k, s in enumerate(symbols)]
    shells = []  # (atom, l, exps, coefs, first function)
    ao = 0
    for k, s in enumerate(symbols):
        for l, e, d in atom_shells(basis, s):
            shells.append((k, l, e, d, ao))
            ao += 2 * l + 1
    S, T, V = (np.zeros((ao, ao)) for _ in range(3))
    for x, (ka, la, ea, da, oa) in enumerate(shells):
        for kb, lb, eb, db, ob in shells[x:]:
            acc = [0.0, 0.0, 0.0]
            for a, wa in zip(ea, da):
                for b, wb in zip(eb, db):
                    blk = primitive_block(la, a, pos[ka], lb, b, pos[kb], pos, charges)
                    acc = [t + wa * wb * m for t, m in zip(acc, blk)]
            for M, blk in zip((S, T, V), acc):
                sph = c2s(la) @ blk @ c2s(lb).T
                M[oa:oa + 2 * la + 1, ob:ob + 2 * lb + 1] = sph
                M[ob:ob + 2 * lb + 1, oa:oa + 2 * la + 1] = sph.T
    return (S, T, V) if parts else (S, T + V)


# ------------------------------------------------------------------------------------------------- the test molecules
def h2(distance_bohr=1.4):
    return ["H", "H"], np.array([[0.0, 0.0, 0.0], [0.0, 0.0, distance_bohr]]) * BOHR


def mol5(seed=5):
    """A seeded, asymmetric C, N, O, F, H molecule (angstrom): a random walk with steps of 1.0 to 1.6 angstrom."""
    rng = np.random.default_rng(seed)
    pos = [np.zeros(3)]
    for _ in range(4):
        v = rng.standard_normal(3)
        pos.append(pos[-1] + v / np.linalg.norm(v) * rng.uniform(1.0, 1.6))
    return ["C", "N", "O", "F", "H"], np.asarray(pos)


def mol3():
    """Three atoms with the 13-function element."""
    return ["Li", "O", "H"], np.array([[0.1, -0.2, 0.05], [1.45, 0.3, -0.4], [1.9, 1.05, 0.2]])


def aligned_edges(symbols, edge_index):
    """bool [E]: the edges whose block the features place on their shell groups, heavy-heavy, heavy-H and H-H, so
    that the row does not change under a rotation; H-heavy (9, 39) and every other shape are not."""
    n = np.array([nao_of(SYNTH, s) for s in symbols])
    r, c = n[np.asarray(edge_index)[0]], n[np.asarray(edge_index)[1]]
    return ((r == 39) & ((c == 39) | (c == 9))) | ((r == 9) & (c == 9))


def random_rotation(seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


@functools.lru_cache(maxsize=None)
def reference(name):
    """(symbols, pos in angstrom, S, H) of a named case, computed once: 'h2' (STO-3G), 'mol5' and 'mol3' (SYNTH)."""
    if name == "h2":
        sym, pos = h2()
        return (sym, pos) + one_electron(STO3G_H, sym, pos / BOHR)
    sym, pos = {"mol5": mol5, "mol3": mol3}[name]()
    return (sym, pos) + one_electron(SYNTH, sym, pos / BOHR)
