"""SBFTransformerV2's atom-context chain (csrc/atom_context.hip, include/x2g_atomctx.h) stated in float64 on the CPU,
each value with its *unit*, and a numpy-float32 emulation that fixes the bound's constants.

Values (numpy float64; nothing from x2gnn; the statement is the reference's model.py:138-141 with the conv's lin_edge,
sbftransformer_conv.py:144, evaluated per atom instead of per triplet):

    A[a]   = sum_{e in [rowptr[a], rowptr[a+1])} x[e]                 (no out-edges: 0)
    z0     = A W0^T + b0,   h = SiLU(z0),   g = h W1^T + b1,   tab = g We^T
    d_g    = d_tab We,   d_h = d_g W1,   d_z0 = d_h SiLU'(z0),   d_A = d_z0 W0,   dx[e] = d_A[a(e)] (+ old dx[e])

Every input is the float32 array the kernel gets, widened to float64; the backward's z0 is an input of its own (the
statement's z0 rounded to float32, or the forward kernel's).

Units.  Every function returns (value, unit) pairs: the unit is the float64 sum of the magnitudes of the terms that
make the value up.  With s = sigmoid(z0), SiLU'(z) = s (1 + z (1 - s)):

    unit(A)    = sum_e |x[e]|                                         (degree 0: 0, the kernel has to write exact zeros)
    unit(z0)   = unit(A) |W0|^T + |b0|
    unit(h)    = |SiLU'(z0)| unit(z0) + |h| + 2^-102
                 (what z0's error does to h, plus h's own rounding; 2^-102 = 2^-126 / 2^-24: where exp(-z0) overflows
                 float32 the exact h is below the smallest normal number and the kernel's -0 is off by less than that)
    unit(g)    = unit(h) |W1|^T + |b1|
    unit(tab)  = unit(g) |We|^T
    unit(d_g)  = |d_tab| |We|,   unit(d_h) = unit(d_g) |W1|
    unit(SiLU'(z0)) = s (1 + |z0| (1 - s)) + 2^-102                   (z0 is an exact input here: its own rounding only)
    unit(d_z0) = unit(d_h) |SiLU'(z0)| + |d_h| unit(SiLU'(z0))
    unit(d_A)  = unit(d_z0) |W0|,   unit(dx[e]) = unit(d_A[a(e)]) (+ |old dx[e]| when added onto old contents)

A kernel passes when its value is finite and |kernel - ref64| <= K * 2^-24 * unit; there is no absolute floor, and
where the unit is exactly 0 the kernel has to return exactly 0 (the A row of an atom without out-edges).

K per family is fixed against the emulation below (``emu_*``: numpy float32, float32 ``exp``, the pool sequential in
row order and every product one fma chain in ascending k), measured against the float64 statement and never against
a kernel: the emulation's worst error / (2^-24 unit) over the shapes of tests/test_gpu_atom_context.py (``cases`` at
the end of this module), times 4, rounded up to a power of two.  4x because the kernels sum in another order (the
MFMA's k-steps interleave four partial chains per 16 terms), which can cost a small multiple of a sequential sum's
error but not more.  ``emulation_report`` measures the ratios; tests/test_atom_context_ref.py asserts that each stays
at or below EMULATION_RATIO and that 4 * EMULATION_RATIO <= K:

    family   worst emulation ratio (output, case)                                          x 4     K
    tab      0.24  (tab, N = 16)                                                            0.93    1
    saved    2.58  (A, N = 17 without biases: the 40-row sequential pool; z0 2.53, h 1.90,  10.3    16
                   g 1.36)
    dgz      3.87  (d_g, N = 31: the 128-term chain of the first product; d_z0 0.70)        15.5    16
    dx       0.076 (dx added onto old contents, N = 17; 0.070 written plainly)              0.31    0.5

(The units grow with every product they pass through, each a sum of magnitudes over 128 terms, while a float32 chain's
error grows like the square root of that: hence the small ratios of tab and dx, three products deep.  tab's K of 1
still means 2^-24 of the summed magnitudes.)
"""
import functools

import numpy as np

E32 = 2.0 ** -24
TINY = 2.0 ** -126 / E32  # float32's smallest normal number, in units
F = np.float32
D = 128
TILE = 16  # atoms per workgroup (kARows)
# worst |emulation - ref64| / (2^-24 unit) per family over the GPU test's shapes, rounded up (emulation_report)
EMULATION_RATIO = dict(tab=0.25, saved=2.6, dgz=3.9, dx=0.08)
K = dict(tab=1.0, saved=16.0, dgz=16.0, dx=0.5)
FAMILY = dict(tab="tab", A="saved", z0="saved", h="saved", g="saved", d_g="dgz", d_z0="dgz", dx="dx")


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def _sig(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z))


def edge_atom(rowptr, E):
    """The atom of every line node (rows of x in no atom's range: -1)."""
    rowptr = np.asarray(rowptr, np.int64)
    atom = np.full(E, -1, np.int64)
    for a in range(len(rowptr) - 1):
        atom[rowptr[a]:rowptr[a + 1]] = a
    return atom


# ------------------------------------------------------------------------------------------------ values, units
def context_fwd(x, rowptr, w0, b0, w1, b1, we):
    """dict(A, z0, h, g, tab) of (value, unit); b0 / b1 may be None."""
    N = len(rowptr) - 1
    x = np.zeros((0, D)) if x is None else _f64(x)
    w0, w1, we = _f64(w0), _f64(w1), _f64(we)
    b0 = np.zeros(D) if b0 is None else _f64(b0)
    b1 = np.zeros(D) if b1 is None else _f64(b1)
    A, uA = np.zeros((N, D)), np.zeros((N, D))
    for a in range(N):
        rows = x[rowptr[a]:rowptr[a + 1]]
        A[a], uA[a] = rows.sum(0), np.abs(rows).sum(0)
    z0, uz0 = A @ w0.T + b0, uA @ np.abs(w0).T + np.abs(b0)
    s = _sig(z0)
    h = z0 * s
    uh = np.abs(s * (1 + z0 * (1 - s))) * uz0 + np.abs(h) + TINY
    g, ug = h @ w1.T + b1, uh @ np.abs(w1).T + np.abs(b1)
    tab, utab = g @ we.T, ug @ np.abs(we).T
    return dict(A=(A, uA), z0=(z0, uz0), h=(h, uh), g=(g, ug), tab=(tab, utab))


def context_bwd(d_tab, z0, rowptr, E, w0, w1, we, dx_old=None):
    """dict(d_g, d_z0, d_A, dx) of (value, unit); z0: the float32 array the kernel is given."""
    d_tab, z0, w0, w1, we = _f64(d_tab), _f64(z0), _f64(w0), _f64(w1), _f64(we)
    dg, udg = d_tab @ we, np.abs(d_tab) @ np.abs(we)
    dh, udh = dg @ w1, udg @ np.abs(w1)
    s = _sig(z0)
    sg, usg = s * (1 + z0 * (1 - s)), s * (1 + np.abs(z0) * (1 - s)) + TINY
    dz, udz = dh * sg, udh * np.abs(sg) + np.abs(dh) * usg
    dA, udA = dz @ w0, udz @ np.abs(w0)
    atom = edge_atom(rowptr, E)
    dx, udx = dA[atom], udA[atom]
    if dx_old is not None:
        dx, udx = dx + _f64(dx_old), udx + np.abs(_f64(dx_old))
    return dict(d_g=(dg, udg), d_z0=(dz, udz), d_A=(dA, udA), dx=(dx, udx))


# ------------------------------------------------------------------------------------------------ float32 emulation
def _fma(a, b, c):
    """fma in float32: the product exact (float64 holds it), one rounding of the sum (to float64, then float32)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def _chain(a, m):
    """a [R, K] @ m [K, C] as one float32 fma chain per output, k ascending."""
    acc = np.zeros((a.shape[0], m.shape[1]), F)
    for k in range(a.shape[1]):
        acc = _fma(a[:, k:k + 1], m[k:k + 1, :], acc)
    return acc


def _emu_sig(z):
    with np.errstate(over="ignore"):
        return (F(1) / (F(1) + np.exp(-z, dtype=F))).astype(F)


def emu_fwd(x, rowptr, w0, b0, w1, b1, we):
    N = len(rowptr) - 1
    x = np.zeros((0, D), F) if x is None else np.asarray(x, F)
    w0, w1, we = (np.asarray(w, F) for w in (w0, w1, we))
    b0 = np.zeros(D, F) if b0 is None else np.asarray(b0, F)
    b1 = np.zeros(D, F) if b1 is None else np.asarray(b1, F)
    A = np.zeros((N, D), F)
    for a in range(N):
        for e in range(rowptr[a], rowptr[a + 1]):
            A[a] = A[a] + x[e]
    z0 = _chain(A, w0.T) + b0
    with np.errstate(over="ignore"):
        h = (z0 / (F(1) + np.exp(-z0, dtype=F))).astype(F)
    g = _chain(h, w1.T) + b1
    return dict(A=A, z0=z0, h=h, g=g, tab=_chain(g, we.T))


def emu_bwd(d_tab, z0, rowptr, E, w0, w1, we, dx_old=None):
    d_tab, z0, w0, w1, we = (np.asarray(v, F) for v in (d_tab, z0, w0, w1, we))
    dg = _chain(d_tab, we)
    dh = _chain(dg, w1)
    s = _emu_sig(z0)
    dz = dh * (s * (F(1) + z0 * (F(1) - s)))
    dA = _chain(dz, w0)
    dx = dA[edge_atom(rowptr, E)]
    if dx_old is not None:
        dx = dx + np.asarray(dx_old, F)
    return dict(d_g=dg, d_z0=dz, dx=dx)


# ------------------------------------------------------------------------------------------------ shapes, inputs
ATOMS = (1, 15, 16, 17, 2 * TILE - 1, 2 * TILE + 1)  # the grid is one workgroup per tile, never capped: no wrap case
HUB_DEGREE = 40


def degrees(N, seed=0):
    """Out-degrees drawn from 0..9, the first, the last and an interior atom without out-edges, one atom of degree
    40 (N = 1: the one atom has three out-edges; N = 2: degrees 0 and 40)."""
    rng = np.random.default_rng(7919 * N + seed)
    deg = rng.integers(0, 10, size=N)
    if N == 1:
        deg[:] = 3
        return deg
    deg[0] = deg[-1] = 0
    if N >= 4:
        deg[N // 2] = 0
    deg[min(1, N - 1) if N < 4 else N // 2 + 1] = HUB_DEGREE
    return deg


def context_inputs(N, empty=False, bias=True, seed=0):
    """Seeded float32 inputs: rowptr [N + 1] int32, x [E, 128], the three weights, two biases (None without), d_tab
    [N, 128] and old contents for dx.  ``empty``: E = 0 (every atom without out-edges)."""
    deg = np.zeros(N, np.int64) if empty else degrees(N, seed)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    E = int(rowptr[-1])
    rng = np.random.default_rng(104729 * N + 31 * bool(empty) + 7 * bool(bias) + seed)
    nrm = lambda *s: rng.standard_normal(s).astype(F)  # noqa: E731
    sc = F(1.0 / np.sqrt(D))
    return dict(rowptr=rowptr, E=E, x=nrm(E, D), w0=nrm(D, D) * sc, w1=nrm(D, D) * sc, we=nrm(D, D) * sc,
                b0=nrm(D) * F(0.1) if bias else None, b1=nrm(D) * F(0.1) if bias else None, d_tab=nrm(N, D),
                dx_old=nrm(E, D))


def cases():
    """(N, empty, bias) of tests/test_gpu_atom_context.py: every atom count with biases; no line node at all at
    N = 17; no biases at N = 17."""
    return [(N, False, True) for N in ATOMS] + [(17, True, True), (17, False, False)]


# ------------------------------------------------------------------------------------------------ the report
def ratio(got, ref, unit):
    """Worst |got - ref| / (2^-24 unit); an element with unit 0 has to be exactly 0 (inf otherwise)."""
    got, ref, unit = np.asarray(got, np.float64), np.asarray(ref), np.asarray(unit)
    err = np.abs(got - ref)
    if not np.isfinite(got).all():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(unit > 0, err / (E32 * unit), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


@functools.lru_cache(maxsize=None)
def emulation_report():
    """{family: (worst emulation error / (2^-24 unit), output, case)} over the GPU test's shapes."""
    worst = {}
    for N, empty, bias in cases():
        i = context_inputs(N, empty, bias)
        case = f"N={N} E={i['E']} bias={bias}"
        wf = (i["w0"], i["b0"], i["w1"], i["b1"], i["we"])
        ref, emu = context_fwd(i["x"], i["rowptr"], *wf), emu_fwd(i["x"], i["rowptr"], *wf)
        pairs = [(ref, emu)]
        z0 = ref["z0"][0].astype(F)
        wb = (i["w0"], i["w1"], i["we"])
        for old in (None, i["dx_old"]):
            pairs.append((context_bwd(i["d_tab"], z0, i["rowptr"], i["E"], *wb, old),
                          emu_bwd(i["d_tab"], z0, i["rowptr"], i["E"], *wb, old)))
        for r, e in pairs:
            for k in e:
                v = ratio(e[k], *r[k])
                if v > worst.get(FAMILY[k], (-1.0,))[0]:
                    worst[FAMILY[k]] = (v, k, case)
    return worst
