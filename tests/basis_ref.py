"""The radial x angular basis (csrc/basis.hip) stated in float64, with an a-priori error bound per element, and
a numpy-float32 emulation of the kernels' formulas that fixes the bound's constant.

Values (numpy / scipy only; nothing from x2gnn.ops; the constants are the oracle's, found by scipy root
bracketing, not the generated tables): ``dist`` from positions, ``envelope`` 1/x - 28 x^5 + 48 x^6 - 21 x^7 at
x = d / cutoff, ``rbf`` = sin(freq x) env, ``bessel_env`` = N_ln j_l(z_ln x) env (l-major), ``cos_theta`` from three
positions or a given angle, ``sph_y`` = sqrt((2l+1)/4pi) P_l(cos theta), ``sbf`` = bessel_env[trip_src] * Y_l0 and
``freq_grad`` = sum_e g env cos(freq x) x, for any (num_spherical <= 7, num_radial <= 16).  Every input is the
float32 array the kernel gets, widened to float64.

Bounds.  Each ``*_unit`` function returns, per element, e32 = 2^-24 times the magnitudes a float32 evaluation
of the kernel's formula rounds against: the sum of the formula's term magnitudes (its own cancellation) plus the
effect of rounding the argument once, through the derivative.  The radial one, with u = z_ln x:

    e32 * ( |env| * (M_ln(x) + |u N_ln j_l'(u)|) + (1/x + 28 x^5 + 48 x^6 + 21 x^7) * |B_ln(x)| )
    M_ln(x) = sum_m |c[l][n][m] x^m trig_m(u)| / x^(l+1)          (c: x2gnn/basis_consts.py, magnitudes only)

A kernel has to stay within ``K`` = 8 unit bounds (the suite's 8 * e32 convention).  K is fixed against the
emulation below (``emu_*``: the kernels' operation order in numpy float32 with correctly rounded sin / cos /
division), never against a kernel: over the test grids the emulation reaches at most ``EMULATION_RATIO`` unit
bounds per output (tests/test_basis_ref.py asserts it), so K leaves the ~3x the device's sincosf, division and
fused multiply-adds may take.  A kernel that needs more is a finding.
"""
import functools
import math

import numpy as np
from scipy import special

from oracle import ref_cpu, triplets

E32 = 2.0 ** -24
K = 8.0  # every bound is K unit bounds
CUTOFF = 5.0
NSPH_MAX, NRAD_MAX = 7, 16
# worst error / unit bound of the float32 emulation over the grids of tests/test_gpu_basis_fp64.py, rounded up
# (``emulation_report`` measures them; tests/test_basis_ref.py asserts that they hold).  bessel_env: 2.6 with the
# distances given, 3.0 with the distances x2g_edge_basis computes from positions itself.
EMULATION_RATIO = dict(dist=1.8, env=2.0, rbf=2.8, bessel_env=3.0, cos_theta=1.6, sph_y=1.4, sbf=2.2, freq_grad=1.5)


def _f64(a):
    return np.asarray(a, np.float64)


# ------------------------------------------------------------------------------------------------ values
@functools.lru_cache(maxsize=None)
def consts():
    """(zeros [7, 16] (the float32 roots, widened), normalisers N_ln [7, 16]) from the oracle."""
    return ref_cpu._basis_consts(NSPH_MAX, NRAD_MAX)


def dist(pos, src, dst):
    p = _f64(pos)
    return np.sqrt(((p[np.asarray(src)] - p[np.asarray(dst)]) ** 2).sum(1))


def env_terms(x):
    """The four term magnitudes of the envelope at x = d / cutoff."""
    return 1.0 / x, 28.0 * x ** 5, 48.0 * x ** 6, 21.0 * x ** 7


def envelope(d, cutoff=CUTOFF, c6=48.0):
    x = _f64(d) / cutoff
    return 1.0 / x - 28.0 * x ** 5 + c6 * x ** 6 - 21.0 * x ** 7


def rbf(d, freq, cutoff=CUTOFF):
    x = _f64(d) / cutoff
    return np.sin(_f64(freq)[None, :] * x[:, None]) * envelope(d, cutoff)[:, None]


def bessel(d, nsph, nrad, cutoff=CUTOFF):
    """[E, nsph * nrad] N_ln j_l(z_ln d / cutoff), l-major."""
    zeros, norm = consts()
    x = _f64(d) / cutoff
    return np.stack([norm[l, n] * special.spherical_jn(l, zeros[l, n] * x) for l in range(nsph) for n in range(nrad)],
                    axis=1)


def bessel_env(d, nsph, nrad, cutoff=CUTOFF):
    return bessel(d, nsph, nrad, cutoff) * envelope(d, cutoff)[:, None]


def _legs(pos, ai, aj, ak):
    p = _f64(pos)
    return p[np.asarray(ai)] - p[np.asarray(aj)], p[np.asarray(ak)] - p[np.asarray(aj)]


def cos_theta(pos, ai, aj, ak):
    """cos of the angle at atom j between j -> i and j -> k."""
    a, b = _legs(pos, ai, aj, ak)
    return np.clip((a * b).sum(1) / np.sqrt((a * a).sum(1) * (b * b).sum(1)), -1.0, 1.0)


def theta(pos, ai, aj, ak):
    """atan2(|a x b|, a . b): the angle the reference hands to F_B_2D."""
    a, b = _legs(pos, ai, aj, ak)
    return np.arctan2(np.sqrt((np.cross(a, b) ** 2).sum(1)), (a * b).sum(1))


def sph_y(c, nsph=NSPH_MAX):
    """[T, nsph] Y_l0 at cos(theta) = c."""
    c = _f64(c)
    return np.stack([math.sqrt((2 * l + 1) / (4 * math.pi)) * special.eval_legendre(l, c) for l in range(nsph)], axis=1)


def sbf(radial, trip_src, y, nrad):
    """[T, nsph * nrad] radial[trip_src] * Y repeated nrad times (l-major)."""
    return _f64(radial)[np.asarray(trip_src)] * np.repeat(_f64(y), nrad, axis=1)


def freq_grad(g, d, env, freq, cutoff=CUTOFF):
    """[R] sum_e g[e, n] env[e] cos(freq[n] x_e) x_e."""
    x = _f64(d) / cutoff
    return (_f64(g) * (_f64(env) * x)[:, None] * np.cos(_f64(freq)[None, :] * x[:, None])).sum(0)


# ------------------------------------------------------------------------------------------------ unit bounds
def dist_unit(d):
    return E32 * _f64(d)


def env_unit(d, cutoff=CUTOFF):
    x = _f64(d) / cutoff
    x_denv = -1.0 / x - 140.0 * x ** 5 + 288.0 * x ** 6 - 147.0 * x ** 7  # x env'(x)
    return E32 * (sum(env_terms(x)) + np.abs(x_denv))


def rbf_unit(d, freq, cutoff=CUTOFF):
    x = _f64(d) / cutoff
    phi = _f64(freq)[None, :] * x[:, None]
    s = np.abs(np.sin(phi))
    env_abs = np.abs(envelope(d, cutoff))[:, None]
    return E32 * env_abs * (s + np.abs(phi * np.cos(phi))) + s * env_unit(d, cutoff)[:, None]


def radial_unit(d, nsph, nrad, cutoff=CUTOFF):
    """The unit bound of bessel_env (module docstring), [E, nsph * nrad]."""
    from x2gnn import basis_consts as bc  # term magnitudes only

    zeros, norm = consts()
    x = _f64(d) / cutoff
    env_abs, a_sum = np.abs(envelope(d, cutoff)), sum(env_terms(x))
    cols = []
    for l in range(nsph):
        for n in range(nrad):
            u = zeros[l, n] * x
            b = norm[l, n] * special.spherical_jn(l, u)
            db = u * norm[l, n] * special.spherical_jn(l, u, derivative=True)
            m_sum = sum(np.abs(bc.COEF[l][n][m] * x ** m * (np.cos(u) if m & 1 else np.sin(u))) for m in range(l + 1))
            cols.append(E32 * (env_abs * (m_sum / x ** (l + 1) + np.abs(db)) + a_sum * np.abs(b)))
    return np.stack(cols, axis=1)


def cos_unit_pos(pos, ai, aj, ak):
    """cos(atan2(|a x b|, a . b)) in float32: the dot product's and the cross product's term magnitudes carried
    to cos theta (d cos = sin^2 d(dot)/|a||b| + sin |cos| d|cross|/|a||b|), the angle's own rounding and the
    cosine's."""
    a, b = _legs(pos, ai, aj, ak)
    ab = np.sqrt((a * a).sum(1) * (b * b).sum(1))
    c = cos_theta(pos, ai, aj, ak)
    th = theta(pos, ai, aj, ak)
    s = np.sqrt(np.maximum(1.0 - c * c, 0.0))
    dot_abs = np.abs(a * b).sum(1) / ab
    aa, bb = np.abs(a), np.abs(b)
    cross_abs = np.stack([aa[:, 1] * bb[:, 2] + aa[:, 2] * bb[:, 1], aa[:, 2] * bb[:, 0] + aa[:, 0] * bb[:, 2],
                          aa[:, 0] * bb[:, 1] + aa[:, 1] * bb[:, 0]], axis=1)
    cross_abs = np.sqrt((cross_abs ** 2).sum(1)) / ab
    return E32 * (s * s * dot_abs + s * np.abs(c) * cross_abs + th * s + np.abs(c))


def cos_unit_theta(th):
    th = _f64(th)
    return E32 * (np.abs(np.cos(th)) + np.abs(th * np.sin(th)))


def sph_y_unit(c, c_unit, nsph=NSPH_MAX):
    """[T, nsph]: the monomial terms' magnitudes sum_p |a_lp c^p| and the argument's own bound through Y'."""
    c = _f64(c)
    cols = []
    for l in range(nsph):
        pref = math.sqrt((2 * l + 1) / (4 * math.pi))
        leg = np.polynomial.legendre.Legendre.basis(l)
        mono = np.polynomial.legendre.leg2poly(leg.coef)
        terms = sum(np.abs(pref * mono[p] * c ** p) for p in range(l + 1))
        cols.append(E32 * terms + np.abs(pref * leg.deriv()(c)) * c_unit)  # (l = 0: Y' = 0)
    return np.stack(cols, axis=1)


def sbf_unit(radial, radial_u, trip_src, y, y_u, nrad):
    """unit(B env) |Y| + |B env| unit(Y), and the product's rounding."""
    src = np.asarray(trip_src)
    r, yy = _f64(radial)[src], np.repeat(_f64(y), nrad, axis=1)
    return _f64(radial_u)[src] * np.abs(yy) + np.abs(r) * np.repeat(_f64(y_u), nrad, axis=1) + E32 * np.abs(r * yy)


def freq_grad_unit(g, d, env, freq, base=None, cutoff=CUTOFF):
    """[R]: e32 sum|terms| for the summation, per term |t| + |t phi tan(phi)| (its roundings, the argument's), and
    the rounding of the accumulated result when the sum is added onto ``base``."""
    x = _f64(d) / cutoff
    phi = _f64(freq)[None, :] * x[:, None]
    amp = np.abs(_f64(g) * (_f64(env) * x)[:, None])
    t = amp * np.abs(np.cos(phi))
    u = E32 * (t.sum(0) + (t + amp * np.abs(phi * np.sin(phi))).sum(0))
    if base is not None:
        u = u + E32 * np.abs(_f64(base) + freq_grad(g, d, env, freq, cutoff))
    return u


# ------------------------------------------------------------------------------------------------ float32 emulation
F = np.float32


class Tables:
    """The constant tables the kernels read (x2gnn/basis_consts.py rounded to float32) and the envelope's x^6
    coefficient; ``perturbed`` returns a copy with one entry scaled (the bounds' self-check)."""

    def __init__(self):
        from x2gnn import basis_consts as bc

        self.zeros, self.coef, self.ycoef = np.array(bc.ZEROS, F), np.array(bc.COEF, F), np.array(bc.YCOEF, F)
        self.env6 = F(48.0)

    def perturbed(self, table, index, factor):
        t = Tables.__new__(Tables)
        t.zeros, t.coef, t.ycoef, t.env6 = self.zeros.copy(), self.coef.copy(), self.ycoef.copy(), self.env6
        if table == "env6":
            t.env6 = F(float(self.env6) * factor)
        else:
            getattr(t, table)[index] = getattr(t, table)[index] * F(factor)
        return t


def emu_dist(pos, src, dst):
    p = np.asarray(pos, F)
    dl = p[np.asarray(src)] - p[np.asarray(dst)]
    return np.sqrt(dl[:, 0] * dl[:, 0] + dl[:, 1] * dl[:, 1] + dl[:, 2] * dl[:, 2])


def emu_env(xs, tab):
    x2 = xs * xs
    x4 = x2 * x2
    x5 = x4 * xs
    x6 = x5 * xs
    x7 = x6 * xs
    return F(1.0) / xs + F(-28.0) * x5 + tab.env6 * x6 + F(-21.0) * x7


def emu_rbf(d, freq, tab, cutoff=CUTOFF):
    xs = np.asarray(d, F) * (F(1.0) / F(cutoff))
    return np.sin(np.asarray(freq, F)[None, :] * xs[:, None]) * emu_env(xs, tab)[:, None]


def emu_bessel_env(d, nsph, nrad, tab, cutoff=CUTOFF):
    d = np.asarray(d, F)
    env = emu_env(d * (F(1.0) / F(cutoff)), tab)
    x = d / F(cutoff)
    out = np.empty((d.shape[0], nsph * nrad), F)
    for l in range(nsph):
        xp = [np.ones_like(x)]
        for _ in range(l + 1):
            xp.append(xp[-1] * x)
        inv = F(1.0) / xp[l + 1]
        for n in range(nrad):
            u = tab.zeros[l, n] * x
            sn, cs = np.sin(u), np.cos(u)
            acc = np.zeros_like(x)
            for m in range(l, -1, -1):
                acc = acc + tab.coef[l, n, m] * xp[m] * (cs if m & 1 else sn)
            out[:, l * nrad + n] = env * (acc * inv)
    return out


def emu_cos_pos(pos, ai, aj, ak):
    p = np.asarray(pos, F)
    a, b = p[np.asarray(ai)] - p[np.asarray(aj)], p[np.asarray(ak)] - p[np.asarray(aj)]
    cosv = a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]
    cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return np.cos(np.arctan2(np.sqrt(cx * cx + cy * cy + cz * cz), cosv))


def emu_sph_y(c, tab, nsph=NSPH_MAX):
    c = np.asarray(c, F)
    c2 = c * c
    cols = []
    for l in range(nsph):
        acc = np.zeros_like(c)
        for p in range(l, -1, -2):
            acc = acc * c2 + tab.ycoef[l, p]
        cols.append(acc * c if l & 1 else acc)
    return np.stack(cols, axis=1)


def emu_sbf(radial, trip_src, y, nrad):
    return np.asarray(radial, F)[np.asarray(trip_src)] * np.repeat(np.asarray(y, F), nrad, axis=1)


def freq_grad_blocks(E):
    return min(max((E + 255) // 256, 1), 128)


def emu_freq_grad(g, d, env, freq, cutoff=CUTOFF):
    """Thread-strided partial sums, a 256-wide tree per block, then the block partials in order."""
    g, d, env, freq = (np.asarray(a, F) for a in (g, d, env, freq))
    E, R = g.shape
    x = d * (F(1.0) / F(cutoff))
    term = (g * env[:, None]) * (np.cos(freq[None, :] * x[:, None]) * x[:, None])
    stride = freq_grad_blocks(E) * 256
    passes = (E + stride - 1) // stride
    padded = np.zeros((passes * stride, R), F)
    padded[:E] = term
    acc = np.zeros((stride, R), F)
    for p in range(passes):
        acc = acc + padded[p * stride:(p + 1) * stride]
    acc = acc.reshape(-1, 256, R)
    off = 128
    while off:
        acc[:, :off] = acc[:, :off] + acc[:, off:2 * off]
        off >>= 1
    out = np.zeros(R, F)
    for b in range(acc.shape[0]):
        out = out + acc[b, 0]
    return out


# ------------------------------------------------------------------------------------------------ grids, geometries
SHAPES = [(7, 6), (7, 16), (3, 5), (1, 1), (7, 1), (2, 16)]  # (num_spherical, num_radial)
EDGE_COUNTS = [1, 63, 64, 65, 2001]
MAIN_E = 2001  # not a multiple of 64
D_EDGE = float(np.float32(5.0 * (1.0 - 2.0 ** -20)))


def main_grid(E=MAIN_E):
    """E distances on [1.0, 4.9999] Angstrom (one: mid-range)."""
    return np.linspace(1.0, 4.9999, E).astype(F) if E > 1 else np.array([2.5], F)


def short_grid():
    """The short-bond sweep: 257 distances on [0.5, 1.0)."""
    return np.linspace(0.5, 1.0, 257, endpoint=False).astype(F)


def edge_point():
    return np.array([D_EDGE], F)


def edge_star(d, seed=0):
    """Positions / edges whose distances are close to ``d``: atom 0 at the origin, atom e + 1 at d_e along a
    seeded direction (an axis when E == 1, so that d is hit exactly), edge e = (e + 1 -> 0)."""
    d = np.asarray(d, F)
    E = d.shape[0]
    rng = np.random.default_rng(seed + E)
    v = rng.standard_normal((E, 3))
    v /= np.sqrt((v * v).sum(1))[:, None]
    if E == 1:
        v[:] = (1.0, 0.0, 0.0)
    pos = np.concatenate([np.zeros((1, 3)), v * d[:, None].astype(np.float64)]).astype(F)
    return pos, np.arange(1, E + 1, dtype=np.int32), np.zeros(E, np.int32)


def perturbed_freq(R, seed=5):
    """pi n scaled by up to 10 % (trained frequencies are no multiples of pi)."""
    rng = np.random.default_rng(seed + R)
    return (math.pi * np.arange(1, R + 1) * (1.0 + 0.1 * rng.random(R))).astype(F)


class Geometry:
    """pos [N, 3] float32, directed edges, their float32 distances, and the oracle's triplets of them."""

    def __init__(self, name, pos, ei):
        self.name, self.pos, self.ei = name, np.ascontiguousarray(pos, F), np.asarray(ei, np.int64)
        trip, j, i, k = triplets.vertex_to_edge(self.ei, self.pos.shape[0])
        self.trip_src, self.ai, self.aj, self.ak = (np.ascontiguousarray(a, np.int32) for a in (trip[0], i, j, k))
        self.E, self.T = self.ei.shape[1], self.trip_src.shape[0]
        self.dist = dist(self.pos, self.ei[0], self.ei[1]).astype(F)

    def head(self, T):
        """The first T triplets (same atoms and edges)."""
        g = Geometry.__new__(Geometry)
        g.__dict__.update(self.__dict__)
        g.name, g.T = f"{self.name}[:{T}]", T
        g.trip_src, g.ai, g.aj, g.ak = self.trip_src[:T], self.ai[:T], self.aj[:T], self.ak[:T]
        return g


def _molecules(name, mols):
    """Join (pos [n, 3], undirected bonds) molecules into one Geometry with both directions of every bond."""
    pos, src, dst, base = [], [], [], 0
    for p, bonds in mols:
        pos.append(np.asarray(p, np.float64))
        for a, b in bonds:
            src += [base + a, base + b]
            dst += [base + b, base + a]
        base += len(p)
    return Geometry(name, np.concatenate(pos), np.array([src, dst]))


def _rotations(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.sqrt((q * q).sum(1))[:, None]
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)


@functools.lru_cache(maxsize=None)
def geometry(name):
    """``golden``: the two molecules of basis.npz.  ``angles``: three-atom molecules i - j - k (two triplets each)
    with the angle at j exactly 0, exactly pi, exactly pi / 2 (on the axes and along directions whose
    components are exact in float32) and within 1e-3 rad of 0 and of pi at seeded orientations.  ``star``: a
    centre with 40 neighbours, 1560 triplets that all read the centre's 40 outgoing rows, across 256-triplet
    blocks."""
    rng = np.random.default_rng(11)
    if name == "golden":
        from conftest import golden

        z = golden("basis.npz")
        g = Geometry(name, z["atom_pos"], z["edge_index"])
        assert np.array_equal(g.trip_src, z["trip"][0])
        return g
    if name == "angles":
        mols = []
        bonds = [(0, 1), (0, 2)]  # atom 0 is j
        o = np.zeros(3)
        for v in ([1.5, 0, 0], [0, 2.0, 0], [1.25, -0.75, 2.5], [0.375, 1.5, -1.125]):
            v = np.array(v)
            mols.append(([o, v, 2.0 * v], bonds))  # theta = 0
            mols.append(([o, v, -0.5 * v], bonds))  # theta = pi
        mols.append(([o, [1.5, 0, 0], [0, 2.5, 0]], bonds))  # theta = pi / 2
        mols.append(([o, [0, 0, 1.25], [3.0, 0, 0]], bonds))
        mols.append(([o, [1.5, 2.0, 0], [-2.0, 1.5, 0]], bonds))
        mols.append(([[1.0, 1.0, 1.0], [2.5, 3.0, 1.0], [0.0, 1.75, 3.0]], bonds))  # (1.5, 2, 0) . (-1, 0.75, 2) = 0
        n = 150
        rot = _rotations(rng, 2 * n)
        eps = np.concatenate([rng.uniform(1e-6, 1e-3, n), math.pi - rng.uniform(1e-6, 1e-3, n)])
        d1, d2 = rng.uniform(1.0, 3.0, 2 * n), rng.uniform(1.0, 3.0, 2 * n)
        for r in range(2 * n):
            a = rot[r] @ np.array([d1[r], 0.0, 0.0])
            b = rot[r] @ np.array([d2[r] * math.cos(eps[r]), d2[r] * math.sin(eps[r]), 0.0])
            shift = rng.uniform(-2, 2, 3)
            mols.append(([shift, shift + a, shift + b], bonds))
        return _molecules(name, mols)
    if name == "star":
        v = rng.standard_normal((40, 3))
        v *= (rng.uniform(1.0, 4.5, 40) / np.sqrt((v * v).sum(1)))[:, None]
        return _molecules(name, [(np.concatenate([np.zeros((1, 3)), v]), [(0, a) for a in range(1, 41)])])
    raise ValueError(name)


def radial_grids():
    """The distance grids of the radial tests, by name."""
    return dict(golden=geometry("golden").dist, main=main_grid(), short=short_grid(), edge=edge_point())


FREQ_GRAD_E = [1, 255, 257, 33025]  # 33 025 > 128 blocks x 256: the stride loop runs twice, the second pass ragged
SBF_NSPH, SBF_NRAD = (7, 3, 1), (6, 16, 1, 5, 8)  # num_radial 6 / 16: the templates; 1, 5, 8: the runtime instance
HEADS = (1, 255, 256, 257)  # triplet counts around the 256-triplet block


def freq_grad_case(E, R):
    """Seeded float32 inputs of x2g_edge_basis_freq_grad: (g [E, R], dist, env, freq, a non-zero dfreq to add to)."""
    rng = np.random.default_rng(1000 * R + E)
    d = rng.uniform(1.0, 4.9999, E).astype(F)
    return (rng.standard_normal((E, R)).astype(F), d, envelope(d).astype(F), perturbed_freq(R),
            rng.standard_normal(R).astype(F))


# ------------------------------------------------------------------------------------------------ reports
def _worst(table, key, ratio):
    table[key] = max(table.get(key, 0.0), float(np.max(ratio)))


def emulation_report(tab=None):
    """{output: worst |emulation - ref64| / unit bound} over every grid and geometry of the GPU tests (with the
    shipped tables when ``tab`` is None)."""
    tab = tab or Tables()
    out = {}
    for name, d in radial_grids().items():
        for ns, nr in SHAPES:
            _worst(out, "bessel_env", np.abs(emu_bessel_env(d, ns, nr, tab) - bessel_env(d, ns, nr)) /
                   radial_unit(d, ns, nr))
        if name == "golden":
            g = geometry("golden")
            pos, src, dst = g.pos, g.ei[0], g.ei[1]
        else:
            pos, src, dst = edge_star(d)
        d64, de = dist(pos, src, dst), emu_dist(pos, src, dst)
        _worst(out, "dist", np.abs(de - d64) / dist_unit(d64))
        _worst(out, "env", np.abs(emu_env(de * (F(1.0) / F(CUTOFF)), tab) - envelope(d64)) / env_unit(d64))
        for R in (1, 6, 16):
            f = perturbed_freq(R)
            _worst(out, "rbf", np.abs(emu_rbf(de, f, tab) - rbf(d64, f)) / rbf_unit(d64, f))
        for ns, nr in SHAPES:  # x2g_edge_basis: the Bessel terms at the distances it computes itself
            _worst(out, "bessel_env", np.abs(emu_bessel_env(de, ns, nr, tab) - bessel_env(d64, ns, nr)) /
                   radial_unit(d64, ns, nr))
    for name in ("golden", "angles", "star"):
        g = geometry(name)
        th32 = theta(g.pos, g.ai, g.aj, g.ak).astype(F)
        for path in ("pos", "theta"):
            if path == "pos":
                c, cu = cos_theta(g.pos, g.ai, g.aj, g.ak), cos_unit_pos(g.pos, g.ai, g.aj, g.ak)
                ce = emu_cos_pos(g.pos, g.ai, g.aj, g.ak)
            else:
                c, cu, ce = np.cos(_f64(th32)), cos_unit_theta(th32), np.cos(th32)
            y, yu, ye = sph_y(c), sph_y_unit(c, cu), emu_sph_y(ce, tab)
            _worst(out, "cos_theta", np.abs(ce - c) / cu)
            _worst(out, "sph_y", np.abs(ye - y) / yu)
            for ns in SBF_NSPH:
                for nr in SBF_NRAD:
                    rad, ru = bessel_env(g.dist, ns, nr), radial_unit(g.dist, ns, nr)
                    s = sbf(rad, g.trip_src, y[:, :ns], nr)
                    su = sbf_unit(rad, ru, g.trip_src, y[:, :ns], yu[:, :ns], nr)
                    se = emu_sbf(emu_bessel_env(g.dist, ns, nr, tab), g.trip_src, ye[:, :ns], nr)
                    _worst(out, "sbf", np.abs(se - s) / su)
    for E in FREQ_GRAD_E:
        for R in (6, 16):
            gg, d, ev, f, _ = freq_grad_case(E, R)
            _worst(out, "freq_grad", np.abs(emu_freq_grad(gg, d, ev, f) - freq_grad(gg, d, ev, f)) /
                   freq_grad_unit(gg, d, ev, f))
    return out


CAP_LEVEL, CAP_SHARE = 1e-3, 0.02


def cap_report():
    """On the main grid, per (output, shape): the share of comparisons whose bound K * unit exceeds CAP_LEVEL of
    their column's largest |value| (``share``), and that share per l for the Bessel terms (``by_l``)."""
    d = main_grid()
    pos, src, dst = edge_star(d)
    d64 = dist(pos, src, dst)
    rep = {}

    def share(ref, unit):
        ref, unit = ref.reshape(ref.shape[0], -1), unit.reshape(ref.shape[0], -1)
        return K * unit > CAP_LEVEL * np.abs(ref).max(0)[None, :]

    for ns, nr in SHAPES:
        for entry, dd in (("x2g_bessel_env", d), ("x2g_edge_basis", d64)):
            over = share(bessel_env(dd, ns, nr), radial_unit(dd, ns, nr))
            rep[f"{entry} bessel_env {ns}x{nr}"] = dict(
                share=float(over.mean()), by_l=[float(over[:, l * nr:(l + 1) * nr].mean()) for l in range(ns)])
    rep["x2g_edge_basis dist"] = dict(share=float(share(d64, dist_unit(d64)).mean()))
    rep["x2g_edge_basis env"] = dict(share=float(share(envelope(d64), env_unit(d64)).mean()))
    for R in (1, 6, 16):
        f = perturbed_freq(R)
        rep[f"x2g_edge_basis rbf R={R}"] = dict(share=float(share(rbf(d64, f), rbf_unit(d64, f)).mean()))
    return rep
