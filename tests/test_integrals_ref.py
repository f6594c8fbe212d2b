"""The float64 statement of the one-electron integrals (tests/integrals_ref.py) grounded independently of any recursion:
Szabo & Ostlund's H2 / STO-3G table, Gauss-Hermite product quadrature for overlap and kinetic integrals of p-d, d-f and
f-f primitive pairs, the Gauss transform of 1/r for their nuclear attraction, and structural properties.  Then the
host side of the feature: the two basis parsers, the binding table of include/x2g_integrals.h and the status codes the
entry point returns before any launch.  No GPU.
"""
import ctypes
import math
import os

import numpy as np
import pytest
from scipy import integrate

import ao_features_ref as ar
import integrals_ref as ir
from conftest import ROOT

OK, EINVAL, EUNSUPPORTED = 0, 1001, 1002
NAME = "x2g_one_electron_blocks"


# ------------------------------------------------------------------------------------------------- the textbook
def test_h2_sto3g_is_szabo_and_ostlunds_table():
    """Modern Quantum Chemistry, section 3.5.2: H2 at R = 1.4 bohr in STO-3G (zeta = 1.24), four decimals."""
    sym, pos = ir.h2()
    S, T, V = ir.one_electron(ir.STO3G_H, sym, pos / ir.BOHR, parts=True)
    V1 = ir.one_electron(ir.STO3G_H, sym, pos / ir.BOHR, parts=True, nuclei=[0])[2]
    got = dict(S12=S[0, 1], T11=T[0, 0], T12=T[0, 1], V1_11=V1[0, 0], V1_12=V1[0, 1], V1_22=V1[1, 1],
               H11=T[0, 0] + V[0, 0], H12=T[0, 1] + V[0, 1])
    want = dict(S12=0.6593, T11=0.7600, T12=0.2365, V1_11=-1.2266, V1_12=-0.5974, V1_22=-0.6538, H11=-1.1204,
                H12=-0.9584)
    print({k: round(float(v), 6) for k, v in got.items()})
    for k in want:
        assert abs(got[k] - want[k]) < 2e-4, (k, got[k])
    assert np.allclose(np.diag(S), 1.0, rtol=0, atol=1e-7)  # (the table's eight-digit coefficients)


# ------------------------------------------------------------------------------------------------- quadrature
PAIRS = [(1, 0.9, 2, 1.3), (2, 0.7, 3, 1.1), (3, 0.8, 3, 0.6)]  # (la, a, lb, b): p-d, d-f, f-f
A, B, C = np.array([0.1, -0.3, 0.2]), np.array([0.7, 0.4, -0.5]), np.array([-0.4, 0.6, 0.9])


def _poly(r, centre, powers):
    d = r - centre
    return d[..., 0] ** powers[0] * d[..., 1] ** powers[1] * d[..., 2] ** powers[2]


def _grad_poly(r, centre, powers, alpha):
    """The polynomial factors of grad(x^i y^j z^k exp(-alpha r^2)) / exp(-alpha r^2): [3, ...]."""
    d = r - centre
    out = []
    for k in range(3):
        low = list(powers)
        low[k] -= 1
        high = list(powers)
        high[k] += 1
        term = -2.0 * alpha * _poly(r, centre, high)
        if powers[k]:
            term = term + powers[k] * _poly(r, centre, low)
        out.append(term)
    return np.stack(out)


def _hermite_grid(q, Q, n=14):
    """Points and weights of int f(r) exp(-q |r - Q|^2) d^3r, exact for polynomials of degree < 2n per dimension."""
    x, w = np.polynomial.hermite.hermgauss(n)
    pts = np.stack(np.meshgrid(x, x, x, indexing="ij"), axis=-1) / math.sqrt(q) + Q
    wts = np.einsum("i,j,k->ijk", w, w, w) / q ** 1.5
    return pts, wts


@pytest.mark.parametrize("la,a,lb,b", PAIRS)
def test_overlap_and_kinetic_against_gauss_hermite(la, a, lb, b):
    p = a + b
    P = (a * A + b * B) / p
    K = math.exp(-a * b / p * ((A - B) ** 2).sum())
    pts, wts = _hermite_grid(p, P)
    S, T, _ = ir.primitive_block(la, a, A, lb, b, B, [C], [0.0])
    worst = 0.0
    for ia, pa in enumerate(ir.cart_components(la)):
        for ib, pb in enumerate(ir.cart_components(lb)):
            s = K * (wts * _poly(pts, A, pa) * _poly(pts, B, pb)).sum()
            t = 0.5 * K * (wts * (_grad_poly(pts, A, pa, a) * _grad_poly(pts, B, pb, b)).sum(axis=0)).sum()
            worst = max(worst, abs(S[ia, ib] - s), abs(T[ia, ib] - t))
    print(f"l = {la}, {lb}: worst |recursion - quadrature| {worst:.3g}")
    assert worst < 1e-12


@pytest.mark.parametrize("la,a,lb,b", PAIRS)
def test_nuclear_attraction_against_the_gauss_transform(la, a, lb, b):
    """1/r = 2/sqrt(pi) int_0^inf exp(-t^2 r^2) dt: each t gives a three-centre overlap, exact by Gauss-Hermite.
    Every Cartesian component pair of the shell pair, integrated together as one vector."""
    p = a + b
    P = (a * A + b * B) / p
    K = math.exp(-a * b / p * ((A - B) ** 2).sum())
    comps_a, comps_b = ir.cart_components(la), ir.cart_components(lb)

    def three_centre(t):
        q = p + t * t
        Q = (p * P + t * t * C) / q
        pts, wts = _hermite_grid(q, Q)
        pa = np.stack([_poly(pts, A, c) for c in comps_a])
        pb = np.stack([_poly(pts, B, c) for c in comps_b])
        return K * math.exp(-p * t * t / q * ((P - C) ** 2).sum()) * np.einsum("ijk,aijk,bijk->ab", wts, pa, pb)

    # t = s / (1 - s) maps [0, inf) to [0, 1); the integrand falls off as t^-3 at least, so the mapped one is bounded
    val, err = integrate.quad_vec(lambda s: three_centre(s / (1.0 - s)) / (1.0 - s) ** 2, 0.0, 1.0 - 1e-12,
                                  epsabs=1e-13, epsrel=1e-12, limit=400)
    want = -2.0 / math.sqrt(math.pi) * val
    _, _, V = ir.primitive_block(la, a, A, lb, b, B, [C], [1.0])
    worst = float(np.abs(V - want).max())
    print(f"l = {la}, {lb}: {V.size} components, worst |recursion - Gauss transform| {worst:.3g} (quad error {err:.1g})")
    assert V.shape == want.shape == (len(comps_a), len(comps_b))
    assert worst < 1e-10


def test_boys_function_against_its_integral():
    for n in (0, 3, 6):
        for x in (0.0, 1e-8, 0.05, 0.1, 0.5, 5.0, 20.0, 35.0, 1e3):
            want = integrate.quad(lambda t: t ** (2 * n) * math.exp(-x * t * t), 0.0, 1.0, epsabs=0, epsrel=1e-13)[0]
            assert abs(ir.boys(n, np.array([x]))[0] - want) <= 1e-12 * want, (n, x)


# ------------------------------------------------------------------------------------------------- structure
def test_structure_of_the_reference_matrices():
    sym, pos, S, H = ir.reference("mol3")
    assert S.shape == (61, 61)
    assert np.abs(np.diag(S) - 1.0).max() <= 1e-12
    # (the statement mirrors shell pairs; a shell's block with itself is symmetric up to float64 rounding)
    assert np.abs(S - S.T).max() <= 1e-15 and np.abs(H - H.T).max() <= 1e-15 * np.abs(H).max()
    assert np.linalg.eigvalsh(S).min() > 0
    moved = ir.one_electron(ir.SYNTH, sym, (pos + np.array([3.0, -2.0, 0.7])) / ir.BOHR)
    assert np.abs(moved[0] - S).max() < 1e-11 and np.abs(moved[1] - H).max() < 1e-10 * np.abs(H).max()


def test_the_features_do_not_change_under_a_rotation():
    """For the block shapes the features place on their groups, (39, 39), (39, 9) and (9, 9), every cell is a norm
    over whole shells or a value among s functions.  A (9, 39) block and every other shape go to (0, 0), where
    hydrogen's p functions fall on the single-index cells (include/x2g_features.h: the reference's branch for that
    shape is never taken): those rows do change, and are left out."""
    sym, pos = ["O", "H", "H"], np.array([[0.0, 0.05, -0.1], [0.75, 0.62, 0.1], [-0.8, 0.5, 0.3]])
    S, H = ir.one_electron(ir.SYNTH, sym, pos / ir.BOHR)
    Sr, Hr = ir.one_electron(ir.SYNTH, sym, (pos @ ir.random_rotation(3).T) / ir.BOHR)
    assert np.abs(Sr - S).max() > 1e-3  # the matrices do change
    sl = ir.aoslice(ir.SYNTH, sym)
    ei = ar.all_directed_edges(3, self_loops=True)
    f0 = ar.edge_features(S, H, sl, ei, nelectron=10)
    f1 = ar.edge_features(Sr, Hr, sl, ei, nelectron=10)
    aligned = ir.aligned_edges(sym, ei)
    assert aligned.sum() == 7 and not aligned[[3, 6]].any()  # all but H -> O
    # the rounding of every element to float32 inside the features: 6e-8 relative, through a norm of up to 49
    np.testing.assert_allclose(f1[aligned], f0[aligned], rtol=2e-6, atol=1e-8)
    assert np.abs(f1[~aligned] - f0[~aligned]).max() > 1e-3


# ------------------------------------------------------------------------------------------------- the parsers
TABLES = ("elem_shell", "shell_l", "shell_prim", "shell_ao", "prim_exp", "prim_coef", "elem_nao", "elem_nshell")


def test_pyscf_dict_and_nwchem_text_give_equal_tables():
    import x2gnn

    a = x2gnn.Basis.from_pyscf(ir.SYNTH)
    b = x2gnn.Basis.from_nwchem(ir.to_nwchem(ir.SYNTH))
    assert a.symbols == b.symbols == list(ir.SYNTH)
    for k in TABLES:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.elem_nao.tolist() == [39, 39, 39, 39, 9, 13] and a.elem_nshell.tolist() == [13, 13, 13, 13, 5, 7]
    assert a.table().dtype == np.int32 and len(a.table()) == len(a) + 1 + 3 * len(a.shell_l) + 1


def test_sorting_general_contractions_sp_blocks_and_normalisation():
    import x2gnn

    full = x2gnn.Basis.from_pyscf(ir.SYNTH)
    li = x2gnn.Basis.from_nwchem(ir.SYNTH_LI_NWCHEM)
    assert li.symbols == ["Li"] and li.shell_l.tolist() == [0, 0, 0, 0, 0, 1, 2]
    assert li.shell_ao.tolist() == [0, 1, 2, 3, 4, 5, 8] and li.elem_nao.tolist() == [13]
    assert np.diff(li.shell_prim).tolist() == [4, 4, 2, 1, 1, 2, 1]  # two columns, the SP block's s, ..., its p, d
    k = full.symbols.index("Li")
    s0, s1 = full.elem_shell[k], full.elem_shell[k + 1]
    p0, p1 = full.shell_prim[s0], full.shell_prim[s1]
    assert np.array_equal(full.prim_exp[p0:p1], li.prim_exp) and np.array_equal(full.prim_coef[p0:p1], li.prim_coef)
    # heavy atoms: sorted by l, stably (the 6-primitive s first, the 3-primitive s second, as in the file)
    c0, c1 = full.elem_shell[0], full.elem_shell[1]
    assert full.shell_l[c0:c1].tolist() == [0] * 5 + [1] * 4 + [2] * 3 + [3]
    assert np.diff(full.shell_prim[c0:c1 + 1]).tolist() == [6, 3, 1, 1, 1, 3, 1, 1, 1, 1, 1, 1, 1]
    # the statement's own normalisation, made apart from the package's
    for sym in ir.SYNTH:
        e = full.symbols.index(sym)
        lo, hi = full.shell_prim[full.elem_shell[e]], full.shell_prim[full.elem_shell[e + 1]]
        want = np.concatenate([d for _, _, d in ir.atom_shells(ir.SYNTH, sym)])
        np.testing.assert_allclose(full.prim_coef[lo:hi], want, rtol=1e-14, atol=0)
    assert np.array_equal(full.elements([9, 1, 3]), [3, 4, 5])


@pytest.mark.parametrize("basis,match", [
    ({"C": [[4, [1.0, 1.0]]]}, "C.*l = 4"),
    ({"N": ir.SYNTH["N"] + [[0, [0.3, 1.0]]]}, "N.*40 functions"),
    ({"O": [[0, [1.0, 1.0], [-2.0, 0.5]]]}, "O.*not positive"),
    ({"O": [[0, [0.0, 1.0]]]}, "O.*not positive"),
    ({"F": []}, "F.*no shell"),
])
def test_basis_errors_name_the_element(basis, match):
    import x2gnn

    with pytest.raises(ValueError, match=match):
        x2gnn.Basis.from_pyscf(basis)


@pytest.mark.parametrize("text,match", [
    ("C G\n 1.0 1.0\n", "C.*l = 4"),
    ("O S\n -1.0 1.0\n", "O.*not positive"),
    ("H S\n", "H"),
    ("H S\n 1.0 1.0\nF P\n", "F"),
    (ir.to_nwchem({"N": ir.SYNTH["N"] + [[0, [0.3, 1.0]]]}), "N.*40 functions"),
])
def test_nwchem_errors_name_the_element(text, match):
    import x2gnn

    with pytest.raises(ValueError, match=match):
        x2gnn.Basis.from_nwchem(text)


def test_an_element_outside_the_basis_raises():
    import x2gnn

    with pytest.raises(ValueError, match="no element N"):
        x2gnn.Basis.from_pyscf(ir.STO3G_H).elements([1, 7])


def test_geom_scf_6_refuses_a_text_without_atoms_and_a_fifth_column():
    import x2gnn

    basis = x2gnn.Basis.from_pyscf(ir.STO3G_H)
    with pytest.raises(ValueError, match="no atom line"):
        x2gnn.geom_scf_6("0\nnothing\n", basis)
    with pytest.raises(ValueError, match="atom line"):
        x2gnn.geom_scf_6("1\nlabel\nH 0.0 0.0 0.0 0.25\n", basis)


def test_geometry_is_parsed_in_float64_after_two_lines():
    from x2gnn.integrals import parse_geometry

    sym, xyz = parse_geometry("2\n-1.5\nh 0.1234567890123 0 0\nO1 1 2 3.5\n")
    assert sym == ["H", "O"] and xyz.dtype == np.float64 and xyz[0, 0] == 0.1234567890123 and xyz[1, 2] == 3.5
    with pytest.raises(ValueError, match="atom line"):
        parse_geometry("1\n0\nH 0 0\n")


# ------------------------------------------------------------------------------------------------- the binding
def test_binding_table_and_exports():
    import x2gnn
    from x2gnn import _lib, integrals

    assert list(_lib.INTEGRALS_SIGNATURES) == [NAME] and list(_lib.INTEGRALS_RESTYPES) == [NAME]
    for table in (_lib.SIGNATURES, _lib.STAGED_SIGNATURES, _lib.MULTI_SIGNATURES, _lib.CONV_SIGNATURES,
                  _lib.ATOMCTX_SIGNATURES, _lib.TRAIN_SIGNATURES, _lib.FEATURES_SIGNATURES, _lib.GRAPH_SIGNATURES):
        assert NAME not in table
    P, I = ctypes.c_void_p, ctypes.c_int64
    assert _lib.INTEGRALS_SIGNATURES[NAME] == [P] * 4 + [I] * 3 + [P] * 8 + [I] * 3 + [P, I, P, P, P]
    assert _lib.INTEGRALS_RESTYPES[NAME] is ctypes.c_int
    assert getattr(_lib.load(), NAME).argtypes == _lib.INTEGRALS_SIGNATURES[NAME]
    for name in ("Basis", "one_electron_matrices", "geom_scf_6"):
        assert name in x2gnn.__all__ and getattr(x2gnn, name) is getattr(integrals, name)


def test_the_header_declares_functions_only_and_leaves_the_abi_alone():
    from x2gnn import _lib

    with open(os.path.join(ROOT, "include", "x2g_integrals.h")) as f:
        sig, res, structs, consts = _lib.parse_header(f.read())
    assert not structs and not consts and list(sig) == [NAME]
    with open(os.path.join(ROOT, "include", "x2g.h")) as f:
        own = _lib.parse_header(f.read())[0]
    assert _lib.SIGNATURES == own and NAME not in own
    assert _lib.load().x2g_abi_version() == 18


# ------------------------------------------------------------------------------------------------- status codes
ADDR = 0x10000  # never dereferenced: every case below is refused, or returns, before a launch
BIG = 1 << 31
PTRS = ("basis_tab", "prim_exp", "prim_coef", "atom_pos", "atom_charge", "atom_elem", "atom_mol", "ao_begin",
        "atom_start", "mat_start", "mol_nao", "pairs", "ovlp", "hcore")


def _table(elem_shell, shell_l, shell_prim, shell_ao):
    return np.ascontiguousarray(np.concatenate([elem_shell, shell_l, shell_prim, shell_ao]).astype(np.int32))


GOOD = ([0, 2], [0, 1], [0, 3, 4], [0, 1])  # one element: an s shell of 3 primitives and a p shell of 1


def _call(tab=GOOD, host=True, n_elem=1, n_shells=2, n_prims=4, M=1, N=2, elems=16, P=0, **null):
    from x2gnn import _lib

    host_tab = _table(*tab)
    a = {k: ctypes.c_void_p(ADDR) for k in PTRS}
    a.update({k: None for k in null})
    return _lib.load().x2g_one_electron_blocks(
        a["basis_tab"], host_tab.ctypes.data_as(ctypes.c_void_p) if host else None, a["prim_exp"], a["prim_coef"],
        n_elem, n_shells, n_prims, a["atom_pos"], a["atom_charge"], a["atom_elem"], a["atom_mol"], a["ao_begin"],
        a["atom_start"], a["mat_start"], a["mol_nao"], M, N, elems, a["pairs"], P, a["ovlp"], a["hcore"], None)


def test_no_pairs_is_ok_without_a_launch():
    assert _call() == OK
    assert _call(M=0, N=0, elems=0) == OK


@pytest.mark.parametrize("name", PTRS)
def test_a_null_pointer_is_einval(name):
    assert _call(**{name: True}) == EINVAL
    assert _call(P=3, **{name: True}) == EINVAL


@pytest.mark.parametrize("kw", [dict(host=False), dict(n_elem=-1), dict(n_shells=-1), dict(n_prims=-1), dict(M=-1),
                                dict(N=-1), dict(elems=-1), dict(P=-1),
                                dict(tab=([0, 2], [0, 1], [0, 3, 2], [0, 1])),      # primitive ranges go backwards
                                dict(tab=([0, 2], [0, 1], [0, 3, 5], [0, 1])),      # and do not end at n_prims
                                dict(tab=([1, 2], [0, 1], [0, 3, 4], [0, 1])),      # the shells do not start at 0
                                dict(tab=([0, 2], [0, -1], [0, 3, 4], [0, 1])),     # a negative l
                                dict(tab=([0, 2], [0, 1], [0, 3, 4], [0, 2]))])     # a gap between the functions
def test_bad_counts_and_tables_are_einval(kw):
    assert _call(**kw) == EINVAL


@pytest.mark.parametrize("kw", [
    dict(tab=([0, 2], [0, 4], [0, 3, 4], [0, 1])),                                              # l = 4
    dict(tab=([0, 6], [3] * 6, list(range(7)), [7 * k for k in range(6)]), n_shells=6, n_prims=6),  # 42 functions
    dict(N=BIG), dict(P=BIG // 4), dict(P=1 << 40), dict(n_prims=BIG), dict(n_shells=BIG), dict(n_elem=BIG),
])
def test_what_the_kernel_cannot_index_is_eunsupported(kw):
    assert _call(**kw) == EUNSUPPORTED


def test_null_wins_over_unsupported_and_nothing_is_read():
    assert _call(N=BIG, ovlp=True) == EINVAL
    assert _call(tab=([0, 2], [0, 4], [0, 3, 4], [0, 1]), pairs=True) == EINVAL


def test_cpu_tensors_raise():
    import torch

    import x2gnn

    basis = x2gnn.Basis.from_pyscf(ir.STO3G_H)
    with pytest.raises(RuntimeError, match="GPU"):
        x2gnn.one_electron_matrices(torch.zeros((2, 3), dtype=torch.float64), [1, 1], [0, 2], basis)
    with pytest.raises(RuntimeError, match="GPU"):
        x2gnn.DeviceDataset.from_records([], basis, "cpu")
