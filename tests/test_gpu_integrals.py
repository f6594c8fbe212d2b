"""The one-electron integrals (csrc/integrals.hip, include/x2g_integrals.h) on the GPU through the raw ABI and through
``x2gnn.one_electron_matrices`` / ``geom_scf_6`` / ``DeviceDataset.from_records(records, basis)``, against the float64
statement of tests/integrals_ref.py (grounded by tests/test_integrals_ref.py).

The bound is |got - ref| <= 1e-9 max(1, |ref|) for every element of S and H: the consumer, the edge features, rounds
every element to float32 (relative step 6e-8), and 1e-9 is 1/60 of that, far above what float64 recursions should
leave.  Everything else is an identity.  The largest molecule has 5 atoms and 165 functions.
"""
import ctypes

import numpy as np
import pytest
import torch

import ao_features_ref as ar
import integrals_ref as ir

pytestmark = pytest.mark.gpu

BOUND = 1e-9
BOYS_SWITCH = 20.0  # csrc/integrals.hip kBoysSwitch: series and downward recursion below, erf and upward from here on
TEXTBOOK = dict(S12=0.6593, T11=0.7600, T12=0.2365, H11=-1.1204, H12=-0.9584)  # Szabo & Ostlund, H2 at 1.4 bohr in STO-3G


def _within(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    dev = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    return float(dev.max()) if dev.size else 0.0


@pytest.fixture(scope="module")
def basis():
    import x2gnn

    return x2gnn.Basis.from_pyscf(ir.SYNTH)


def _run(basis, cuda, mols, pairs=None):
    """one_electron_matrices of [(symbols, pos in angstrom)]."""
    import x2gnn

    Z = np.concatenate([[ir.Z_OF[s] for s in sym] for sym, _ in mols])
    pos = np.concatenate([p for _, p in mols])
    start = np.concatenate([[0], np.cumsum([len(sym) for sym, _ in mols])])
    return x2gnn.one_electron_matrices(torch.from_numpy(pos).to(cuda), Z, start, basis, pairs=pairs)


def _mats(ao, m=0):
    nao, s = int(ao.mol_nao[m]), int(ao.mat_start[m])
    return (ao.ovlp[s:s + nao * nao].cpu().numpy().reshape(nao, nao),
            ao.hcore[s:s + nao * nao].cpu().numpy().reshape(nao, nao))


@pytest.fixture(scope="module")
def mol5_all(basis, cuda):
    sym, pos, _, _ = ir.reference("mol5")
    return _run(basis, cuda, [(sym, pos)])


# ------------------------------------------------------------------------------------------------- 1. H2 / STO-3G
def test_h2_sto3g_textbook_and_reference(cuda):
    import x2gnn

    sym, pos, S_ref, H_ref = ir.reference("h2")
    S, H = _mats(_run(x2gnn.Basis.from_pyscf(ir.STO3G_H), cuda, [(sym, pos)]))
    _, T_ref, _ = ir.one_electron(ir.STO3G_H, sym, pos / ir.BOHR, parts=True)
    print(f"H2: S12 {S[0, 1]:.6f} H11 {H[0, 0]:.6f} H12 {H[0, 1]:.6f}; worst {max(_within(S, S_ref), _within(H, H_ref)):.3g}")
    assert abs(S[0, 1] - TEXTBOOK["S12"]) < 2e-4
    assert abs(H[0, 0] - TEXTBOOK["H11"]) < 2e-4 and abs(H[0, 1] - TEXTBOOK["H12"]) < 2e-4
    assert abs(T_ref[0, 0] - TEXTBOOK["T11"]) < 2e-4 and abs(T_ref[0, 1] - TEXTBOOK["T12"]) < 2e-4
    assert _within(S, S_ref) <= BOUND and _within(H, H_ref) <= BOUND
    assert np.array_equal(S, S.T) and np.array_equal(H, H.T)


# ------------------------------------------------------------------------------------------------- 2. five atoms
def test_five_atoms_all_pairs(mol5_all):
    _, _, S_ref, H_ref = ir.reference("mol5")
    S, H = _mats(mol5_all)
    assert S.shape == (165, 165)
    print(f"mol5: worst deviation S {_within(S, S_ref):.3g}, H {_within(H, H_ref):.3g}")
    assert _within(S, S_ref) <= BOUND
    assert _within(H, H_ref) <= BOUND
    assert np.abs(np.diag(S) - 1.0).max() <= 1e-12
    assert np.array_equal(S, S.T) and np.array_equal(H, H.T)
    assert mol5_all.hcore_div.cpu().tolist() == [6.0 + 7 + 8 + 9 + 1]
    assert np.array_equal(np.stack([mol5_all.ao_begin.cpu().numpy(), mol5_all.ao_end.cpu().numpy()], axis=1),
                          ir.aoslice(ir.SYNTH, ["C", "N", "O", "F", "H"])[:, 2:])


# ------------------------------------------------------------------------------------------------- 3. Boys sweep
BOYS_X = [0.0, 1e-8, 1e-3, 0.5, 5.0, 12.0, 25.0, 35.0, 50.0, 100.0, 1e3, 1e5, BOYS_SWITCH - 1e-6, BOYS_SWITCH,
          BOYS_SWITCH + 1e-6]
SWEEP_BASIS = {"C": [[0, [1.1, 1.0]], [3, [0.9, 1.0]]], "F": [[0, [2.0, 1.0]]]}


def test_boys_sweep(cuda):
    """Two atoms with one s and one f primitive each, 1.2 bohr apart, and a one-primitive nucleus on a line through
    their midpoint (the centre P of the s-s and of the f-f product) at the distance that makes x = p |P - C|^2 the
    listed value, once for the s-s pair's p = 2.2 and once for the f-f pair's p = 1.8."""
    import x2gnn

    sweep = x2gnn.Basis.from_pyscf(SWEEP_BASIS)
    A, B = np.array([0.0, 0.0, -0.6]), np.array([0.0, 0.0, 0.6])
    line = np.array([0.6, -0.48, 0.64])  # unit vector, off every axis
    mols = []
    for p in (2.2, 1.8):
        for x in BOYS_X:
            mols.append((["C", "C", "F"], np.stack([A, B, line * np.sqrt(x / p)]) * ir.BOHR))
    ao = _run(sweep, cuda, mols)
    worst = 0.0
    for m, (sym, pos) in enumerate(mols):
        S_ref, H_ref = ir.one_electron(SWEEP_BASIS, sym, pos / ir.BOHR)
        S, H = _mats(ao, m)
        dev = max(_within(S, S_ref), _within(H, H_ref))
        worst = max(worst, dev)
        assert dev <= BOUND, (m, BOYS_X[m % len(BOYS_X)], dev)
    print(f"Boys sweep: worst deviation {worst:.3g} over {len(mols)} placements")


# ------------------------------------------------------------------------------------------------- 4. batching
def test_a_molecule_in_a_batch_is_the_molecule_alone(basis, cuda, mol5_all):
    cases = [ir.reference(n)[:2] for n in ("mol5", "mol3")] + [(["H", "H"], ir.h2()[1])]
    cases = [cases[0], cases[2], cases[1]]
    both = _run(basis, cuda, cases)
    assert both.mol_nao.cpu().tolist() == [165, 18, 61]
    for m, case in enumerate(cases):
        alone = mol5_all if m == 0 else _run(basis, cuda, [case])
        for got, want in zip(_mats(both, m), _mats(alone)):
            assert np.array_equal(got, want), m
    _, _, S_ref, H_ref = ir.reference("mol3")
    S, H = _mats(both, 2)
    assert _within(S, S_ref) <= BOUND and _within(H, H_ref) <= BOUND


# ------------------------------------------------------------------------------------------------- 5. pairs
def test_pairs_subset(basis, cuda, mol5_all):
    sym, pos, _, _ = ir.reference("mol5")
    listed = [(0, 1), (1, 0), (2, 4), (4, 2), (0, 1), (3, 3)]
    got = _run(basis, cuda, [(sym, pos)], pairs=torch.tensor(listed, device=cuda).T.contiguous())
    sl = ir.aoslice(ir.SYNTH, sym)[:, 2:]
    mask = np.zeros((165, 165), bool)
    for i, j in listed:
        mask[sl[i, 0]:sl[i, 1], sl[j, 0]:sl[j, 1]] = True
        mask[sl[j, 0]:sl[j, 1], sl[i, 0]:sl[i, 1]] = True
    for part, full in zip(_mats(got), _mats(mol5_all)):
        assert np.array_equal(part[mask], full[mask])
        assert (part[~mask] == 0).all()


def test_cross_molecule_and_outside_pairs_raise(basis, cuda):
    cases = [ir.reference("mol3")[:2], (["H", "H"], ir.h2()[1])]
    for bad in ([[0], [3]], [[1], [5]], [[-1], [0]]):
        with pytest.raises(ValueError, match="share a molecule"):
            _run(basis, cuda, cases, pairs=torch.tensor(bad, device=cuda))
    with pytest.raises(RuntimeError, match="GPU"):
        _run(basis, cuda, cases, pairs=torch.tensor([[0], [1]]))
    with pytest.raises(RuntimeError, match="GPU"):
        import x2gnn

        x2gnn.one_electron_matrices(torch.zeros((2, 3), dtype=torch.float64), [1, 1], [0, 2], basis)


def test_raw_abi_skips_a_bad_pair_and_leaves_its_neighbours(basis, cuda, mol5_all):
    from x2gnn import _lib

    sym, pos, _, _ = ir.reference("mol5")
    Z = np.array([ir.Z_OF[s] for s in sym])
    N, total = 5, 165 * 165
    tab, pexp, pcoef = basis.device_tables(cuda)
    host_tab = basis.table()

    def dev(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(cuda)

    bohr = dev(pos / ir.BOHR, np.float64)
    z, elem, mol = dev(Z, np.int32), dev(basis.elements(Z), np.int32), dev(np.zeros(N), np.int32)
    start = dev([0, N], np.int64)
    pairs = dev([[0, 7, -1, 4, 1 << 40, 2], [1, 0, 2, 2, 3, N]], np.int64)
    SENT = -777.25
    ovlp = torch.full((total,), SENT, dtype=torch.float64, device=cuda)
    hcore = torch.full((total,), SENT, dtype=torch.float64, device=cuda)
    p, i64 = _lib.ptr, ctypes.c_int64
    _lib.call("x2g_one_electron_blocks", p(tab), host_tab.ctypes.data_as(ctypes.c_void_p), p(pexp), p(pcoef),
              i64(len(basis)), i64(len(basis.shell_l)), i64(len(basis.prim_exp)), p(bohr), p(z), p(elem), p(mol),
              p(mol5_all.ao_begin), p(start), p(mol5_all.mat_start), p(mol5_all.mol_nao), i64(1), i64(N), i64(total),
              p(pairs), i64(pairs.shape[1]), p(ovlp), p(hcore), _lib.stream_ptr())
    sl = ir.aoslice(ir.SYNTH, sym)[:, 2:]
    mask = np.zeros((165, 165), bool)
    for i, j in ((0, 1), (4, 2)):
        mask[sl[i, 0]:sl[i, 1], sl[j, 0]:sl[j, 1]] = True
        mask[sl[j, 0]:sl[j, 1], sl[i, 0]:sl[i, 1]] = True
    for part, full in zip((ovlp, hcore), _mats(mol5_all)):
        part = part.cpu().numpy().reshape(165, 165)
        assert np.array_equal(part[mask], full[mask])
        assert (part[~mask] == SENT).all()
    # a molecule whose matrix would not fit the arrays, or whose atom range leaves [0, N], is skipped whole
    for kw in (dict(total=total - 1), dict(start=[0, N + 1])):
        ovlp.fill_(SENT)
        other_start = dev(kw.get("start", [0, N]), np.int64)
        _lib.call("x2g_one_electron_blocks", p(tab), host_tab.ctypes.data_as(ctypes.c_void_p), p(pexp), p(pcoef),
                  i64(len(basis)), i64(len(basis.shell_l)), i64(len(basis.prim_exp)), p(bohr), p(z), p(elem), p(mol),
                  p(mol5_all.ao_begin), p(other_start), p(mol5_all.mat_start),
                  p(mol5_all.mol_nao), i64(1), i64(N), i64(kw.get("total", total)), p(pairs), i64(pairs.shape[1]),
                  p(ovlp), p(hcore), _lib.stream_ptr())
        assert bool((ovlp == SENT).all()), kw


# ------------------------------------------------------------------------------------------------- 6. features
def test_features_of_device_matrices_and_of_the_rotated_molecule(basis, cuda, mol5_all):
    from x2gnn.features import AOMatrices, ao_edge_features

    sym, pos, S_ref, H_ref = ir.reference("mol5")
    ei = torch.from_numpy(ar.all_directed_edges(5)).to(cuda)
    ref_ao = AOMatrices.from_molecules([(S_ref, H_ref, ir.aoslice(ir.SYNTH, sym), 31)]).to(cuda)
    want = ao_edge_features(ref_ao, ei, ref_ao.atom_mol()).cpu().numpy()
    got = ao_edge_features(mol5_all, ei, mol5_all.atom_mol()).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-8)
    # rotated: the rows whose block sits on the features' shell groups (all but H -> heavy, whose (9, 39) block the
    # reference places at (0, 0): tests/test_integrals_ref.py shows on the statement that those rows do change)
    rotated = _run(basis, cuda, [(sym, pos @ ir.random_rotation(11).T)])
    rot = ao_edge_features(rotated, ei, rotated.atom_mol()).cpu().numpy()
    aligned = ir.aligned_edges(sym, ei.cpu().numpy())
    assert aligned.sum() == 16
    np.testing.assert_allclose(rot[aligned], want[aligned], rtol=2e-6, atol=1e-8)
    assert not np.array_equal(_mats(rotated)[0], _mats(mol5_all)[0])  # (the matrices themselves do change)


# ------------------------------------------------------------------------------------------------- 7. geom_scf_6
GEOM = """3
-76.4 some label
O 0.1234567890123 -0.2000000001 0.05
H 0.9876543210987 0.3 -0.4000000002
Li 1.9 1.05 0.2
"""


def test_geom_scf_6(basis, cuda):
    import x2gnn

    S, Hd, sl = x2gnn.geom_scf_6(GEOM, basis)
    sym = ["O", "H", "Li"]
    assert S.dtype == Hd.dtype == torch.float64 and S.device.type == Hd.device.type == "cpu"
    assert tuple(S.shape) == tuple(Hd.shape) == (61, 61)
    assert isinstance(sl, np.ndarray) and sl.dtype.kind == "i" and np.array_equal(sl, ir.aoslice(ir.SYNTH, sym))
    assert sl[:, :2].tolist() == [[0, 13], [13, 18], [18, 25]]
    pos = np.array([[0.1234567890123, -0.2000000001, 0.05], [0.9876543210987, 0.3, -0.4000000002], [1.9, 1.05, 0.2]])
    exact = _run(basis, cuda, [(sym, pos)])
    assert np.array_equal(S.numpy(), _mats(exact)[0])
    assert torch.equal(Hd, torch.from_numpy(_mats(exact)[1]) / 12)  # the float64 division by 8 + 1 + 3 electrons
    rounded = _run(basis, cuda, [(sym, pos.astype(np.float32).astype(np.float64))])
    assert not np.array_equal(S.numpy(), _mats(rounded)[0])  # the text's digits, not float32's
    S_ref, H_ref = ir.one_electron(ir.SYNTH, sym, pos / ir.BOHR)
    assert _within(S.numpy(), S_ref) <= BOUND and _within(Hd.numpy() * 12, H_ref) <= BOUND


# ------------------------------------------------------------------------------------------------- 8. dataset
def _records():
    from x2gnn import datasets as ds

    rng = np.random.default_rng(8)
    out = []
    for k, sym in enumerate((["C", "H", "H", "O", "N", "H"], ["F", "H"], ["N", "C", "H", "O"])):
        pos = np.cumsum(rng.uniform(0.55, 0.95, size=(len(sym), 3)) * rng.choice([-1.0, 1.0], size=(len(sym), 3)), axis=0)
        text = f"{len(sym)}\n{-40.5 - k}\n" + "".join(f"{s} {x!r} {y!r} {z!r}\n" for s, (x, y, z) in zip(sym, pos.tolist()))
        out.append(ds.MolRecord(atom=text, R=torch.from_numpy(pos.astype(np.float32)),
                                Z=torch.tensor([ir.Z_OF[s] for s in sym]), N=torch.tensor([len(sym)]),
                                Label=torch.tensor([-40.5 - k]), idx=torch.tensor([k])))
    return out


def test_dataset_from_a_basis(basis, cuda):
    import x2gnn
    from x2gnn import datasets as ds
    from x2gnn.integrals import parse_geometry

    records = _records()
    pos = np.concatenate([parse_geometry(r.atom)[1] for r in records])
    assert pos.dtype == np.float64 and not np.array_equal(pos, pos.astype(np.float32))
    Z = np.concatenate([r.Z.numpy() for r in records])
    start = np.concatenate([[0], np.cumsum([len(r.Z) for r in records])])
    full = x2gnn.one_electron_matrices(torch.from_numpy(pos).to(cuda), Z, start, basis)
    want = x2gnn.DeviceDataset.from_records(records, full, cuda)
    for kw in (dict(), dict(max_edges_per_launch=1)):
        got = x2gnn.DeviceDataset.from_records(records, basis, cuda, **kw)
        assert got.edge_attr.shape == want.edge_attr.shape and got.edge_attr.shape[0] > 0
        assert torch.equal(got.edge_attr, want.edge_attr)
        assert bool(torch.isfinite(got.edge_attr).all())
        for name in ("x", "atom_pos", "edge_index", "y", "mol_trips"):
            assert torch.equal(getattr(got, name), getattr(want, name)), name
        for name in ("nodes", "edges", "triplets", "max_degree", "symmetric", "atom_start", "edge_start"):
            assert np.array_equal(getattr(got, name), getattr(want, name)), name
        assert got.num_features == want.num_features == 338
    rows = ds.records_to_data(records, basis, cuda)
    assert torch.equal(torch.cat([d.edge_attr for d in rows]), want.edge_attr.cpu())
    old = ds.records_to_data(records, full, cuda)
    assert all(torch.equal(a.edge_attr, b.edge_attr) and torch.equal(a.edge_index, b.edge_index)
               for a, b in zip(rows, old))
