"""The AO edge-feature kernel (csrc/ao_features.hip, include/x2g_features.h) through the raw ABI and through
x2gnn.features / x2gnn.datasets, against the fp64 statement of the operation (tests/ao_features_ref.py) and against the
rows the reference itself recorded (tests/golden/ao_features.npz).

Bounds (nothing taken from the code under test).  Against the statement: a cell that is exactly zero there is exactly
zero; a single x single cell is the float32 element, bitwise; a norm cell is the statement's float64 value (float64
sum of the squares of the float32 elements in the same order, float64 root) rounded once to float32, so
|err| <= 2^-23 |f| (one float32 ulp, which also covers a root that is not correctly rounded).  Against the reference's
recorded rows: that plus the 10 * 2^-24 of its two float32 norm stages (tests/test_ao_features_ref.py).

Every call writes into the middle of a buffer filled with a sentinel: the row before and the row after the [E, 338]
range have to stay untouched, bit for bit.
"""
import ctypes

import numpy as np
import pytest
import torch

import ao_features_ref as ar
from conftest import golden

pytestmark = pytest.mark.gpu

OK, EINVAL, EUNSUPPORTED = 0, 1001, 1002
ULP = 2.0 ** -23
REF_BOUND = 10 * 2.0 ** -24
SINGLE = ar.single_mask()
SENTINEL = 0x5A5A5A5A  # int32 bits of every canary float
CASES = ("a", "b", "c")


def _dev(a, cuda):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Flat:
    """The ABI's arrays on the device, from numpy (built by hand where AOMatrices would refuse the input)."""

    def __init__(self, cuda, ovlp, hcore, mat_start, mol_nao, ao_begin, ao_end, atom_mol, hcore_div=None):
        self.cuda = cuda
        self.M, self.N = len(mol_nao), len(atom_mol)
        self.ovlp, self.hcore = _dev(np.asarray(ovlp, np.float64), cuda), _dev(np.asarray(hcore, np.float64), cuda)
        self.mat_start = _dev(np.asarray(mat_start, np.int64), cuda)
        self.mol_nao = _dev(np.asarray(mol_nao, np.int32), cuda)
        self.ao_begin, self.ao_end = (_dev(np.asarray(a, np.int32), cuda) for a in (ao_begin, ao_end))
        self.atom_mol = _dev(np.asarray(atom_mol, np.int32), cuda)
        self.hcore_div = None if hcore_div is None else _dev(np.asarray(hcore_div, np.float64), cuda)

    @classmethod
    def of(cls, cuda, mols, divide_in_kernel=False):
        """``mols``: fixture-style dicts.  H is given pre-divided unless ``divide_in_kernel``."""
        from x2gnn.features import AOMatrices

        ao = AOMatrices.from_molecules([(m["S"], m["H"] if divide_in_kernel else m["Hdiv"], m["aoslice"]) +
                                        ((m["nelectron"],) if divide_in_kernel else ()) for m in mols])
        return cls(cuda, ao.ovlp.numpy(), ao.hcore.numpy(), ao.mat_start.numpy(), ao.mol_nao.numpy(),
                   ao.ao_begin.numpy(), ao.ao_end.numpy(), ao.atom_mol().numpy(),
                   ao.hcore_div.numpy() if divide_in_kernel else None)

    def run(self, edges, want=OK, E=None, **override):
        """(rows [E, 338] float32 on the host, canaries untouched) of one raw call."""
        from x2gnn import _lib

        ei = np.ascontiguousarray(np.asarray(edges, np.int64).reshape(2, -1))
        E_true = ei.shape[1]
        E = E_true if E is None else E
        buf = torch.full((E_true + 2, ar.ROW), SENTINEL, device=self.cuda, dtype=torch.int32).view(torch.float32)
        ei_d = _dev(ei if E_true else np.zeros((2, 1), np.int64), self.cuda)  # (an empty tensor has no address)
        a = dict(ovlp=self.ovlp, hcore=self.hcore, mat_start=self.mat_start, mol_nao=self.mol_nao,
                 hcore_div=self.hcore_div, ao_begin=self.ao_begin, ao_end=self.ao_end, atom_mol=self.atom_mol,
                 edge_index=ei_d, out=buf[1:], M=self.M, N=self.N)
        a.update(override)
        rc = _lib.load().x2g_ao_edge_features(
            _p(a["ovlp"]), _p(a["hcore"]), _p(a["mat_start"]), _p(a["mol_nao"]), _p(a["hcore_div"]), _p(a["ao_begin"]),
            _p(a["ao_end"]), _p(a["atom_mol"]), _p(a["edge_index"]), a["M"], a["N"], E, _p(a["out"]),
            _lib.stream_ptr())
        torch.cuda.synchronize()  # (the inputs live until the kernel has read them)
        assert rc == want, f"status {rc}, expected {want}"
        bits = _bits(buf)
        canaries = bool((bits[0] == SENTINEL).all()) and bool((bits[E_true + 1] == SENTINEL).all())
        assert canaries, "a canary row was written"
        return buf[1:E_true + 1].cpu().numpy(), bits[1:E_true + 1].numpy()


def check_against_statement(got, stmt, what):
    """The three properties of the module docstring; prints the worst norm cell before asserting."""
    assert got.dtype == np.float32 and got.shape == stmt.shape, what
    g = got.astype(np.float64)
    assert np.isfinite(g).all(), what
    zero = stmt == 0
    assert (g[zero] == 0).all(), f"{what}: a cell that is zero in the statement is not"
    assert np.array_equal(got[:, SINGLE].view(np.int32), stmt[:, SINGLE].astype(np.float32).view(np.int32)), \
        f"{what}: single x single cells are not bitwise the float32 elements"
    norm = ~zero & ~SINGLE[None, :]
    worst = float((np.abs(g - stmt)[norm] / np.abs(stmt[norm])).max() / ULP) if norm.any() else 0.0
    print(f"{what}: worst norm cell {worst:.3g} ulp (bound 1)")
    assert worst <= 1.0, what


def check_against_reference(got, ref, what):
    g, r = got.astype(np.float64), ref.astype(np.float64)
    assert np.array_equal(g == 0, r == 0), what
    assert np.array_equal(got[:, SINGLE].view(np.int32), ref[:, SINGLE].view(np.int32)), what
    nz = r != 0
    worst = float((np.abs(g - r)[nz] / np.abs(r[nz])).max() / (ULP + REF_BOUND))
    print(f"{what}: worst cell against the reference {worst:.3g} of the bound")
    assert worst <= 1.0, what


@pytest.fixture(scope="module")
def fx():
    z = golden("ao_features.npz")
    out = {}
    for k in CASES:
        d = {n: z[f"{k}.{n}"] for n in ("S", "H", "Hdiv", "aoslice", "edge_index", "out")}
        d["nelectron"] = int(z[f"{k}.nelectron"])
        d["stmt"] = ar.edge_features(d["S"], d["H"], d["aoslice"], d["edge_index"], d["nelectron"])
        out[k] = d
    return out


@pytest.fixture(scope="module")
def alone(fx, cuda):
    """Each fixture molecule in a launch of its own: (rows, bits)."""
    return {k: Flat.of(cuda, [fx[k]]).run(fx[k]["edge_index"]) for k in CASES}


def _interleaved(fx):
    """The three molecules' edges with batch-global atom indices, dealt round-robin: (edge_index, case, local edge)."""
    offs, at = {}, 0
    for k in CASES:
        offs[k] = at
        at += len(fx[k]["aoslice"])
    todo = {k: list(range(fx[k]["edge_index"].shape[1])) for k in CASES}
    cols, owner = [], []
    while any(todo.values()):
        for k in CASES:
            if todo[k]:
                e = todo[k].pop(0)
                cols.append(fx[k]["edge_index"][:, e] + offs[k])
                owner.append((k, e))
    return np.stack(cols, axis=1), owner


@pytest.mark.parametrize("case", CASES)
def test_fixture_molecule_alone(fx, alone, case):
    rows, _ = alone[case]
    check_against_statement(rows, fx[case]["stmt"], f"case {case}")
    check_against_reference(rows, fx[case]["out"], f"case {case}")


def test_batched_rows_equal_the_stand_alone_rows_and_two_runs_agree(fx, alone, cuda):
    flat = Flat.of(cuda, [fx[k] for k in CASES])
    ei, owner = _interleaved(fx)
    rows, bits = flat.run(ei)
    _, again = flat.run(ei)
    assert np.array_equal(bits, again), "two runs differ"
    for row, (k, e) in enumerate(owner):
        assert np.array_equal(bits[row], alone[k][1][e]), f"batched row {row} differs from case {k} edge {e} alone"
    stmt = np.stack([fx[k]["stmt"][e] for k, e in owner])
    check_against_statement(rows, stmt, "batched")
    check_against_reference(rows, np.stack([fx[k]["out"][e] for k, e in owner]), "batched")


def test_division_in_the_kernel_equals_the_pre_divided_matrix(fx, cuda):
    ei, _ = _interleaved(fx)
    _, pre = Flat.of(cuda, [fx[k] for k in CASES]).run(ei)
    _, div = Flat.of(cuda, [fx[k] for k in CASES], divide_in_kernel=True).run(ei)
    assert np.array_equal(pre, div)


@pytest.fixture(scope="module")
def sweep():
    """One molecule with atoms of 1, 9, 13 and 39 functions and every ordered pair of them as an edge, self-loops
    (the diagonal blocks) included: all 16 block shapes.  Magnitudes from 1e-30 to 1e3."""
    counts = [1, 9, 13, 39]
    rng = np.random.default_rng(611)
    nao = sum(counts)
    d = dict(S=ar.random_symmetric(rng, nao, -30.0, 3.0), H=ar.random_symmetric(rng, nao, -30.0, 3.0),
             aoslice=ar.aoslice_of(counts), edge_index=ar.all_directed_edges(4, self_loops=True), nelectron=14)
    d["Hdiv"] = d["H"] / np.float64(d["nelectron"])
    d["stmt"] = ar.edge_features(d["S"], d["H"], d["aoslice"], d["edge_index"], d["nelectron"])
    return d


def test_every_block_shape_and_tiny_values(sweep, cuda):
    width = (sweep["aoslice"][:, 3] - sweep["aoslice"][:, 2]).tolist()
    shapes = {(width[i], width[j]) for i, j in sweep["edge_index"].T}
    assert shapes == {(r, c) for r in (1, 9, 13, 39) for c in (1, 9, 13, 39)}
    rows, bits = Flat.of(cuda, [sweep]).run(sweep["edge_index"])
    check_against_statement(rows, sweep["stmt"], "sweep")
    # norm cells whose squares are below float32's smallest normal: a float32 sum would have lost them
    stmt = sweep["stmt"]
    tiny = (stmt > 0) & (stmt * stmt < 2.0 ** -126) & ~SINGLE[None, :]
    assert tiny.sum() > 10
    assert (rows[tiny] > 0).all()
    _, div = Flat.of(cuda, [sweep], divide_in_kernel=True).run(sweep["edge_index"])
    assert np.array_equal(bits, div)


def test_one_edge_and_no_edge(fx, alone, cuda):
    flat = Flat.of(cuda, [fx["a"]])
    for e in (0, 7, 19):  # the first block's first wave pair, an odd edge, the last
        _, bits = flat.run(fx["a"]["edge_index"][:, e:e + 1])
        assert np.array_equal(bits[0], alone["a"][1][e])
    # E == 0: X2G_OK and nothing written (run() checks the two canary rows, which are the whole buffer then)
    rows, _ = flat.run(np.zeros((2, 0), np.int64))
    assert rows.shape == (0, ar.ROW)
    # ... also when the pointers would have allowed a write
    _, bits = flat.run(fx["a"]["edge_index"][:, :3], E=0)
    assert (bits == SENTINEL).all()


@pytest.mark.parametrize("override", [
    dict(ovlp=None), dict(hcore=None), dict(mat_start=None), dict(mol_nao=None), dict(ao_begin=None),
    dict(ao_end=None), dict(atom_mol=None), dict(edge_index=None), dict(out=None), dict(M=-1), dict(N=-1),
])
def test_refused_calls_write_nothing(fx, cuda, override):
    _, bits = Flat.of(cuda, [fx["b"]]).run(fx["b"]["edge_index"], want=EINVAL, **override)
    assert (bits == SENTINEL).all()


def test_refused_counts_write_nothing(fx, cuda):
    flat = Flat.of(cuda, [fx["b"]])
    for E, want in ((-1, EINVAL), ((1 << 31) // (338 * 4) + 1, EUNSUPPORTED)):
        _, bits = flat.run(fx["b"]["edge_index"], want=want, E=E)
        assert (bits == SENTINEL).all()


def test_invalid_edges_get_nan_rows_and_leave_the_rest_alone(cuda):
    """Two molecules: m0 of two hydrogen-like atoms (18 functions), m1 of 58 functions whose atom table holds one good
    atom and every kind of bad one.  The kernel may read an edge's atom indices, then atom_mol / ao_begin / ao_end of
    an index inside [0, N), then mol_nao / mat_start of a molecule inside [0, M), and the matrices only through a
    range it has found inside them: nothing below sends it anywhere else."""
    rng = np.random.default_rng(77)
    S0, H0, S1, H1 = (ar.random_symmetric(rng, n) for n in (18, 18, 58, 58))
    #            atom: 0  1   2   3   4   5  6   7   8
    ao_begin = [0, 9, 0, 40, 49, 5, 9, -3, 0]
    ao_end = [9, 18, 40, 49, 60, 5, 3, 4, 9]  # 2: 40 functions, 4: beyond nao, 5: empty, 6: reversed, 7: begins below 0
    atom_mol = [0, 0, 1, 1, 1, 1, 1, 1, 7]  # 8: a molecule that does not exist
    flat = Flat(cuda, np.concatenate([S0.ravel(), S1.ravel()]), np.concatenate([H0.ravel(), H1.ravel()]),
                [0, 18 * 18], [18, 58], ao_begin, ao_end, atom_mol)
    N = len(atom_mol)
    valid = [(0, 1), (1, 0), (3, 3), (1, 1)]
    invalid = [(0, 3), (3, 1),          # the two atoms are in different molecules
               (2, 3), (3, 2),          # an atom with 40 functions
               (4, 3), (3, 4),          # an ao_end beyond nao
               (N, 0), (0, N), (-1, 0), (0, 1 << 40),  # an atom index outside [0, N)
               (5, 3), (6, 3), (7, 3),  # empty, reversed, negative begin
               (8, 8)]                  # a molecule index outside [0, M)
    order = [("v", 0), ("i", 0), ("i", 1), ("v", 1), ("i", 2), ("i", 3), ("i", 4), ("v", 2), ("i", 5), ("i", 6),
             ("i", 7), ("i", 8), ("i", 9), ("v", 3), ("i", 10), ("i", 11), ("i", 12), ("i", 13)]
    ei = np.array([(valid if kind == "v" else invalid)[k] for kind, k in order], np.int64).T
    rows, bits = flat.run(ei)
    alone_rows, alone_bits = flat.run(np.array(valid, np.int64).T)
    for row, (kind, k) in enumerate(order):
        if kind == "v":
            assert np.array_equal(bits[row], alone_bits[k]), f"valid edge {valid[k]} changed beside invalid ones"
        else:
            assert np.isnan(rows[row]).all(), f"invalid edge {invalid[k]}: row is not all NaN"
    # and the valid rows are right: (0, 1), (1, 0), (1, 1) in m0; (3, 3) in m1
    sl0, sl1 = ar.aoslice_of([9, 9]), np.array([[0, 0, 0, 40], [0, 0, 40, 49]])
    stmt = np.concatenate([ar.edge_features(S0, H0, sl0, np.array([[0, 1], [1, 0]])),
                           ar.edge_features(S1, H1, sl1, np.array([[1], [1]])),
                           ar.edge_features(S0, H0, sl0, np.array([[1], [1]]))])
    check_against_statement(alone_rows, stmt, "valid edges")


def test_reference_signature(fx, alone, cuda):
    """torch float64 matrices, numpy aoslice, torch edge_index, as the reference's ``mapping`` passes them."""
    import x2gnn

    d = fx["a"]
    out = x2gnn.bi_gen_edge_feature_6(torch.from_numpy(d["S"]), torch.from_numpy(d["Hdiv"]), d["aoslice"],
                                      torch.from_numpy(d["edge_index"]), torch.tensor([8, 1, 1, 6, 1]))
    assert out.dtype == torch.float32 and out.device.type == "cpu" and tuple(out.shape) == (20, 338)
    assert np.array_equal(_bits(out).numpy(), alone["a"][1])
    check_against_reference(out.numpy(), d["out"], "bi_gen_edge_feature_6")
    on_dev = x2gnn.bi_gen_edge_feature_6(torch.from_numpy(d["S"]).to(cuda), torch.from_numpy(d["Hdiv"]).to(cuda),
                                         d["aoslice"], torch.from_numpy(d["edge_index"]).to(cuda))
    assert on_dev.is_cuda and np.array_equal(_bits(on_dev).numpy(), alone["a"][1])


# ------------------------------------------------------------------------------------------------- end to end
def _records_and_matrices():
    """Three molecules of 3, 4 and 5 atoms, all inside the cutoff, with seeded matrices of matching AO counts."""
    from x2gnn import datasets as ds
    from x2gnn.features import AOMatrices

    rng = np.random.default_rng(2024)
    zs = ([8, 1, 1], [6, 1, 1, 1], [6, 8, 1, 1, 1])
    recs, mols, parts = [], [], []
    for k, z in enumerate(zs):
        R = torch.from_numpy(rng.uniform(-1.2, 1.2, size=(len(z), 3)).astype(np.float32))
        recs.append(ds.MolRecord(atom="", R=R, Z=torch.tensor(z), N=torch.tensor([len(z)]),
                                 Label=torch.tensor([float(k) - 0.5]), idx=torch.tensor([k])))
        counts = [9 if a == 1 else 39 for a in z]
        nao = sum(counts)
        S, H = ar.random_symmetric(rng, nao, -4.0, 0.0), ar.random_symmetric(rng, nao, -4.0, 0.0)
        parts.append((S, H, ar.aoslice_of(counts), sum(z)))
        mols.append(dict(S=S, H=H, aoslice=parts[-1][2], nelectron=sum(z)))
    return recs, AOMatrices.from_molecules(parts), mols


def test_records_to_device_dataset_to_model(cuda):
    import x2gnn
    from x2gnn import datasets as ds
    from x2gnn.data import Batch

    recs, ao, mols = _records_and_matrices()
    datas = ds.records_to_data(recs, ao, cuda)
    assert [int(d.edge_index.shape[1]) for d in datas] == [6, 12, 20]
    per_mol = []
    for d, m in zip(datas, mols):
        assert d.edge_attr.dtype == torch.float32 and d.edge_attr.device.type == "cpu"
        assert tuple(d.edge_attr.shape) == (d.edge_index.shape[1], 338) and d._meta is not None
        ei = d.edge_index.numpy()
        rows, bits = Flat.of(cuda, [m], divide_in_kernel=True).run(ei)
        assert np.array_equal(_bits(d.edge_attr).numpy(), bits)
        check_against_statement(rows, ar.edge_features(m["S"], m["H"], m["aoslice"], ei, m["nelectron"]), "record")
        per_mol.append(torch.from_numpy(rows))
    # one molecule per launch gives the same rows
    for d, one in zip(datas, ds.records_to_data(recs, ao, cuda, max_edges_per_launch=1)):
        assert torch.equal(_bits(d.edge_attr), _bits(one.edge_attr))
    want = torch.cat(per_mol)
    assert torch.equal(_bits(Batch.from_data_list(datas).edge_attr), _bits(want))
    batch = x2gnn.DeviceDataset(datas, cuda).batch([0, 1, 2])
    assert torch.equal(_bits(batch.edge_attr), _bits(want))
    torch.manual_seed(0)
    model = x2gnn.xgnn_poly(device="cuda", conv_layers=2, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16,
                            embedding_size=128).to(cuda).eval()
    with torch.no_grad():
        energies = model(batch)
    assert tuple(energies.shape) == (3,) and bool(torch.isfinite(energies).all())


def test_a_record_with_an_atom_too_few_raises(cuda):
    from x2gnn import datasets as ds
    from x2gnn.features import AOMatrices

    recs, ao, mols = _records_and_matrices()
    parts = [(m["S"], m["H"], m["aoslice"], m["nelectron"]) for m in mols]
    S, H, sl, n = parts[1]
    parts[1] = (S[:-9, :-9].copy(), H[:-9, :-9].copy(), sl[:-1], n)  # the last hydrogen left out
    with pytest.raises(ValueError, match="record 1"):
        ds.records_to_data(recs, AOMatrices.from_molecules(parts), cuda)
