"""The fp64 statement of the AO edge features (tests/ao_features_ref.py) against what the reference's own
``bi_gen_edge_feature_6`` recorded (tests/golden/ao_features.npz, made by tests/golden/make_ao_golden.py), the
host-side container and checks of x2gnn.features, and the binding table of include/x2g_features.h.  No GPU.

Bound of the statement against the reference (nothing taken from either side's result): both round the same float64
elements to float32, so the exactly-zero cells are the same set and the single x single cells are bitwise equal.  A norm
cell is made by the reference in two float32 stages, first over the column group and then over the row group, of at
most 7 terms each: a float32 sum of n squares and its root are within (n/2 + 1.5) * 2^-24 relative, which is
(7/2 + 1.5) * 2^-24 = 5 * 2^-24 per stage and 10 * 2^-24 for both; the statement's own float64 arithmetic adds
nothing at that scale.  Measured on the fixture: 2.31 * 2^-24 at most (case a).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import ao_features_ref as ar
from conftest import ROOT, golden

REF_BOUND = 10 * 2.0 ** -24
CASES = ("a", "b", "c")
SINGLE = ar.single_mask()
OK, EINVAL, EUNSUPPORTED = 0, 1001, 1002


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


def _worst(stmt, ref):
    """Largest relative difference over the norm cells, in units of the bound."""
    d = np.abs(stmt - ref.astype(np.float64))[:, ~SINGLE]
    scale = np.abs(stmt[:, ~SINGLE])
    return float((d[scale > 0] / scale[scale > 0]).max() / REF_BOUND) if (scale > 0).any() else 0.0


@pytest.mark.parametrize("case", CASES)
def test_statement_matches_the_reference(fx, case):
    d = fx[case]
    stmt, ref = d["stmt"], d["out"]
    assert ref.dtype == np.float32 and ref.shape == (d["edge_index"].shape[1], 338) == stmt.shape
    assert np.array_equal(stmt == 0, ref == 0)
    assert np.array_equal(stmt[:, SINGLE].astype(np.float32).view(np.int32), ref[:, SINGLE].view(np.int32))
    w = _worst(stmt, ref)
    print(f"case {case}: worst norm cell {w * 10:.3g} * 2^-24")
    assert w <= 1.0


@pytest.mark.parametrize("case", CASES)
def test_division_is_the_generators(fx, case):
    """H / nelectron in the statement is the float64 division the generator made for the reference."""
    d = fx[case]
    assert np.array_equal(d["H"] / np.float64(d["nelectron"]), d["Hdiv"])
    again = ar.edge_features(d["S"], d["Hdiv"], d["aoslice"], d["edge_index"])
    assert np.array_equal(again.view(np.int64), d["stmt"].view(np.int64))


def test_the_quirk_is_in_the_fixture(fx):
    """Case a's edge 1 -> 0 is hydrogen -> heavy, a (9, 39) block: the reference has it at rows 0..8, so row group 0
    is not zero, which it would be with the block at rows 2..10."""
    d = fx["a"]
    e = int(np.flatnonzero((d["edge_index"][0] == 1) & (d["edge_index"][1] == 0))[0])
    f = d["out"][e, :169].reshape(13, 13)
    assert (f[0] != 0).all() and (f[9:] == 0).all()  # rows 0..8 filled, 17..38 empty
    repaired = ar.edge_features(d["S"], d["H"], d["aoslice"], d["edge_index"], d["nelectron"], "quirk_repaired")
    assert (repaired[e, :169].reshape(13, 13)[0] == 0).all()


@pytest.mark.parametrize("variant", ar.WRONG)
def test_statement_tells_wrong_kernels_apart(fx, variant):
    """Each error a kernel could make misses the reference's rows of case a by far more than the bound."""
    d = fx["a"]
    wrong = ar.edge_features(d["S"], d["H"], d["aoslice"], d["edge_index"], d["nelectron"], variant)
    ref = d["out"].astype(np.float64)
    scale = np.maximum(np.abs(wrong), np.abs(ref))
    rel = (np.abs(wrong - ref)[scale > 0] / scale[scale > 0]).max()
    print(f"{variant}: misses by {rel:.3g} relative = {rel / REF_BOUND:.3g} bounds")
    assert rel > 1e4 * REF_BOUND


def test_oversized_block_raises():
    S = np.zeros((40, 40))
    with pytest.raises(ValueError):
        ar.edge_features(S, S, ar.aoslice_of([40]), np.array([[0], [0]]))


# ------------------------------------------------------------------------------------------------- AOMatrices
def _mols(fx, with_div=True):
    return [(fx[k]["S"], fx[k]["H"], fx[k]["aoslice"]) + ((fx[k]["nelectron"],) if with_div else ()) for k in CASES]


def test_from_molecules_layout(fx):
    from x2gnn.features import AOMatrices

    ao = AOMatrices.from_molecules(_mols(fx))
    assert len(ao) == 3 and ao.num_atoms == 11
    assert ao.mol_nao.tolist() == [105, 18, 62] and ao.mol_nao.dtype == torch.int32
    assert ao.mat_start.tolist() == [0, 105 * 105, 105 * 105 + 18 * 18] and ao.mat_start.dtype == torch.int64
    assert ao.atom_start.tolist() == [0, 5, 7, 11]
    assert ao.hcore_div.tolist() == [42.0, 2.0, 30.0] and ao.hcore_div.dtype == torch.float64
    assert ao.ao_begin.dtype == ao.ao_end.dtype == torch.int32
    assert (ao.ao_end - ao.ao_begin).tolist() == [39, 9, 9, 39, 9, 9, 9, 39, 13, 1, 9]
    assert ao.atom_mol().tolist() == [0] * 5 + [1] * 2 + [2] * 4 and ao.atom_mol().dtype == torch.int32
    s = int(ao.mat_start[2])
    assert np.array_equal(ao.ovlp[s:s + 62 * 62].numpy().reshape(62, 62), fx["c"]["S"])
    assert np.array_equal(ao.hcore[s:s + 62 * 62].numpy().reshape(62, 62), fx["c"]["H"])
    assert AOMatrices.from_molecules(_mols(fx, with_div=False)).hcore_div is None
    # torch inputs give the same container
    t = AOMatrices.from_molecules([(torch.from_numpy(S), torch.from_numpy(H), torch.from_numpy(sl), n)
                                   for S, H, sl, n in _mols(fx)])
    assert torch.equal(t.ovlp, ao.ovlp) and torch.equal(t.hcore, ao.hcore) and torch.equal(t.ao_end, ao.ao_end)
    part = ao.slice(1, 3)
    assert len(part) == 2 and part.mat_start.tolist() == [0, 18 * 18] and part.atom_start.tolist() == [0, 2, 6]
    assert torch.equal(part.ovlp, ao.ovlp[105 * 105:]) and part.hcore_div.tolist() == [2.0, 30.0]
    assert part.ao_begin.tolist() == ao.ao_begin[5:].tolist()


@pytest.mark.parametrize("with_div", [True, False])
def test_save_load_round_trip_is_bitwise(fx, tmp_path, with_div):
    from x2gnn.features import AOMatrices

    ao = AOMatrices.from_molecules(_mols(fx, with_div))
    path = os.path.join(tmp_path, "ao.npz")
    ao.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert all(z[k].dtype != object for k in z.files)
    back = AOMatrices.load(path)
    for k in ("ovlp", "hcore", "mat_start", "mol_nao", "hcore_div", "ao_begin", "ao_end", "atom_start"):
        a, b = getattr(ao, k), getattr(back, k)
        if a is None:
            assert b is None and not with_div
            continue
        assert a.dtype == b.dtype and a.shape == b.shape
        assert a.numpy().tobytes() == b.numpy().tobytes(), k


def _sl(*ranges):
    return np.array([[0, 0, b, e] for b, e in ranges], np.int64)


@pytest.mark.parametrize("mol,exc,words", [
    ((np.zeros((4, 5)), np.zeros((4, 5)), _sl((0, 4))), ValueError, ("molecule 1", "square")),
    ((np.zeros((4, 4)), np.zeros((5, 5)), _sl((0, 4))), ValueError, ("molecule 1", "shape")),
    ((np.zeros((4, 4), np.float32), np.zeros((4, 4)), _sl((0, 4))), TypeError, ("molecule 1", "float64")),
    ((np.zeros((4, 4)), np.zeros((4, 4), np.float32), _sl((0, 4))), TypeError, ("molecule 1", "float64")),
    ((torch.zeros(4, 4), torch.zeros(4, 4), _sl((0, 4))), TypeError, ("molecule 1", "float64")),
    ((np.zeros((4, 4), np.int64), np.zeros((4, 4)), _sl((0, 4))), TypeError, ("molecule 1", "float64")),
    ((np.zeros((4, 4)), np.zeros((4, 4)), _sl((0, 2), (2, 5))), ValueError, ("molecule 1", "atom 1", "outside")),
    ((np.zeros((4, 4)), np.zeros((4, 4)), _sl((0, 2), (-1, 2))), ValueError, ("molecule 1", "atom 1")),
    ((np.zeros((4, 4)), np.zeros((4, 4)), _sl((0, 2), (2, 4), (3, 3))), ValueError, ("molecule 1", "atom 2", "empty")),
    ((np.zeros((4, 4)), np.zeros((4, 4)), _sl((3, 1))), ValueError, ("molecule 1", "atom 0", "reversed")),
    ((np.zeros((50, 50)), np.zeros((50, 50)), _sl((0, 10), (10, 50))), ValueError, ("molecule 1", "atom 1", "39")),
    ((np.zeros((4, 4)), np.zeros((4, 4)), np.zeros((2, 3), np.int64)), ValueError, ("molecule 1", "aoslice")),
])
def test_from_molecules_validation(mol, exc, words):
    from x2gnn.features import AOMatrices

    good = (np.eye(9), np.eye(9), _sl((0, 9)))
    with pytest.raises(exc) as info:
        AOMatrices.from_molecules([good, mol])
    assert all(w in str(info.value) for w in words), str(info.value)


def test_nelectron_for_all_or_none():
    from x2gnn.features import AOMatrices

    good = (np.eye(9), np.eye(9), _sl((0, 9)))
    with pytest.raises(ValueError):
        AOMatrices.from_molecules([good + (2,), good])
    assert len(AOMatrices.from_molecules([good, good])) == 2
    assert len(AOMatrices.from_molecules([])) == 0


def test_cpu_tensors_raise(fx):
    """There is no CPU implementation: the batched call and the reference-signature call refuse CPU-only work."""
    from x2gnn.features import AOMatrices, ao_edge_features

    ao = AOMatrices.from_molecules(_mols(fx))
    with pytest.raises(RuntimeError, match="GPU"):
        ao_edge_features(ao, torch.from_numpy(fx["a"]["edge_index"]), ao.atom_mol())


def test_constants():
    from x2gnn import features, synth

    assert features.AO_PAD == 39 == ar.PAD
    assert [tuple(g) for g in features.AO_GROUPS] == ar.GROUPS
    assert features.EDGE_FEATURES == synth.EDGE_FEATURES == 2 * 13 * 13 == ar.ROW
    covered = [i for lo, hi in features.AO_GROUPS for i in range(lo, hi)]
    assert covered == list(range(39))


# ------------------------------------------------------------------------------------------------- the binding
def test_binding_table():
    from x2gnn import _lib

    names = {"x2g_ao_edge_features"}
    assert set(_lib.FEATURES_SIGNATURES) == names == set(_lib.FEATURES_RESTYPES)
    for table in (_lib.SIGNATURES, _lib.STAGED_SIGNATURES, _lib.MULTI_SIGNATURES, _lib.CONV_SIGNATURES,
                  _lib.ATOMCTX_SIGNATURES, _lib.TRAIN_SIGNATURES):
        assert not names & set(table)
    P, I = ctypes.c_void_p, ctypes.c_int64
    assert _lib.FEATURES_SIGNATURES["x2g_ao_edge_features"] == [P] * 9 + [I] * 3 + [P, P]
    assert _lib.FEATURES_RESTYPES["x2g_ao_edge_features"] is ctypes.c_int
    lib = _lib.load()
    assert lib.x2g_ao_edge_features.argtypes == _lib.FEATURES_SIGNATURES["x2g_ao_edge_features"]


def test_the_header_declares_functions_only_and_leaves_the_abi_alone():
    from x2gnn import _lib

    with open(os.path.join(ROOT, "include", "x2g_features.h")) as f:
        sig, res, structs, consts = _lib.parse_header(f.read())
    assert not structs and not consts and list(sig) == ["x2g_ao_edge_features"]
    with open(os.path.join(ROOT, "include", "x2g.h")) as f:
        own = _lib.parse_header(f.read())[0]
    assert _lib.SIGNATURES == own and "x2g_ao_edge_features" not in own
    assert _lib.load().x2g_abi_version() == 18


def test_exports():
    import x2gnn
    from x2gnn import datasets, features

    for name in ("AOMatrices", "ao_edge_features", "bi_gen_edge_feature_6"):
        assert name in x2gnn.__all__ and getattr(x2gnn, name) is getattr(features, name)
    assert callable(datasets.records_to_data)


A = 0x10000  # never dereferenced: every case below is refused, or returns, before a launch
E_MAX = (1 << 31) // (338 * 4)  # the largest E whose last byte offset is below 2^31


def _args(**kw):
    a = dict(ovlp=A, hcore=A, mat_start=A, mol_nao=A, hcore_div=None, ao_begin=A, ao_end=A, atom_mol=A, edge_index=A,
             M=1, N=2, E=0, out=A)
    a.update(kw)
    p = {k: None if a[k] is None else ctypes.c_void_p(a[k]) for k in a if k not in "MNE"}
    return tuple(p[k] for k in ("ovlp", "hcore", "mat_start", "mol_nao", "hcore_div", "ao_begin", "ao_end", "atom_mol",
                                "edge_index")) + (a["M"], a["N"], a["E"], p["out"], None)


@pytest.mark.parametrize("kw,want", [
    (dict(), OK), (dict(hcore_div=A), OK), (dict(M=0, N=0), OK),
    (dict(ovlp=None), EINVAL), (dict(hcore=None), EINVAL), (dict(mat_start=None), EINVAL),
    (dict(mol_nao=None), EINVAL), (dict(ao_begin=None), EINVAL), (dict(ao_end=None), EINVAL),
    (dict(atom_mol=None), EINVAL), (dict(edge_index=None), EINVAL), (dict(out=None), EINVAL),
    (dict(M=-1), EINVAL), (dict(N=-1), EINVAL), (dict(E=-1), EINVAL),
    (dict(E=E_MAX + 1), EUNSUPPORTED), (dict(E=1 << 40), EUNSUPPORTED),
    (dict(E=E_MAX + 1, ovlp=None), EINVAL),
])
def test_argument_validation_without_gpu(kw, want):
    from x2gnn import _lib

    assert E_MAX * 338 * 4 < 1 << 31 <= (E_MAX + 1) * 338 * 4
    assert _lib.load().x2g_ao_edge_features(*_args(**kw)) == want


# ------------------------------------------------------------------------------------------------- the dataset path
def test_records_to_data_checks_before_any_device_work():
    """The atom-count check of qm9_allprop.py:15 and the molecule count are host checks: they raise without a GPU."""
    from x2gnn import datasets as ds
    from x2gnn.features import AOMatrices

    R = torch.tensor([[0.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0]])
    rec = ds.MolRecord(atom="", R=R, Z=torch.tensor([8, 1, 1]), N=torch.tensor([3]), Label=torch.tensor([0.5]),
                       idx=torch.tensor([7]))
    short = AOMatrices.from_molecules([(np.eye(48), np.eye(48), ar.aoslice_of([39, 9]))])
    with pytest.raises(ValueError, match="record 0"):
        ds.records_to_data([rec], short, "cuda")
    with pytest.raises(ValueError, match="2 records"):
        ds.records_to_data([rec, rec], short, "cuda")
