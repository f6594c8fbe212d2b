"""The fp64 statement of the radius graph and its band (tests/radius_graph_ref.py) against the host's float32 form
(``datasets.bonds(datasets.distance_matrix(R))``, the reference's ``calculate_Dij`` + ``gen_bonds_mini``), the exact
lattice fixture, the binding table of include/x2g_graph.h, the status codes returned before any launch, the exports and
the host checks of ``DeviceDataset.from_records``.  No GPU.

Nothing here is taken from the kernel: the band is derived in radius_graph_ref's docstring, the caps on undecided
pairs are the table's, and the lattice's expected edges come from integer arithmetic.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import ao_features_ref as ar
import radius_graph_ref as rg
from conftest import ROOT

OK, EINVAL, EUNSUPPORTED, EWORKSPACE = 0, 1001, 1002, 1003
NAMES = ["x2g_radius_graph_count_workspace", "x2g_radius_graph_count", "x2g_radius_graph_fill"]


# ------------------------------------------------------------------------------------------------- statement and band
@pytest.mark.parametrize("name", list(rg.FIXTURES))
def test_host_form_equals_the_statement_on_decided_pairs(name):
    from x2gnn import datasets as ds

    make, cap = rg.FIXTURES[name]
    mols = make()

    def host(k):
        R = torch.from_numpy(mols[k])
        return rg.adjacency_from_edges(ds.bonds(ds.distance_matrix(R), rg.CUTOFF).numpy(), len(mols[k]))

    wrong, undecided, pairs, asym = rg.compare(mols, host)
    print(f"{name}: {len(mols)} molecules, {pairs} ordered pairs, {undecided} undecided "
          f"({undecided / pairs:.3g}, cap {cap:g}), {wrong} decided pairs wrong")
    assert wrong == 0
    assert undecided <= cap * pairs


def test_the_fixtures_are_what_the_table_says():
    aid = rg.aid_molecules()
    assert len(aid) == 451 and max(len(R) for R in aid) == 146 == len(aid[21])
    assert [len(R) for R in aid[:16]] == [len(R) for R in rg.aid_molecules(range(16))]
    assert min(len(R) for R in aid[:16]) >= 64  # rows of more than one 64-lane step
    s160 = rg.s160_molecules(4)
    from x2gnn.synth import synthetic_molecules

    for R, mol in zip(s160, synthetic_molecules(4, "S160", seed=0)):
        assert np.array_equal(R, mol["atom_pos"])
    assert [R.shape for R in rg.uniform_molecules()] == [(300, 3)] * 6
    plus = rg.aid_molecules([0], shift=100.0)[0]
    assert plus.dtype == np.float32 and np.abs(plus - aid[0] - 100).max() < 1e-4


def test_band_covers_the_float32_gram_form():
    """The float32 Gram form, evaluated here with numpy float32 scalars in the header's order, stays inside the band
    for every pair within 0.5 A of the cutoff (AID + 100 A: the largest coordinates of the table)."""
    f = np.float32
    worst = 0.0
    for R in rg.aid_molecules(range(4), shift=100.0):
        x, y, z = (R[:, k] for k in range(3))
        # (numpy has no float32 fma: the products are formed in float64, exact for 24-bit factors, and each sum
        # rounded once, which is what fmaf gives up to a double rounding far below the band)
        g = (z[:, None].astype(np.float64) * z[None, :] +
             (y[:, None].astype(np.float64) * y[None, :] + f(1) * (x[:, None] * x[None, :])).astype(f)).astype(f)
        gd = np.diag(g)
        d2 = (gd[:, None] + gd[None, :]).astype(f) - (f(2) * g)
        with np.errstate(invalid="ignore"):
            d32 = np.sqrt(d2.astype(f)).astype(np.float64)
        d64, b = rg.distances(R), rg.band(R)
        near = (np.abs(d64 - rg.CUTOFF) < 0.5) & ~np.eye(len(R), dtype=bool)
        worst = max(worst, float((np.abs(d32 - d64)[near] / b[near]).max()))
    print(f"float32 Gram form: worst |d32 - d64| = {worst:.3g} bands")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------- the lattice
def test_lattice_statement_is_the_integer_arithmetic():
    mols = rg.lattice_molecules()
    ei, start = rg.graph(mols)
    want = rg.lattice_expected()
    assert start.tolist() == [0, 6, 7, 7, 9, 12]
    assert np.array_equal(ei, want[0])
    pairs = set(zip(*ei[:, :int(want[2][0])].tolist()))
    assert (0, 1) not in pairs and (0, 2) not in pairs        # d^2 = 25: strict <
    assert (0, 3) in pairs and (3, 0) in pairs                # d^2 = 24
    assert (0, 4) not in pairs and (4, 0) not in pairs        # coincident
    assert want[2].tolist() == [int(want[2][0]), 0, 0, 0, 2] and want[5].tolist() == [5, -1, -1, -1, 1]
    assert not rg.decided(mols[0])[0, 1] and rg.decided(mols[0])[0, 3]
    # the host's float32 form is exact here too
    from x2gnn import datasets as ds

    host = [ds.bonds(ds.distance_matrix(torch.from_numpy(R)), rg.CUTOFF).numpy() if len(R) else np.zeros((2, 0), np.int64)
            for R in mols]
    assert np.array_equal(np.concatenate(host, axis=1), ei)


@pytest.mark.parametrize("variant", rg.WRONG)
def test_statement_tells_wrong_graphs_apart(variant):
    mols = rg.lattice_molecules()
    wrong = rg.graph(mols, variant=variant)[0]
    right = rg.lattice_expected()[0]
    assert wrong.shape != right.shape or not np.array_equal(wrong, right)


def test_non_finite_atoms_have_no_edge():
    R = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 1, 0]], np.float32)
    ei = rg.edges_of(rg.adjacency(R))
    assert sorted(set(ei.ravel().tolist())) == [0, 1, 4] and ei.shape[1] == 6


# ------------------------------------------------------------------------------------------------- the binding
def test_binding_table():
    from x2gnn import _lib

    assert list(_lib.GRAPH_SIGNATURES) == NAMES and set(_lib.GRAPH_RESTYPES) == set(NAMES)
    for table in (_lib.SIGNATURES, _lib.STAGED_SIGNATURES, _lib.MULTI_SIGNATURES, _lib.CONV_SIGNATURES,
                  _lib.ATOMCTX_SIGNATURES, _lib.TRAIN_SIGNATURES, _lib.FEATURES_SIGNATURES):
        assert not set(NAMES) & set(table)
    P, I, F, S = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
    assert _lib.GRAPH_SIGNATURES["x2g_radius_graph_count_workspace"] == [I]
    assert _lib.GRAPH_SIGNATURES["x2g_radius_graph_count"] == [P, P, I, I, F] + [P] * 7 + [S, P]
    assert _lib.GRAPH_SIGNATURES["x2g_radius_graph_fill"] == [P, P, P, I, I, F, I, P, P, P]
    assert _lib.GRAPH_RESTYPES["x2g_radius_graph_count_workspace"] is ctypes.c_size_t
    assert _lib.GRAPH_RESTYPES["x2g_radius_graph_count"] is _lib.GRAPH_RESTYPES["x2g_radius_graph_fill"] is ctypes.c_int
    lib = _lib.load()
    for name in NAMES:
        assert getattr(lib, name).argtypes == _lib.GRAPH_SIGNATURES[name]


def test_the_header_declares_functions_only_and_leaves_the_abi_alone():
    from x2gnn import _lib

    with open(os.path.join(ROOT, "include", "x2g_graph.h")) as f:
        sig, res, structs, consts = _lib.parse_header(f.read())
    assert not structs and not consts and list(sig) == NAMES
    with open(os.path.join(ROOT, "include", "x2g.h")) as f:
        own = _lib.parse_header(f.read())[0]
    assert _lib.SIGNATURES == own and not set(NAMES) & set(own)
    assert _lib.load().x2g_abi_version() == 18


def test_exports():
    import x2gnn
    from x2gnn import graph

    assert "radius_graph" in x2gnn.__all__ and x2gnn.radius_graph is graph.radius_graph
    assert callable(x2gnn.DeviceDataset.from_records)


A = 0x10000  # never dereferenced: every case below is refused, or returns, before a launch
BIG = 1 << 31
COUNT_KEYS = ("pos", "atom_start", "degree", "row_start", "mol_edges", "mol_triplets", "mol_max_degree",
              "mol_last_bonded", "workspace")


def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def _count(**kw):
    a = dict({k: A for k in COUNT_KEYS}, N=0, M=0, ws_bytes=1 << 20)
    a.update(kw)
    return (_p(a["pos"]), _p(a["atom_start"]), a["N"], a["M"], 5.0, _p(a["degree"]), _p(a["row_start"]),
            _p(a["mol_edges"]), _p(a["mol_triplets"]), _p(a["mol_max_degree"]), _p(a["mol_last_bonded"]),
            _p(a["workspace"]), a["ws_bytes"], None)


@pytest.mark.parametrize("kw,want", [
    (dict(), OK), (dict(N=0, M=3), OK), (dict(N=3, M=0), OK),
    *[({k: None}, EINVAL) for k in COUNT_KEYS],
    (dict(N=-1), EINVAL), (dict(M=-1), EINVAL), (dict(N=-1, M=-1), EINVAL),
    (dict(N=BIG, M=1), EUNSUPPORTED), (dict(N=1 << 40, M=1), EUNSUPPORTED), (dict(N=BIG, M=0), EUNSUPPORTED),
    (dict(N=BIG, M=1, pos=None), EINVAL),
    (dict(N=100000, M=1, ws_bytes=8), EWORKSPACE),
])
def test_count_refuses_before_any_launch(kw, want):
    from x2gnn import _lib

    assert _lib.load().x2g_radius_graph_count(*_count(**kw)) == want


def _fill(**kw):
    a = dict(pos=A, atom_start=A, row_start=A, edge_local=A, edge_global=None, N=0, M=0, E=0)
    a.update(kw)
    return (_p(a["pos"]), _p(a["atom_start"]), _p(a["row_start"]), a["N"], a["M"], 5.0, a["E"], _p(a["edge_local"]),
            _p(a["edge_global"]), None)


@pytest.mark.parametrize("kw,want", [
    (dict(), OK), (dict(edge_global=A), OK), (dict(N=5, M=2, E=0), OK), (dict(N=0, M=2, E=4), OK),
    (dict(N=5, M=0, E=4), OK),
    (dict(pos=None), EINVAL), (dict(atom_start=None), EINVAL), (dict(row_start=None), EINVAL),
    (dict(edge_local=None), EINVAL), (dict(N=-1), EINVAL), (dict(M=-1), EINVAL), (dict(E=-1), EINVAL),
    (dict(N=BIG, M=1, E=1), EUNSUPPORTED), (dict(N=BIG, M=1, E=1, edge_local=None), EINVAL),
])
def test_fill_refuses_before_any_launch(kw, want):
    from x2gnn import _lib

    assert _lib.load().x2g_radius_graph_fill(*_fill(**kw)) == want


def test_workspace_query():
    from x2gnn import _lib

    q = _lib.load().x2g_radius_graph_count_workspace
    assert q(0) == 0 and q(-5) == 0 and q(BIG) == 0
    assert q(1) == 8 and q(2047) == 8 and q(2048) == 16  # N + 1 slots in tiles of 2048, one int64 each
    assert q(BIG - 1) == ((BIG + 2047) // 2048) * 8


# ------------------------------------------------------------------------------------------------- host-side checks
def test_radius_graph_refuses_cpu_tensors_and_bad_atom_starts():
    import x2gnn

    pos = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        x2gnn.radius_graph(pos, np.array([0, 4]))
    with pytest.raises(RuntimeError, match="GPU"):
        x2gnn.radius_graph(pos.numpy(), np.array([0, 4]))


@pytest.mark.parametrize("start", [[1, 4], [0, 3], [0, 5], [0, 3, 2, 4], [], [[0, 4]], [0.0, 4.0]])
def test_atom_start_validation(start):
    from x2gnn.graph import _atom_start

    with pytest.raises(ValueError, match="atom_start"):
        _atom_start(np.asarray(start), 4)
    assert _atom_start(torch.tensor([0, 2, 2, 4]), 4).tolist() == [0, 2, 2, 4]
    assert _atom_start(np.array([0, 4], np.int32), 4).dtype == np.int64


def _record_and_short_matrices():
    from x2gnn import datasets as ds
    from x2gnn.features import AOMatrices

    R = torch.tensor([[0.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0]])
    rec = ds.MolRecord(atom="", R=R, Z=torch.tensor([8, 1, 1]), N=torch.tensor([3]), Label=torch.tensor([0.5]),
                       idx=torch.tensor([7]))
    return rec, AOMatrices.from_molecules([(np.eye(48), np.eye(48), ar.aoslice_of([39, 9]))])


def test_from_records_host_checks_raise_without_a_gpu():
    import x2gnn

    rec, ao = _record_and_short_matrices()
    with pytest.raises(ValueError, match="2 records"):
        x2gnn.DeviceDataset.from_records([rec, rec], ao, "cuda")
    with pytest.raises(RuntimeError, match="GPU"):
        x2gnn.DeviceDataset.from_records([rec], ao, "cpu")


def test_ao_edge_features_out_is_an_argument():
    import inspect

    from x2gnn.features import ao_edge_features

    sig = inspect.signature(ao_edge_features)
    assert list(sig.parameters) == ["ao", "edge_index", "atom_mol", "out"] and sig.parameters["out"].default is None
