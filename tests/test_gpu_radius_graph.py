"""The radius-graph kernels (csrc/radius_graph.hip, include/x2g_graph.h) through the raw ABI and through
x2gnn.radius_graph, ``ao_edge_features(out=...)`` and ``DeviceDataset.from_records``, against the fp64 statement of the
operation and its band (tests/radius_graph_ref.py) and, for the dataset, against the path it replaces.

Bounds (nothing taken from the code under test).  On the lattice fixture every quantity is exact and is compared with
integer arithmetic.  On the other fixtures a pair further from the cutoff than the band (derived in radius_graph_ref)
has to be decided as in float64, the undecided pairs are capped by the table there, and the adjacency has to be
symmetric everywhere.  Everything else is an identity: order, counts, global ids, two runs, one launch against many.

Every raw call writes into the middle of buffers filled with a sentinel, and the words after each output's last
element have to stay untouched.
"""
import ctypes

import numpy as np
import pytest
import torch

import ao_features_ref as ar
import radius_graph_ref as rg

pytestmark = pytest.mark.gpu

OK, EINVAL, EUNSUPPORTED = 0, 1001, 1002
S32 = 0x5A5A5A5A
S64 = 0x5A5A5A5A5A5A5A5A
TAIL = 8  # sentinel words after every output


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Raw:
    """One count + fill through the C ABI with sentinel-filled outputs; everything read back as numpy."""

    def __init__(self, cuda, pos, start, cutoff=rg.CUTOFF):
        self.cuda, self.cutoff = cuda, cutoff
        self.N, self.M = len(pos), len(start) - 1
        self.pos = torch.from_numpy(np.ascontiguousarray(pos, np.float32).reshape(-1, 3)).to(cuda)
        self.start = torch.from_numpy(np.ascontiguousarray(start, np.int64)).to(cuda)
        if self.N == 0:
            self.pos = torch.zeros((1, 3), device=cuda)  # (an empty tensor has no address)

    def _i32(self, n):
        return torch.full((n + TAIL,), S32, dtype=torch.int32, device=self.cuda)

    def _i64(self, n):
        return torch.full((n + TAIL,), S64, dtype=torch.int64, device=self.cuda)

    def count(self, want=OK, **override):
        from x2gnn import _lib

        lib = _lib.load()
        N, M = self.N, self.M
        self.out = dict(degree=self._i32(N), row_start=self._i64(N + 1), mol_edges=self._i64(M),
                        mol_triplets=self._i64(M), mol_max_degree=self._i64(M), mol_last_bonded=self._i32(M))
        need = int(lib.x2g_radius_graph_count_workspace(N))
        ws = torch.full((need // 8 + TAIL,), S64, dtype=torch.int64, device=self.cuda)
        a = dict(pos=self.pos, atom_start=self.start, N=N, M=M, workspace=ws, ws_bytes=need, **self.out)
        a.update(override)
        rc = lib.x2g_radius_graph_count(
            _p(a["pos"]), _p(a["atom_start"]), a["N"], a["M"], self.cutoff, _p(a["degree"]), _p(a["row_start"]),
            _p(a["mol_edges"]), _p(a["mol_triplets"]), _p(a["mol_max_degree"]), _p(a["mol_last_bonded"]),
            _p(a["workspace"]), a["ws_bytes"], _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == want, f"status {rc}, expected {want}"
        assert bool((ws[need // 8:] == S64).all()), "the workspace was written beyond the queried size"
        host = {k: v.cpu().numpy() for k, v in self.out.items()}
        sizes = dict(degree=N, row_start=N + 1, mol_edges=M, mol_triplets=M, mol_max_degree=M, mol_last_bonded=M)
        for k, n in sizes.items():
            sentinel = S32 if host[k].dtype == np.int32 else S64
            assert (host[k][n:] == sentinel).all(), f"{k}: the tail was written"
            if want != OK:
                assert (host[k] == sentinel).all(), f"{k}: written by a refused call"
        return {k: host[k][:n] for k, n in sizes.items()}

    def fill(self, E, want=OK, with_global=True, rows=None, **override):
        """``rows``: how many edge slots the buffers really have (default E)."""
        from x2gnn import _lib

        rows = E if rows is None else rows
        local, glob = self._i64(2 * rows), self._i64(2 * rows)
        a = dict(pos=self.pos, atom_start=self.start, row_start=self.out["row_start"], N=self.N, M=self.M, E=E,
                 edge_local=local, edge_global=glob if with_global else None)
        a.update(override)
        rc = _lib.load().x2g_radius_graph_fill(
            _p(a["pos"]), _p(a["atom_start"]), _p(a["row_start"]), a["N"], a["M"], self.cutoff, a["E"],
            _p(a["edge_local"]), _p(a["edge_global"]), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == want, f"status {rc}, expected {want}"
        lh, gh = local.cpu().numpy(), glob.cpu().numpy()
        assert (lh[2 * rows:] == S64).all() and (gh[2 * rows:] == S64).all(), "an edge tail was written"
        if not with_global:
            assert (gh == S64).all()
        return lh[:2 * rows].reshape(2, rows), gh[:2 * rows].reshape(2, rows)


def _run(cuda, mols, cutoff=rg.CUTOFF):
    """x2gnn.radius_graph of a list of position arrays: (result, atom_start)."""
    import x2gnn

    pos, start = rg.flat(mols)
    return x2gnn.radius_graph(torch.from_numpy(pos).to(cuda), start, cutoff, global_ids=True), start


# ------------------------------------------------------------------------------------------------- the lattice
def test_lattice_through_the_raw_abi(cuda):
    pos, start = rg.flat(rg.lattice_molecules())
    ei, degree, edges, trips, top, last = rg.lattice_expected()
    raw = Raw(cuda, pos, start)
    got = raw.count()
    assert np.array_equal(got["degree"], degree)
    assert np.array_equal(got["row_start"], np.concatenate([[0], np.cumsum(degree)]))
    assert np.array_equal(got["mol_edges"], edges) and np.array_equal(got["mol_triplets"], trips)
    assert np.array_equal(got["mol_max_degree"], top) and np.array_equal(got["mol_last_bonded"], last)
    assert last.tolist() == [5, -1, -1, -1, 1] and edges[2] == 0  # the -1s and the empty molecule are in it
    E = int(got["row_start"][-1])
    local, glob = raw.fill(E)
    assert np.array_equal(local, ei)
    assert np.array_equal(glob, ei + np.repeat(start[:-1], edges)[None, :])
    only_local, _ = raw.fill(E, with_global=False)
    assert np.array_equal(only_local, ei)


def test_lattice_through_the_python_surface(cuda):
    g, start = _run(cuda, rg.lattice_molecules())
    ei, degree, edges, trips, top, last = rg.lattice_expected()
    assert g.edge_index.dtype == torch.int64 and g.edge_index.is_cuda and g.degree.dtype == torch.int32
    assert np.array_equal(g.edge_index.cpu().numpy(), ei) and g.num_edges == ei.shape[1]
    assert np.array_equal(g.degree.cpu().numpy(), degree)
    assert np.array_equal(g.row_start.cpu().numpy(), np.concatenate([[0], np.cumsum(degree)]))
    for got, want in ((g.edges, edges), (g.triplets, trips), (g.max_degree, top), (g.last_bonded, last)):
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and np.array_equal(got, want)
    import x2gnn

    pos, _ = rg.flat(rg.lattice_molecules())
    plain = x2gnn.radius_graph(torch.from_numpy(pos).to(cuda), torch.from_numpy(start))
    assert plain.edge_index_global is None and torch.equal(plain.edge_index, g.edge_index)
    # a cutoff of its own: d^2 = 25 is inside 5.5, and d = 1 is not inside 1
    wide = x2gnn.radius_graph(torch.from_numpy(pos).to(cuda), start, cutoff=5.5)
    assert np.array_equal(wide.edge_index.cpu().numpy(), rg.lattice_expected(cutoff_sq=30.25)[0])
    assert x2gnn.radius_graph(torch.from_numpy(pos).to(cuda), start, cutoff=1.0).num_edges == 0


def test_no_atoms_and_no_molecules(cuda):
    import x2gnn

    g = x2gnn.radius_graph(torch.zeros((0, 3), device=cuda), np.array([0, 0, 0]), global_ids=True)
    assert g.num_edges == 0 and g.edge_index_global.shape == (2, 0) and g.row_start.tolist() == [0]
    assert g.edges.tolist() == [0, 0] and g.last_bonded.tolist() == [-1, -1] and g.degree.shape == (0,)
    g = x2gnn.radius_graph(torch.zeros((0, 3), device=cuda), np.array([0]))
    assert g.num_edges == 0 and g.edges.shape == (0,)
    with pytest.raises(ValueError, match="atom_start"):
        x2gnn.radius_graph(torch.zeros((3, 3), device=cuda), np.array([0, 2]))


def test_non_finite_coordinates_give_no_edge(cuda):
    R = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 1, 0], [3e38, 0, 0]], np.float32)
    g, _ = _run(cuda, [R])
    assert np.array_equal(g.edge_index.cpu().numpy(), rg.edges_of(rg.adjacency(R[:5])))
    assert g.degree.tolist() == [2, 2, 0, 0, 2, 0] and g.last_bonded.tolist() == [4]


# ------------------------------------------------------------------------------------------------- the table's fixtures
@pytest.fixture(scope="module")
def results(cuda):
    """Each fixture's molecules in one call, made once: name -> (molecules, result, atom_start, edge_index on the
    host)."""
    cache = {}

    def get(name):
        if name not in cache:
            mols = rg.FIXTURES[name][0]()
            g, start = _run(cuda, mols)
            cache[name] = (mols, g, start, g.edge_index.cpu().numpy())
        return cache[name]

    return get


@pytest.mark.parametrize("name", list(rg.FIXTURES))
def test_fixture_against_the_statement(results, name):
    from x2gnn.device_dataset import molecule_stats

    mols, g, start, ei = results(name)
    cap = rg.FIXTURES[name][1]
    edge_start = np.concatenate([[0], np.cumsum(g.edges)])
    assert ei.shape[1] == edge_start[-1] == int(g.row_start[-1])

    def got(k):
        return rg.adjacency_from_edges(ei[:, edge_start[k]:edge_start[k + 1]], len(mols[k]))

    wrong, undecided, pairs, asym = rg.compare(mols, got)
    print(f"{name}: {pairs} ordered pairs, {undecided} undecided ({undecided / pairs:.3g}, cap {cap:g}), "
          f"{wrong} decided pairs wrong, {asym} molecules not symmetric")
    assert wrong == 0 and asym == 0
    assert undecided <= cap * pairs
    # argwhere order: the adjacency's own row-major listing is the edge list (which also says: no edge twice)
    for k in range(len(mols)):
        assert np.array_equal(rg.edges_of(got(k)), ei[:, edge_start[k]:edge_start[k + 1]]), f"molecule {k}: order"
    nodes = np.diff(start)
    trips, top, sym = molecule_stats(nodes, g.edges, ei)
    assert np.array_equal(g.triplets, trips) and np.array_equal(g.max_degree, top) and sym.all()
    mol_of_edge = np.repeat(np.arange(len(mols)), g.edges)
    assert np.array_equal(g.edge_index_global.cpu().numpy(), ei + start[:-1][mol_of_edge][None, :])
    deg = np.bincount(g.edge_index_global[0].cpu().numpy(), minlength=int(start[-1]))
    assert np.array_equal(g.degree.cpu().numpy(), deg)
    assert np.array_equal(g.row_start.cpu().numpy(), np.concatenate([[0], np.cumsum(deg)]))
    last = np.array([ei[:, edge_start[k]:edge_start[k + 1]].max(initial=-1) for k in range(len(mols))])
    assert np.array_equal(g.last_bonded, last)


def test_molecules_in_one_call_equal_each_alone_and_two_runs_agree(results, cuda):
    """The 17 AID molecules of the table (the first 16 and the largest) in one call against each in a call of its
    own, and the whole call twice."""
    mols = rg.aid_molecules(list(range(16)) + [21])
    g, start = _run(cuda, mols)
    again, _ = _run(cuda, mols)
    for name in ("edge_index", "edge_index_global", "degree", "row_start"):
        assert torch.equal(getattr(g, name), getattr(again, name)), name
    for name in ("edges", "triplets", "max_degree", "last_bonded"):
        assert np.array_equal(getattr(g, name), getattr(again, name)), name
    ei = g.edge_index.cpu().numpy()
    edge_start = np.concatenate([[0], np.cumsum(g.edges)])
    for k, R in enumerate(mols):
        one, _ = _run(cuda, [R])
        assert np.array_equal(one.edge_index.cpu().numpy(), ei[:, edge_start[k]:edge_start[k + 1]]), k
        assert np.array_equal(one.degree.cpu().numpy(), g.degree[start[k]:start[k + 1]].cpu().numpy())
        assert (one.edges[0], one.triplets[0], one.max_degree[0], one.last_bonded[0]) == \
            (g.edges[k], g.triplets[k], g.max_degree[k], g.last_bonded[k])


def test_sentinel_tails_on_a_multi_tile_scan(cuda):
    """AID's first 40 molecules: more atoms than one scan tile of 2048, rows of one to three 64-lane steps."""
    mols = rg.aid_molecules(range(40))
    pos, start = rg.flat(mols)
    assert len(pos) > 2048
    raw = Raw(cuda, pos, start)
    got = raw.count()
    E = int(got["row_start"][-1])
    local, glob = raw.fill(E)
    g, _ = _run(cuda, mols)
    assert np.array_equal(local, g.edge_index.cpu().numpy()) and np.array_equal(glob, g.edge_index_global.cpu().numpy())
    assert np.array_equal(got["degree"], g.degree.cpu().numpy()) and np.array_equal(got["mol_edges"], g.edges)
    assert np.array_equal(got["row_start"], np.concatenate([[0], np.cumsum(got["degree"])]))


def test_fill_never_writes_at_or_beyond_num_edges(cuda):
    """The fill told a smaller E than row_start holds: the slots below it are the true edges' source row, nothing is
    written from E on (the buffers hold E slots and a sentinel tail)."""
    pos, start = rg.flat(rg.lattice_molecules())
    raw = Raw(cuda, pos, start)
    E = int(raw.count()["row_start"][-1])
    full, _ = raw.fill(E)
    short, short_glob = raw.fill(E - 5)
    assert np.array_equal(short[0], full[0, :E - 5]) and np.array_equal(short[1], full[1, :E - 5])
    assert np.array_equal(short_glob[0] - short[0], np.repeat(start[:-1], rg.lattice_expected()[2])[:E - 5])
    # a row_start that points outside: nothing is written there either
    raw.out["row_start"][:raw.N + 1] = torch.tensor([-3] + [E + 7] * raw.N, device=cuda)
    wild, _ = raw.fill(E)
    assert ((wild == S64) | ((wild >= 0) & (wild < 6))).all()


# ------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("override", [
    dict(pos=None), dict(atom_start=None), dict(degree=None), dict(row_start=None), dict(mol_edges=None),
    dict(mol_triplets=None), dict(mol_max_degree=None), dict(mol_last_bonded=None), dict(workspace=None),
    dict(N=-1), dict(M=-1),
])
def test_refused_count_writes_nothing(cuda, override):
    pos, start = rg.flat(rg.lattice_molecules())
    Raw(cuda, pos, start).count(want=EINVAL, **override)


def test_unsupported_and_empty_counts_write_nothing(cuda):
    pos, start = rg.flat(rg.lattice_molecules())
    raw = Raw(cuda, pos, start)
    raw.count(want=EUNSUPPORTED, N=1 << 31)
    raw.count(want=EUNSUPPORTED, M=1 << 31)
    for kw in (dict(N=0), dict(M=0)):  # X2G_OK without a launch: every output keeps its sentinel
        raw.count(want=OK, **kw)
        for k, v in raw.out.items():
            h = v.cpu().numpy()
            assert (h == (S32 if h.dtype == np.int32 else S64)).all(), k


def test_refused_fill_writes_nothing(cuda):
    pos, start = rg.flat(rg.lattice_molecules())
    raw = Raw(cuda, pos, start)
    E = int(raw.count()["row_start"][-1])
    for want, kw in ((EINVAL, dict(pos=None)), (EINVAL, dict(atom_start=None)), (EINVAL, dict(row_start=None)),
                     (EINVAL, dict(edge_local=None)), (EINVAL, dict(N=-1)), (EINVAL, dict(M=-1)),
                     (EINVAL, dict(E=-1)), (EUNSUPPORTED, dict(N=1 << 31)), (OK, dict(E=0)), (OK, dict(N=0)),
                     (OK, dict(M=0))):
        kw = dict(kw)
        local, glob = raw.fill(kw.pop("E", E), want=want, rows=E, **kw)
        assert (local == S64).all() and (glob == S64).all(), kw


def test_untrusted_atom_start_reads_and_writes_nothing_outside(cuda):
    """Ranges that are reversed, negative or beyond N: the atoms they would own get degree 0, their molecules zero
    counts and -1, and the molecule that is in order keeps its edges."""
    R = rg.lattice_molecules()[0]
    pos = np.concatenate([R, R])
    ei = rg.lattice_expected()[0][:, :int(rg.lattice_expected()[2][0])]
    for start, good in (([0, 6, 40], 0), ([0, 6, -2, 12], 0), ([0, 6, 3, 12], 0), ([-5, 6, 12], 1)):
        raw = Raw(cuda, pos, np.array(start, np.int64))
        got = raw.count()
        assert got["mol_edges"][good] == ei.shape[1], start
        assert got["row_start"][-1] == got["degree"].sum()
        local, _ = raw.fill(int(got["row_start"][-1]))
        assert ((local >= 0) & (local < 12)).all()


# ------------------------------------------------------------------------------------------------- out=
def _records_and_matrices():
    """Three molecules of 3, 4 and 5 atoms, all inside the cutoff (6, 12 and 20 edges), with seeded matrices of
    matching AO counts."""
    from x2gnn import datasets as ds
    from x2gnn.features import AOMatrices

    rng = np.random.default_rng(2024)
    zs = ([8, 1, 1], [6, 1, 1, 1], [6, 8, 1, 1, 1])
    recs, parts = [], []
    for k, z in enumerate(zs):
        R = torch.from_numpy(rng.uniform(-1.2, 1.2, size=(len(z), 3)).astype(np.float32))
        recs.append(ds.MolRecord(atom="", R=R, Z=torch.tensor(z), N=torch.tensor([len(z)]),
                                 Label=torch.tensor([float(k) - 0.5]), idx=torch.tensor([k])))
        counts = [9 if a == 1 else 39 for a in z]
        nao = sum(counts)
        S, H = ar.random_symmetric(rng, nao, -4.0, 0.0), ar.random_symmetric(rng, nao, -4.0, 0.0)
        parts.append((S, H, ar.aoslice_of(counts), sum(z)))
    return recs, AOMatrices.from_molecules(parts), parts


def _s160_records_and_matrices(n=12):
    """``n`` S160 molecules (9 heavy atoms and 9 hydrogens each: 432 functions) with seeded symmetric matrices."""
    from x2gnn import datasets as ds
    from x2gnn.features import AOMatrices
    from x2gnn.synth import SHAPES, random_geometry

    geo, rng = np.random.default_rng(0), np.random.default_rng(99)
    recs, parts = [], []
    for k in range(n):
        z, pos = random_geometry(geo, SHAPES["S160"])
        recs.append(ds.MolRecord(atom="", R=torch.from_numpy(pos.astype(np.float32)), Z=torch.from_numpy(z),
                                 N=torch.tensor([len(z)]), Label=torch.tensor([0.25 * k]), idx=torch.tensor([k])))
        counts = [9 if a == 1 else 39 for a in z]
        nao = sum(counts)
        parts.append((ar.random_symmetric(rng, nao, -4.0, 0.0), ar.random_symmetric(rng, nao, -4.0, 0.0),
                      ar.aoslice_of(counts), int(z.sum())))
    return recs, AOMatrices.from_molecules(parts), parts


def test_ao_edge_features_into_a_slice(cuda):
    from x2gnn.features import ao_edge_features

    recs, ao, _ = _records_and_matrices()
    pos = torch.cat([r.R for r in recs]).to(cuda)
    g = __import__("x2gnn").radius_graph(pos, ao.atom_start, global_ids=True)
    E = g.num_edges
    assert E == 38
    dev = ao.to(cuda)
    want = ao_edge_features(dev, g.edge_index_global, dev.atom_mol())
    big = torch.full((E + 4, 338), S32, dtype=torch.int32, device=cuda).view(torch.float32)
    back = ao_edge_features(dev, g.edge_index_global, dev.atom_mol(), out=big[2:E + 2])
    assert back.data_ptr() == big[2:].data_ptr() and tuple(back.shape) == (E, 338)
    bits = big.view(torch.int32)
    assert torch.equal(bits[2:E + 2], want.view(torch.int32))
    assert bool((bits[:2] == S32).all()) and bool((bits[E + 2:] == S32).all())
    for bad in (big[2:E + 1], big[2:E + 2].to(torch.float64), big[2:E + 2].cpu(), big[2:E + 2, :337],
                big.view(-1)[:E * 338], torch.zeros((338, E), device=cuda).t(), np.zeros((E, 338), np.float32)):
        with pytest.raises(ValueError, match="out must be"):
            ao_edge_features(dev, g.edge_index_global, dev.atom_mol(), out=bad)
    assert bool((bits[:2] == S32).all()) and bool((bits[E + 2:] == S32).all())


# ------------------------------------------------------------------------------------------------- from_records
TENSORS = ("x", "atom_pos", "edge_index", "edge_attr", "y", "mol_trips")
CACHES = ("nodes", "edges", "triplets", "max_degree", "symmetric", "atom_start", "edge_start")


def _assert_same_dataset(new, old):
    for k in TENSORS:
        a, b = getattr(new, k), getattr(old, k)
        assert a.dtype == b.dtype and a.device == b.device and a.shape == b.shape, k
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b), k
    for k in CACHES:
        a, b = getattr(new, k), getattr(old, k)
        assert isinstance(a, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b), k
    assert new.num_features == old.num_features == 338 and len(new) == len(old) and new.device == old.device


@pytest.fixture(scope="module")
def old_path(cuda):
    """The parent's path, made once per record set: name -> (records, matrices, DeviceDataset)."""
    import x2gnn
    from x2gnn import datasets as ds

    out = {}
    for name, make in (("three", _records_and_matrices), ("s160", _s160_records_and_matrices)):
        recs, ao, _ = make()
        out[name] = (recs, ao, x2gnn.DeviceDataset(ds.records_to_data(recs, ao, cuda), cuda))
    return out


@pytest.mark.parametrize("name", ["three", "s160"])
@pytest.mark.parametrize("per_launch", [1 << 18, 1])
def test_from_records_equals_the_round_trip(cuda, old_path, name, per_launch):
    import x2gnn

    recs, ao, old = old_path[name]
    new = x2gnn.DeviceDataset.from_records(recs, ao, cuda, max_edges_per_launch=per_launch)
    if name == "three":
        assert new.edges.tolist() == [6, 12, 20]
    _assert_same_dataset(new, old)
    assert bool(torch.isfinite(new.edge_attr).all())


def _energies(batch, cuda):
    """The batch through a seeded two-layer xgnn_poly, made anew for every batch (as tests/test_gpu_device_dataset.py
    compares two batches: each sees a model in the same state)."""
    import x2gnn

    torch.manual_seed(0)
    model = x2gnn.xgnn_poly(device="cuda", conv_layers=2, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16,
                            embedding_size=128).to(cuda).eval()
    with torch.no_grad():
        return model(batch).detach().clone()


@pytest.mark.parametrize("name", ["three", "s160"])
def test_from_records_batches_run_the_model_to_the_same_bits(cuda, old_path, name):
    import x2gnn

    recs, ao, old = old_path[name]
    new = x2gnn.DeviceDataset.from_records(recs, ao, cuda)
    idx = list(range(len(recs)))[::-1]
    a, b = new.batch(idx), old.batch(idx)
    assert list(a._store) == list(b._store)
    for k in a._store:
        va, vb = a._store[k], b._store[k]
        assert torch.equal(va, vb) if torch.is_tensor(va) else va == vb, k
    ya, yb = _energies(a, cuda), _energies(b, cuda)
    assert tuple(ya.shape) == (len(recs),) and bool(torch.isfinite(ya).all()) and torch.equal(ya, yb)


def test_from_records_names_a_record_whose_last_atom_is_out_of_reach(cuda):
    """Record 1's last hydrogen moved 30 A away: its bonds reach atom 2 of 4, the matrices have 4 atoms."""
    import x2gnn
    from x2gnn import datasets as ds

    recs, ao, _ = _records_and_matrices()
    R = recs[1].R.clone()
    R[3] += 30.0
    recs[1] = ds.MolRecord(atom="", R=R, Z=recs[1].Z, N=recs[1].N, Label=recs[1].Label, idx=torch.tensor([41]))
    with pytest.raises(ValueError, match=r"record 1 \(idx 41\)"):
        x2gnn.DeviceDataset.from_records(recs, ao, cuda)
    with pytest.raises(ValueError, match=r"record 1 \(idx 41\)"):
        ds.records_to_data(recs, ao, cuda)


def test_from_records_without_records(cuda):
    import x2gnn
    from x2gnn.features import AOMatrices

    new, old = x2gnn.DeviceDataset.from_records([], AOMatrices.from_molecules([]), cuda), x2gnn.DeviceDataset([], cuda)
    assert len(new) == 0 and new.edge_attr is None and old.edge_attr is None and new.num_features == old.num_features
    for k in CACHES:
        assert np.array_equal(getattr(new, k), getattr(old, k)) and getattr(new, k).dtype == getattr(old, k).dtype, k
    for k in ("x", "atom_pos", "edge_index", "y"):
        assert getattr(new, k).shape == getattr(old, k).shape and getattr(new, k).dtype == getattr(old, k).dtype, k
