"""x2gnn.padding on the host (no GPU): the filler graph has exactly the counts asked for everywhere in the region
the module promises, never other counts anywhere, and DeviceDataset.capacity keeps an epoch inside that region."""
import numpy as np
import pytest

from padded_cases import FILLERS, INDEX_LISTS, molecules


def check_filler(fl, dn, de, dt, C, F):
    """Every property of a filler graph the padded batch relies on; the counts recounted by the dataset's own
    statistics (device_dataset.molecule_stats)."""
    from x2gnn.device_dataset import molecule_stats
    from x2gnn.padding import CUTOFF

    assert fl.x.shape == (dn,) and fl.atom_pos.shape == (dn, 3) and fl.edge_index.shape == (2, de)
    assert fl.x.dtype == np.int64 and fl.atom_pos.dtype == np.float32 and fl.edge_index.dtype == np.int64
    assert fl.nodes.shape == fl.edges.shape == fl.triplets.shape == (F,)
    assert int(fl.nodes.sum()) == dn and int(fl.edges.sum()) == de and int(fl.triplets.sum()) == dt
    assert (fl.edges >= 1).all()  # every filler molecule has an edge
    src, dst = fl.edge_index
    assert ((src >= 0) & (src < dn) & (dst >= 0) & (dst < dn)).all()
    assert (src != dst).all()  # no self-loop
    key = src * dn + dst
    assert (np.diff(key) > 0).all()  # sorted by (src, dst), no edge twice
    assert np.array_equal(np.sort(dst * dn + src), key)  # symmetric
    assert int(np.bincount(src, minlength=dn).max()) <= C
    # the molecules' atoms and edges are consecutive and no edge leaves its molecule
    a_end, e_end = np.cumsum(fl.nodes), np.cumsum(fl.edges)
    mol_of_atom = np.searchsorted(a_end, np.arange(dn), side="right")
    mol_of_edge = np.searchsorted(e_end, np.arange(de), side="right")
    assert np.array_equal(mol_of_atom[src], mol_of_edge) and np.array_equal(mol_of_atom[dst], mol_of_edge)
    # recount, molecule by molecule, with molecule-local ids as the dataset holds them
    a_start = np.concatenate([[0], a_end[:-1]])
    local = fl.edge_index - a_start[mol_of_edge]
    trips, max_deg, sym = molecule_stats(fl.nodes, fl.edges, local)
    assert np.array_equal(trips, fl.triplets) and int(trips.sum()) == dt
    assert sym.all() and int(max_deg.max()) <= C
    d = np.linalg.norm(fl.atom_pos[src].astype(np.float64) - fl.atom_pos[dst].astype(np.float64), axis=1)
    assert (d > 0).all() and (d < CUTOFF).all()


def test_position_table_points_are_distinct_and_within_the_cutoff():
    from x2gnn.padding import CUTOFF, POSITIONS

    p = POSITIONS.astype(np.float64)
    assert p.shape[0] >= 1024 and p.dtype == np.float64 and POSITIONS.dtype == np.float32
    head = p[:300]
    d = np.linalg.norm(head[:, None] - head[None], axis=-1)
    assert (d[~np.eye(len(head), dtype=bool)] > 0.1).all()
    assert 2 * np.linalg.norm(p, axis=1).max() < CUTOFF  # any two points: closer than the cutoff
    assert len(np.unique(POSITIONS, axis=0)) == len(POSITIONS)


@pytest.mark.parametrize("C", [3, 4, 5, 6])
@pytest.mark.parametrize("F", FILLERS)
def test_filler_plan_exhaustively_for_small_sizes(C, F):
    """Every (dn, de, dt) with dn < 12: inside the region a graph of exactly these counts; outside it None or,
    where a graph is returned all the same, again exactly these counts."""
    from x2gnn.padding import filler_plan, in_region

    inside = 0
    for dn in range(0, 12):
        for de in range(0, C * dn + 4, 2):
            for dt in range(0, C * (C - 1) * dn + 4, 2):
                fl = filler_plan(dn, de, dt, C, F)
                if in_region(dn, de, dt, C, F):
                    inside += 1
                    assert fl is not None, (dn, de, dt)
                if fl is not None:
                    check_filler(fl, dn, de, dt, C, F)
    assert inside >= 20  # (the region is not empty at these sizes)


def test_filler_plan_refuses_what_no_graph_has():
    from x2gnn.padding import filler_plan, in_region

    for args in [(10, 7, 4, 5, 1), (10, 8, 3, 5, 1),   # odd counts
                 (4, 12, 24, 2, 1),                      # K4's counts, but its degree 3 is above C
                 (4, 14, 30, 5, 1),                      # more edges than 4 atoms hold
                 (30, 20, 400, 17, 1),                   # more triplets than 20 edge ends make at degree <= 17
                 (20, 40, 2, 6, 1),                      # fewer than the even spread
                 (3, 4, 2, 5, 2), (1, 2, 0, 5, 1), (10, 10, 10, 0, 1), (10, 10, 10, 5, 0), (-1, 2, 0, 3, 1)]:
        assert filler_plan(*args) is None, args
        assert not in_region(*args), args
    fl = filler_plan(4, 12, 24, 3, 1)  # K4 itself
    assert fl is not None
    check_filler(fl, 4, 12, 24, 3, 1)


@pytest.mark.parametrize("C", [12, 17, 28, 61])
def test_filler_plan_on_a_seeded_sample_of_larger_sizes(C):
    """Config 2's degrees reach 17, QM9's 28, config 5's 61: points drawn from the whole region (its lowest and
    highest triplet counts included)."""
    from x2gnn.padding import filler_plan, in_region, region_bounds

    rng = np.random.default_rng(100 + C)
    done = 0
    while done < 60:
        F = int(rng.integers(1, 4))
        dn = int(rng.integers(4, 500))
        de = 2 * int(rng.integers(1, C * dn // 2))
        b = region_bounds(dn - 2 * (F - 1), de - 2 * (F - 1), C)
        if b is None:
            continue
        pick = done % 3
        dt = b[0] if pick == 0 else b[1] if pick == 1 else b[0] + 2 * int(rng.integers(0, (b[1] - b[0]) // 2 + 1))
        assert in_region(dn, de, dt, C, F)
        fl = filler_plan(dn, de, dt, C, F)
        assert fl is not None, (dn, de, dt, C, F)
        check_filler(fl, dn, de, dt, C, F)
        assert not in_region(dn, de, b[1] + 2, C, F) and not in_region(dn, de, b[0] - 2, C, F)
        done += 1


def _dataset():
    import x2gnn

    return x2gnn.DeviceDataset(molecules(), "cpu")


def test_the_index_lists_differ_in_every_count():
    ds = _dataset()
    assert ds.symmetric.all() and len(ds) == 12
    for per in (ds.nodes, ds.edges, ds.triplets):
        totals = [int(per[i].sum()) for i in INDEX_LISTS]
        assert len(set(totals)) == len(INDEX_LISTS) >= 4, totals
    assert all(len(i) == 3 for i in INDEX_LISTS)
    assert INDEX_LISTS[0][0] == 7 and ds.nodes[7] == 2 and any(6 in i for i in INDEX_LISTS)


@pytest.mark.parametrize("F", FILLERS)
def test_capacity_makes_every_list_solvable(F):
    from x2gnn import ops
    from x2gnn.padding import Capacity, filler_plan, in_region

    ds = _dataset()
    cap = ds.capacity(INDEX_LISTS, fillers=F)
    assert isinstance(cap, Capacity) and cap == ds.capacity([np.asarray(i) for i in INDEX_LISTS], fillers=F)
    assert (cap.real_graphs, cap.fillers, cap.graphs) == (3, F, 3 + F)
    pool = sorted({i for l in INDEX_LISTS for i in l})
    assert cap.max_degree == int(ds.max_degree[pool].max()) == 17  # the pool's own: no filler raises it
    assert int(ds.nodes[pool].max()) <= cap.max_mol_atoms <= ops.MOL_ROWPTR_MAX_ATOMS
    assert cap.edges % 2 == 0 and cap.triplets % 2 == 0
    for idx in INDEX_LISTS:
        dn, de, dt = (cap.nodes - int(ds.nodes[idx].sum()), cap.edges - int(ds.edges[idx].sum()),
                      cap.triplets - int(ds.triplets[idx].sum()))
        assert in_region(dn, de, dt, cap.max_degree, F), idx
        fl = filler_plan(dn, de, dt, cap.max_degree, F)
        assert fl is not None, idx
        check_filler(fl, dn, de, dt, cap.max_degree, F)
        assert int(fl.nodes.max()) <= cap.max_mol_atoms
    with pytest.raises(AttributeError):
        cap.nodes = 1  # frozen


def test_capacity_refuses_ragged_lists_and_a_non_symmetric_pool():
    import x2gnn
    from device_dataset_cases import mixed_molecules

    ds = _dataset()
    with pytest.raises(ValueError, match="same length"):
        ds.capacity([[0, 1, 2], [3, 4]])
    with pytest.raises(ValueError, match="at least one"):
        ds.capacity([])
    with pytest.raises(IndexError):
        ds.capacity([[0, 1, 12]])
    with pytest.raises(ValueError, match="fillers"):
        ds.capacity(INDEX_LISTS, fillers=0)
    mixed = x2gnn.DeviceDataset(mixed_molecules(), "cpu")
    with pytest.raises(ValueError, match="symmetric"):
        mixed.capacity([[0, 1, 8], [2, 3, 4]])
    assert mixed.capacity([[0, 1, 9], [2, 3, 4]]).real_graphs == 3  # (the same dataset without that molecule)
    with pytest.raises(ValueError, match="reach"):
        ds.capacity([[7, 7, 7], [7, 7, 7]])  # degree 1 only: no filler has a triplet to vary
