"""x2gnn.DeviceDataset's host side (no GPU): the vectorised per-molecule statistics, the epoch loader's index
semantics, the index check in front of every launch, and x2g_batch_assemble's argument checks."""
import ctypes

import numpy as np
import pytest

from device_dataset_cases import mixed_molecules


def test_vectorised_molecule_statistics_equal_per_molecule_calls():
    from x2gnn.data import _is_symmetric
    from x2gnn.device_dataset import molecule_stats
    from x2gnn.synth import triplet_count

    mols = mixed_molecules()
    # a multigraph (one directed edge twice, its multiset symmetric), an edgeless atom and an edgeless molecule
    dup = {"x": np.array([6, 6, 1]), "edge_index": np.array([[0, 0, 1, 1], [1, 1, 0, 0]], dtype=np.int64)}
    lone = {"x": np.array([8]), "edge_index": np.zeros((2, 0), dtype=np.int64)}
    mols = mols[:3] + [dup, lone] + mols[3:]
    nodes = np.array([len(m["x"]) for m in mols])
    edges = np.array([m["edge_index"].shape[1] for m in mols])
    trips, max_deg, sym = molecule_stats(nodes, edges, np.concatenate([m["edge_index"] for m in mols], axis=1))
    assert trips.dtype == np.int64 and max_deg.dtype == np.int64 and sym.dtype == bool
    for i, m in enumerate(mols):
        ei, n = m["edge_index"], len(m["x"])
        assert trips[i] == triplet_count(ei, n), i
        assert max_deg[i] == (int(np.bincount(ei[0], minlength=n).max()) if ei.shape[1] else 0), i
        assert bool(sym[i]) == _is_symmetric(ei, n), i
    assert not sym[3] and sym[4] and not sym[10] and sym[9]
    for m in mixed_molecules():
        assert "triplet_num" not in m or m["triplet_num"] == triplet_count(m["edge_index"], len(m["x"]))


def test_statistics_refuse_atom_ids_outside_the_molecule():
    from x2gnn.device_dataset import molecule_stats

    with pytest.raises(ValueError, match="molecule-local"):
        molecule_stats([2, 2], [1, 1], np.array([[0, 2], [1, 0]]))  # the second molecule's edge was incremented
    with pytest.raises(ValueError, match="edges"):
        molecule_stats([2], [3], np.array([[0, 1], [1, 0]]))


def test_host_caches_of_a_dataset():
    import x2gnn

    mols = mixed_molecules()
    ds = x2gnn.DeviceDataset(mols, "cpu")
    assert len(ds) == 10
    np.testing.assert_array_equal(ds.nodes, [len(m["x"]) for m in mols])
    np.testing.assert_array_equal(ds.edges, [m["edge_num"] for m in mols])
    np.testing.assert_array_equal(ds.triplets, [m["triplet_num"] for m in mols])
    np.testing.assert_array_equal(ds.atom_start, np.concatenate([[0], np.cumsum(ds.nodes)]))
    np.testing.assert_array_equal(ds.edge_start, np.concatenate([[0], np.cumsum(ds.edges)]))
    assert ds.symmetric.tolist() == [True] * 8 + [False, True]
    assert ds.edges[8] % 2 == 1 and ds.triplets[7] == 0
    assert ds.mol_trips.dtype.is_floating_point is False and ds.mol_trips.tolist() == ds.triplets.tolist()
    assert tuple(ds.edge_index.shape) == (2, int(ds.edges.sum())) and int(ds.edge_index.max()) < int(ds.nodes.max())


def test_loader_covers_an_epoch_reproducibly():
    import x2gnn

    ds = x2gnn.DeviceDataset(mixed_molecules(), "cpu")
    ep = ds.loader(4, seed=5)
    lists = ep.index_lists()
    assert [len(b) for b in lists] == [4, 4, 2] and len(ep) == 3
    assert sorted(np.concatenate(lists).tolist()) == list(range(10))  # each index exactly once
    again = ds.loader(4, seed=5).index_lists()
    assert all(np.array_equal(a, b) for a, b in zip(lists, again))
    other = ds.loader(4, seed=6).index_lists()
    assert not all(np.array_equal(a, b) for a, b in zip(lists, other))
    dropped = ds.loader(4, seed=5, drop_last=True)
    assert [len(b) for b in dropped.index_lists()] == [4, 4] and len(dropped) == 2
    assert all(np.array_equal(a, b) for a, b in zip(dropped.index_lists(), lists))
    plain = ds.loader(3, shuffle=False).index_lists()
    assert np.concatenate(plain).tolist() == list(range(10))
    sub = ds.loader(2, seed=1, indices=[9, 2, 4, 7, -10])
    assert [len(b) for b in sub.index_lists()] == [2, 2, 1]
    assert sorted(np.concatenate(sub.index_lists()).tolist()) == [0, 2, 4, 7, 9]
    with pytest.raises(IndexError):
        ds.loader(2, indices=[3, 10])


def test_batch_refuses_an_index_outside_the_dataset_before_any_launch(monkeypatch):
    import x2gnn
    from x2gnn import _lib

    def no_library(*a, **k):
        raise AssertionError("the library was reached before the index check")

    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "call", no_library)
    ds = x2gnn.DeviceDataset(mixed_molecules(), "cpu")
    for bad in ([-11], [10], [0, 3, 10], [2, -11]):
        with pytest.raises(IndexError):
            ds.batch(bad)
        with pytest.raises(IndexError):
            ds.shard_batch(bad, 2, 0)
    empty = x2gnn.DeviceDataset([], "cpu")
    assert len(empty) == 0
    for bad in ([0], [-1]):
        with pytest.raises(IndexError):
            empty.batch(bad)


def _assemble_args(**over):
    """x2g_batch_assemble's arguments with never-dereferenced pointers (the checks fail first)."""
    p = ctypes.c_void_p(16)
    a = dict(x_all=p, pos_all=p, ei_all=p, stride=100, attr_all=p, F=338, y_all=p, trips_all=p, off=p, B=2, N=5,
             E=8, x=p, pos=p, batch=p, ptr=p, ei=p, attr=p, edge_num=p, y=p, src=p, dst=p, src_t=p, dst_t=p, atom_t=p,
             mol_ptr=p, line_ptr=p, trips=p, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return tuple(a.values())


@pytest.mark.parametrize("over", [
    dict(B=-1), dict(N=-1), dict(E=-1), dict(F=-1), dict(stride=-1),
    dict(off=None), dict(ptr=None), dict(mol_ptr=None), dict(line_ptr=None), dict(edge_num=None),
    dict(x_all=None), dict(pos_all=None), dict(x=None), dict(pos=None), dict(batch=None), dict(atom_t=None),
    dict(ei_all=None), dict(ei=None), dict(src=None), dict(dst=None), dict(src_t=None), dict(dst_t=None),
    dict(attr=None), dict(attr_all=None), dict(y=None), dict(trips_all=None), dict(F=0),
    dict(B=0),  # atoms and edges without a molecule
])
def test_assemble_argument_validation_without_gpu(over):
    from x2gnn import _lib

    assert _lib.load().x2g_batch_assemble(*_assemble_args(**over)) == 1001


def test_assemble_empty_batch_launches_nothing_and_index_overflow_is_unsupported():
    """B = 0 returns 0 with nothing to dereference; the int32 index forms hold atom and edge ids, so a batch of
    2^31 atoms or edges is refused before anything is touched.  (Destination offsets are 64-bit like the source's:
    a batch whose edge_attr passes 2^31 bytes is in range and has no refusal of its own.)"""
    from x2gnn import _lib

    fn = _lib.load().x2g_batch_assemble
    assert fn(*_assemble_args(B=0, N=0, E=0)) == 0
    assert fn(*_assemble_args(E=1 << 31)) == 1002
    assert fn(*_assemble_args(N=1 << 31)) == 1002
    assert fn(*_assemble_args(B=1 << 31)) == 1002
