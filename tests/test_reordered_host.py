"""DeviceDataset.reordered on the host (device "cpu"): the reordered dataset against one built from the reordered
molecules — every cache and every tensor — for permutations, subsets, repeats and negative indices."""
import numpy as np
import pytest
import torch

from device_dataset_cases import mixed_molecules

CACHES = ("nodes", "edges", "triplets", "max_degree", "symmetric", "atom_start", "edge_start")
TENSORS = ("x", "atom_pos", "edge_index", "edge_attr", "y", "mol_trips")


def assert_same_dataset(a, b):
    for k in CACHES:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype, k
        np.testing.assert_array_equal(x, y, err_msg=k)
    assert a.num_features == b.num_features and len(a) == len(b) and a.device == b.device
    for k in TENSORS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape and x.is_contiguous() and torch.equal(x, y), k


@pytest.fixture(scope="module")
def mols():
    return mixed_molecules()


@pytest.fixture(scope="module")
def dataset(mols):
    import x2gnn

    return x2gnn.DeviceDataset(mols, "cpu")


# positions in mixed_molecules(): 0-5 S160, 6 S5A, 7 the 2-atom molecule, 8 the 3-atom non-symmetric one (odd E), 9 S160
@pytest.mark.parametrize("order", [[8, 3, 6, 0, 9, 7, 2, 5, 1, 4], list(range(10)), list(range(9, -1, -1)), [9, 8],
                                   [2, 2, 7], [7], [-1, 0, -10]])
def test_reordered_equals_a_dataset_of_the_reordered_molecules(dataset, mols, order):
    import x2gnn

    got = dataset.reordered(order)
    assert_same_dataset(got, x2gnn.DeviceDataset([mols[i] for i in order], "cpu"))
    assert got.edge_attr.data_ptr() != dataset.edge_attr.data_ptr()  # its own storage, the source untouched
    assert_same_dataset(dataset, x2gnn.DeviceDataset(mols, "cpu"))


def test_reordering_twice_composes(dataset, mols):
    import x2gnn

    p, q = [8, 3, 6, 0, 9, 7, 2, 5, 1, 4], [4, 4, 0, 9, 1]
    assert_same_dataset(dataset.reordered(p).reordered(q), x2gnn.DeviceDataset([mols[p[i]] for i in q], "cpu"))


def test_a_split_of_the_reordered_dataset_is_contiguous_slabs(dataset):
    """The reference's regime (trainer.py:23-27): permute once, cut the splits unshuffled.  Every batch of such a
    loader is a run of molecules, and its edge_attr rows are one slab of the reordered dataset."""
    perm = np.random.default_rng(5).permutation(10)
    ds = dataset.reordered(perm)
    loader = ds.loader(3, shuffle=False, indices=range(2, 10))
    lists = loader.index_lists()
    assert [len(i) for i in lists] == [3, 3, 2]
    for idx in lists:
        assert (np.diff(idx) == 1).all()
        lo, hi = int(ds.edge_start[idx[0]]), int(ds.edge_start[idx[-1] + 1])
        want = torch.cat([dataset.edge_attr[int(dataset.edge_start[m]):int(dataset.edge_start[m + 1])]
                          for m in perm[idx]])
        assert torch.equal(ds.edge_attr[lo:hi], want)


def test_reordered_refuses_an_index_outside_the_dataset(dataset):
    with pytest.raises(IndexError):
        dataset.reordered([0, 10])
    with pytest.raises(IndexError):
        dataset.reordered([-11])
    empty = dataset.reordered([])
    assert len(empty) == 0 and empty.edge_attr.shape == (0, 338) and empty.edge_start.tolist() == [0]
