"""DeviceDataset.reordered on the GPU: the caches, the device tensors and batch() outputs of a dataset built from
the permuted molecules, bit for bit; and a trainer stepping over the reordered dataset's unshuffled split computes
what it computes over the same molecules drawn from the original."""
import numpy as np
import pytest
import torch

from device_dataset_cases import mixed_molecules
from test_gpu_device_dataset import assert_same_batch

pytestmark = pytest.mark.gpu

CFG = dict(conv_layers=2, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)
# positions in mixed_molecules(): 0-5 S160, 6 S5A, 7 the 2-atom molecule, 8 the 3-atom non-symmetric one (odd E), 9 S160
PERM = [8, 3, 6, 0, 9, 7, 2, 5, 1, 4]


@pytest.fixture(scope="module")
def mols():
    return mixed_molecules()


@pytest.fixture(scope="module")
def dataset(cuda, mols):
    import x2gnn

    return x2gnn.DeviceDataset(mols, cuda)


def test_reordered_dataset_equals_one_built_in_that_order(cuda, dataset, mols):
    import x2gnn

    got = dataset.reordered(PERM)
    ref = x2gnn.DeviceDataset([mols[i] for i in PERM], cuda)
    for k in ("nodes", "edges", "triplets", "max_degree", "symmetric", "atom_start", "edge_start"):
        assert getattr(got, k).dtype == getattr(ref, k).dtype, k
        np.testing.assert_array_equal(getattr(got, k), getattr(ref, k), err_msg=k)
    for k in ("x", "atom_pos", "edge_index", "edge_attr", "y", "mol_trips"):
        g, r = getattr(got, k), getattr(ref, k)
        assert g.device == r.device and g.dtype == r.dtype and g.shape == r.shape and g.is_contiguous(), k
        assert torch.equal(g, r), k
    for idx in ([0, 1, 2, 3], [9, 0, 4], [1, 2], [5], list(range(10))):
        b = got.batch(idx)
        assert_same_batch(b, ref.batch(idx))
        assert_same_batch(b, dataset.batch([PERM[i] for i in idx]))
    # an unshuffled split of the reordered dataset: runs of molecules, edge_attr one slab of the dataset each
    for idx in got.loader(3, shuffle=False, indices=range(1, 10)).index_lists():
        lo, hi = int(got.edge_start[idx[0]]), int(got.edge_start[idx[-1] + 1])
        assert torch.equal(got.batch(idx).edge_attr, got.edge_attr[lo:hi])


def test_training_over_the_reordered_split_equals_the_original_molecules(cuda, dataset):
    import x2gnn

    sym = [3, 6, 0, 9, 2, 7, 5, 1, 4]  # (the symmetric molecules: the center-kernel path)
    ds = dataset.reordered(sym)
    res = []
    for reordered in (False, True):
        torch.manual_seed(0)
        tr = x2gnn.Trainer(x2gnn.xgnn_poly(device="cuda", **CFG).to(cuda))
        losses = []
        for idx in ds.loader(4, shuffle=False).index_lists():  # 4, 4 and a ragged 1
            b = ds.batch(idx) if reordered else dataset.batch([sym[i] for i in idx])
            losses.append(tr.step(b).detach().clone())
        torch.cuda.synchronize()
        res.append((torch.stack(losses), tr.opt.flat.clone(), tr.opt.ema.clone()))
    assert res[0][0].shape == (3,) and torch.isfinite(res[0][0]).all()
    for a, b in zip(*res):
        assert torch.equal(a, b)
