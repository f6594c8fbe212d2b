"""x2gnn.DeviceDataset on the GPU: a batch assembled on the device (x2g_batch_assemble) equals the host
collate's, tensor for tensor and bit for bit, and a model or trainer fed with it computes the same bits."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from device_dataset_cases import mixed_molecules

pytestmark = pytest.mark.gpu

CFG = dict(conv_layers=4, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)

# positions in mixed_molecules(): 0-5 S160, 6 S5A, 7 the 2-atom molecule, 8 the 3-atom non-symmetric one (odd E),
# 9 S160
INDEX_LISTS = {
    "all": list(range(10)),
    "permutation": [8, 3, 6, 0, 9, 7, 2, 5, 1, 4],
    "repeat": [2, 6, 2, 8, 8, 0],
    "first": [0],
    "last": [9],
    "tiny_then_odd": [7, 8],
    "odd_first": [8, 9],
    "negative": [-1, -10, 4],
}


@pytest.fixture(scope="module")
def mols():
    return mixed_molecules()


@pytest.fixture(scope="module")
def dataset(cuda, mols):
    import x2gnn

    return x2gnn.DeviceDataset(mols, cuda)


def collated(mols, idx, cuda, monkeypatch):
    """The host collate's batch on the device, the schedule left to the device as DeviceDataset leaves it."""
    from x2gnn import data as xdata

    monkeypatch.setattr(xdata, "HOST_SCHEDULE", False)
    return xdata.collate([mols[i] for i in idx]).to(cuda)


def assert_same_batch(got, ref):
    assert list(got._store) == list(ref._store)  # the same keys (in the same order)
    for k, r in ref._store.items():
        g = got._store[k]
        if torch.is_tensor(r):
            assert torch.is_tensor(g) and g.dtype == r.dtype and g.shape == r.shape and g.device == r.device, k
            assert torch.equal(g, r), k
        else:
            assert type(g) is type(r) and g == r, k
    gm, rm = got.host_meta(), ref.host_meta()
    assert set(gm) == set(rm)
    for k in rm:
        assert gm[k].dtype == rm[k].dtype
        np.testing.assert_array_equal(gm[k], rm[k])
    assert got.num_graphs == ref.num_graphs and got.num_nodes == ref.num_nodes


@pytest.mark.parametrize("name", list(INDEX_LISTS))
def test_assembled_batch_equals_collate(cuda, monkeypatch, dataset, mols, name):
    """Every tensor, scalar and host array of batch(idx) equals collate's; once on plain torch.empty outputs and
    once with every output pre-filled with a sentinel (NaN / a negative id) that must be gone afterwards: no
    element is left unwritten, whatever the slab sizes and alignments."""
    idx = INDEX_LISTS[name]
    ref = collated(mols, idx, cuda, monkeypatch)
    assert_same_batch(dataset.batch(idx), ref)
    monkeypatch.setattr(dataset, "_debug_fill", (-7777, float("nan")))
    got = dataset.batch(np.asarray(idx))
    for k, v in got._store.items():
        if torch.is_tensor(v):
            gone = not bool(torch.isnan(v).any()) if v.dtype.is_floating_point else not bool((v == -7777).any())
            assert gone, k
    assert_same_batch(got, ref)
    if 8 in idx or -2 in idx:
        assert got._store["_x2g_symmetric"] is False
    if name == "odd_first":  # the slab behind the odd one starts 8 bytes off a 16-byte boundary
        assert (int(got.edge_num[0]) * 338 * 4) % 16 == 8


def test_batches_stay_valid_after_later_ones(cuda, monkeypatch, dataset, mols):
    """Outputs are fresh allocations: earlier batches are untouched by later calls (more calls than staging slots)."""
    lists = [[0, 1], [6], [7, 8, 9], [2, 2], [5, 4, 3], [9, 0]]
    got = [dataset.batch(i) for i in lists]
    torch.cuda.synchronize()
    for g, i in zip(got, lists):
        assert_same_batch(g, collated(mols, i, cuda, monkeypatch))


def _fwd_bwd(batch, cuda):
    import x2gnn

    torch.manual_seed(0)
    m = x2gnn.xgnn_poly(device="cuda", **CFG).to(cuda)
    e = m(batch)
    loss = torch.nn.functional.smooth_l1_loss(e, batch.y)
    loss.backward()
    torch.cuda.synchronize()
    return e.detach().clone(), loss.detach().clone(), [p.grad.detach().clone() for p in m.parameters()
                                                       if p.grad is not None]


def test_model_on_assembled_batch_equals_collated_bitwise(cuda, monkeypatch, dataset, mols):
    idx = [4, 0, 5, 2, 9]
    ref = collated(mols, idx, cuda, monkeypatch)
    got = dataset.batch(idx)
    assert got._store["_x2g_symmetric"] is True
    e_r, l_r, g_r = _fwd_bwd(ref, cuda)
    e_g, l_g, g_g = _fwd_bwd(got, cuda)
    assert torch.isfinite(e_r).all() and len(g_r) > 10
    assert torch.equal(e_g, e_r) and torch.equal(l_g, l_r)
    assert len(g_g) == len(g_r)
    for a, r in zip(g_g, g_r):
        assert torch.equal(a, r)


def test_trainer_steps_on_fresh_batches_equal_collated_bitwise(cuda, monkeypatch, dataset, mols):
    import x2gnn
    from x2gnn.train import Trainer

    lists = [[0, 1, 2, 3], [5, 4, 9, 0], [3, 3, 1, 2, 5]]
    res = []
    for fresh in (False, True):
        torch.manual_seed(0)
        tr = Trainer(x2gnn.xgnn_poly(device="cuda", **CFG).to(cuda))
        losses = []
        for idx in lists:
            b = dataset.batch(idx) if fresh else collated(mols, idx, cuda, monkeypatch)
            losses.append(tr.step(b).detach().clone())
        torch.cuda.synchronize()
        res.append((torch.stack(losses), tr.opt.flat.detach().clone()))
    assert torch.isfinite(res[0][0]).all()
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


def test_from_collated_equals_from_data_list(cuda):
    import x2gnn
    from x2gnn import datasets as xds
    from x2gnn.data import Batch

    cds = xds.CollatedDataset.load(os.path.join(GOLDEN, "pyg_inmemory_v21.pt"))
    with pytest.raises(ValueError, match="prepare_target"):
        x2gnn.DeviceDataset.from_collated(cds, cuda)  # y is still [M, 12]
    xds.prepare_target(cds, 7)
    ds = x2gnn.DeviceDataset.from_collated(cds, cuda)
    assert len(ds) == len(cds) == 3
    for idx in ([0, 1, 2], [2, 0], [1, 1]):
        ref = Batch.from_data_list([cds[i] for i in idx]).to(cuda)
        got = ds.batch(idx)
        for k in ("x", "edge_index", "edge_attr", "atom_pos", "edge_num", "batch", "ptr", "y"):
            g, r = got._store[k], ref._store[k]
            assert g.dtype == r.dtype and g.shape == r.shape and torch.equal(g, r), k
        assert got.num_graphs == ref.num_graphs
        np.testing.assert_array_equal(got.host_meta()["triplets"], ref.host_meta()["triplets"])


def test_shard_batch_equals_collate_shard(cuda, monkeypatch, dataset, mols):
    from x2gnn import data as xdata
    from x2gnn import dist as xdist

    monkeypatch.setattr(xdata, "HOST_SCHEDULE", False)
    idx = [5, 6, 0, 7, 9, 2, 8]
    sizes = []
    for rank in range(2):
        ref, local_r, global_r = xdist.collate_shard([mols[i] for i in idx], 2, rank)
        got, local_g, global_g = dataset.shard_batch(idx, 2, rank)
        assert (local_g, global_g) == (local_r, global_r) and global_g == len(idx)
        assert_same_batch(got, ref.to(cuda))
        assert got._store["_x2g_count_z"].numel() == sum(len(mols[i]["x"]) for i in idx)
        sizes.append(local_g)
    assert sum(sizes) == len(idx) and min(sizes) > 0


def test_batch_and_forward_capture_in_a_graph(cuda, monkeypatch, dataset, mols):
    """batch() reads nothing back from the device: it and a forward record into a HIP graph (a device->host read
    is illegal under capture), as train.Inference.capture records a forward; the replay equals the eager result."""
    import x2gnn

    idx = [3, 9, 1, 4]
    torch.manual_seed(0)
    model = x2gnn.xgnn_poly(device="cuda", **CFG).to(cuda).eval()

    def run():
        with torch.no_grad():
            return model(dataset.batch(idx)).sum()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            eager = run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(eager) and torch.equal(out, eager)
    with torch.no_grad():
        assert torch.equal(model(collated(mols, idx, cuda, monkeypatch)).sum(), eager)
