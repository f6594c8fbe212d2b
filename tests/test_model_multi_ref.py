"""The oracle with K-wide readouts (oracle.ref_cpu.XGNN, each readout's last Linear widened in the test) pinned to
the reference's own K = 3 run (tests/golden/model_multi.npz, written by make_multi_golden.py), at
tests/test_oracle.py's tolerances; and the host-side shapes of the multi-target path."""
import numpy as np
import pytest
import torch

from helpers import rel_err
from model_multi_cases import MODELS, batch_k, fixture, oracle_of, small_batch

from oracle import ref_cpu


@pytest.mark.parametrize("model", MODELS)
def test_widened_oracle_vs_reference(model):
    z = fixture(model)
    m = oracle_of(z)
    b = batch_k(z)
    res = ref_cpu.run_batch(m, b)
    assert res.shape == z["energies"].shape == (b.y.numel(),)
    assert rel_err(res.detach().numpy(), z["energies"]) < 1e-4
    loss = torch.nn.functional.smooth_l1_loss(res, b.y.view(-1))
    assert float(loss.detach()) == pytest.approx(float(z["loss"]), rel=1e-4)
    loss.backward()
    np.testing.assert_allclose(m.emb_block.embedding.weight.detach().numpy(), z["emb_after"], rtol=1e-6, atol=1e-7)
    scale = max(float(z["gnorm." + n]) for n, _ in m.named_parameters())
    checked = 0
    for n, p in m.named_parameters():
        ref_norm = float(z["gnorm." + n])
        got = 0.0 if p.grad is None else float(p.grad.double().norm())
        assert abs(got - ref_norm) <= 1e-3 * ref_norm + 1e-6 * scale, (n, got, ref_norm)
        if "grad." + n in z.files:
            ref = z["grad." + n]
            assert np.abs(p.grad.numpy() - ref).max() <= 2e-3 * np.abs(ref).max() + 1e-6 * scale, n
            checked += 1
    assert checked >= 5 and tuple(z["grad.fin_model.readouts.2.mlp.4.weight"].shape) == (3, 128)


def test_fixture_holds_data_only_and_stays_small():
    import os

    from conftest import GOLDEN

    path = os.path.join(GOLDEN, "model_multi.npz")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(GOLDEN, "model_small.npz"))
    z = np.load(path, allow_pickle=False)  # (no pickled objects: arrays alone)
    assert all(z[k].dtype.kind in "fiuU" for k in z.files)


def test_host_model_on_wide_labels_runs_on_the_cpu():
    """collate -> [B, K] labels; the K-target modules build and load on the host (the GPU tests run them)."""
    import x2gnn
    from x2gnn.data import collate

    b = collate(small_batch(3))
    assert tuple(b.y.shape) == (3, 3) and b.y.dtype == torch.float32
    assert tuple(collate(small_batch(1)).y.shape) == (3,)
    m = x2gnn.xgnn_poly(conv_layers=2, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128,
                        num_target=3)
    sd = m.state_dict()
    m2 = x2gnn.xgnn_poly(conv_layers=2, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128,
                         num_target=3)
    m2.load_state_dict(sd)
    assert all(torch.equal(a, c) for a, c in zip(m.state_dict().values(), m2.state_dict().values()))
