"""The fp64 statement of the K-target readout heads (tests/readout_multi_ref.py) made trustworthy on the CPU: equal
to a Linear(D, K) of torch and, at K = 1, to readout_ref's heads; its backward equal to torch.autograd; the
numpy-float32 emulation inside the bounds with the margin they were fixed for; the bounds narrow enough to catch
wrong variants.  And the host side of multi-target training: ``prepare_targets`` column by column against
``prepare_target``, ``collate`` with K-wide labels, the binding tables of include/x2g_multi.h, the models' shapes."""
import os

import numpy as np
import pytest
import torch

import readout_multi_ref as mr
import readout_ref as rr

from conftest import GOLDEN

D64 = torch.float64


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if b.size else 0.0


# ------------------------------------------------------------------------------ the statement
@pytest.mark.parametrize("D,K,G", [(4, 2, 1), (128, 12, 5), (256, 16, 8)])
def test_heads_k_equal_torch_linear(D, K, G):
    """heads_k == the sum of nn.Linear(D, K) layers in float64 (a group without a bias: 0), pooled == index_add."""
    rp = mr.seg_rowptr_for(D)
    i = mr.head_k_inputs(D, K, G, int(rp[-1]))
    total = 0.0
    for h, w, b in zip(i["hs"], i["ws"], i["bs"]):
        total = total + torch.nn.functional.linear(_t(h), _t(w), None if b is None else _t(b))
    assert _rel(mr.heads_k(i["hs"], i["ws"], i["bs"])[0], total.numpy()) < 1e-12
    pooled = torch.zeros(len(rp) - 1, K, dtype=D64).index_add_(0, torch.from_numpy(rr.owner_of(rp)), total)
    assert _rel(mr.heads_k_pool(i["hs"], i["ws"], i["bs"], rp)[0], pooled.numpy()) < 1e-12


def test_heads_k_at_one_target_is_readout_ref():
    """K = 1: value and unit of readout_ref.heads / heads_pool / heads_bwd, column 0."""
    D, G = 16, 3
    rp = mr.seg_rowptr_for(D)
    i = mr.head_k_inputs(D, 1, G, int(rp[-1]), len(rp) - 1)
    ws1 = [w[0] for w in i["ws"]]
    bs1 = [None if b is None else float(b[0]) for b in i["bs"]]
    for ours, theirs in ((mr.heads_k(i["hs"], i["ws"], i["bs"]), rr.heads(i["hs"], ws1, bs1)),
                         (mr.heads_k_pool(i["hs"], i["ws"], i["bs"], rp), rr.heads_pool(i["hs"], ws1, bs1, rp))):
        for a, b in zip(ours, theirs):
            np.testing.assert_allclose(a[:, 0], b, rtol=1e-15, atol=0)
    ours, theirs = mr.heads_k_bwd(i["dout"], i["hs"], i["ws"], rp), rr.heads_bwd(i["dout"][:, 0], i["hs"], ws1, rp)
    for g in range(G):
        for k in ("dh", "dw", "db"):
            for a, b in zip(ours[g][k], theirs[g][k]):
                np.testing.assert_allclose(np.asarray(a).reshape(np.shape(b)), b, rtol=1e-15, atol=0)


@pytest.mark.parametrize("per_segment", [False, True])
@pytest.mark.parametrize("D,K,G", [(8, 5, 3), (128, 12, 5)])
def test_heads_k_bwd_equals_autograd(D, K, G, per_segment):
    rp = mr.seg_rowptr_for(D)
    i = mr.head_k_inputs(D, K, G, int(rp[-1]), len(rp) - 1 if per_segment else None)
    hs, ws = [_t(h).requires_grad_() for h in i["hs"]], [_t(w).requires_grad_() for w in i["ws"]]
    bs = [torch.zeros(K, dtype=D64, requires_grad=True) if b is None else _t(b).requires_grad_() for b in i["bs"]]
    out = sum(h @ w.T + b for h, w, b in zip(hs, ws, bs))
    if per_segment:
        out = torch.zeros(len(rp) - 1, K, dtype=D64).index_add_(0, torch.from_numpy(rr.owner_of(rp)), out)
    grads = torch.autograd.grad((out * _t(i["dout"])).sum(), hs + ws + bs)
    ours = mr.heads_k_bwd(i["dout"], i["hs"], i["ws"], rp if per_segment else None)
    for g in range(G):
        assert _rel(ours[g]["dh"][0], grads[g].numpy()) < 1e-12
        assert _rel(ours[g]["dw"][0], grads[G + g].numpy()) < 1e-12
        assert _rel(ours[g]["db"][0], grads[2 * G + g].numpy()) < 1e-12


def test_error_cols_known_answer():
    pred = np.array([[1.0, -2.0], [3.5, 0.25], [0.0, 0.25]], np.float32)
    target = np.array([[0.5, 2.0], [3.5, 0.0], [-2.0, 0.25]], np.float32)
    np.testing.assert_array_equal(mr.error_cols(pred, target),
                                  np.array([[2.5, 4.25, 2.0, 3.0], [4.25, 16.0625, 4.0, 3.0]]))


# ------------------------------------------------------------------------------ the emulation and the constants
def test_emulation_stays_inside_the_bounds():
    """Per family the float32 emulation's worst error / (2^-24 unit) over the GPU test's shapes is at most
    EMULATION_RATIO (the figure in the module's docstring); K_BOUND is a power of two, at least 4x that figure and
    less than 8x it (the smallest such power)."""
    rep = mr.emulation_report()
    print("worst |emulation - ref64| / (2^-24 unit):", {k: (round(v[0], 3),) + v[1:] for k, v in rep.items()})
    assert set(rep) == set(mr.EMULATION_RATIO) == set(mr.K_BOUND)
    for fam, (ratio, output, case) in rep.items():
        assert ratio <= mr.EMULATION_RATIO[fam], (fam, ratio, output, case)
        k = mr.K_BOUND[fam]
        assert 4 * mr.EMULATION_RATIO[fam] <= k
        assert k == 2.0 ** round(np.log2(k)) and 4 * ratio <= k < 8 * ratio, (fam, k, ratio)


def test_case_lists_cover_what_the_issue_names():
    cases = mr.fwd_cases() + [(D, K, G, 0, "") for D, K, G in mr.pool_cases()] + \
        [c + ("",) for c in mr.bwd_cases()] + [(D, K, G, 0, "") for D, K, G, _ in mr.bwd_seg_cases()]
    assert {c[1] for c in cases} == set(mr.KS) == {1, 2, 5, 12, 16}
    assert {c[0] for c in cases} == set(mr.DS) == {4, 16, 128, 256}
    assert {c[2] for c in cases} == set(mr.GS) == {1, 5, 8}
    assert {c[3] for c in mr.bwd_cases()} == set(rr.HEAD_BWD_ROWS)
    for D in mr.DS:  # every target count at every width, forward and pooled
        assert {K for d, K, _, _, _ in mr.fwd_cases() if d == D} == set(mr.KS)
        assert {K for d, K, _ in mr.pool_cases() if d == D} == set(mr.KS)
        lens = np.diff(mr.seg_rowptr_for(D))
        assert (lens == 0).any() and (lens == 300).any()


# ------------------------------------------------------------------------------ the bounds have teeth
def _outside(fam, got, ref_unit):
    return rr._ratio(got, *ref_unit) > mr.K_BOUND[fam]


def test_wrong_variants_leave_the_bound():
    D, K, G = 16, 5, 3
    rp = mr.seg_rowptr_for(D)
    i = mr.head_k_inputs(D, K, G, int(rp[-1]), len(rp) - 1)
    ref, pref = mr.heads_k(i["hs"], i["ws"], i["bs"]), mr.heads_k_pool(i["hs"], i["ws"], i["bs"], rp)
    assert rr._ratio(ref[0], *ref) == 0.0
    assert _outside("heads_k", ref[0] * (1 + 1e-5), ref) and _outside("heads_k", pref[0] * (1 + 1e-5), pref)
    # the weight read as [D, K]; targets swapped; one group's bias taken from target 0 for every target
    wt = [w.reshape(D, K).T for w in i["ws"]]
    assert _outside("heads_k", mr.heads_k(i["hs"], wt, i["bs"])[0], ref)
    assert _outside("heads_k", ref[0][:, ::-1], ref)
    b0 = [None if b is None else np.full(K, b[0], np.float32) for b in i["bs"]]
    assert _outside("heads_k", mr.heads_k(i["hs"], i["ws"], b0)[0], ref)
    # the last row of the 300-row segment dropped from the pooled sum
    seg = int(np.argmax(np.diff(rp)))
    keep = np.ones(int(rp[-1]))
    keep[rp[seg + 1] - 1] = 0.0
    assert _outside("heads_k", rr.seg_sum(ref[0] * keep[:, None], rp), pref)
    # the backward from per-segment dout: an empty segment's dout put on the next segment's rows
    rp2 = np.array([0, 0, 1, 3, 3, 4, 4], np.int32)
    i2 = mr.head_k_inputs(D, K, G, 4, 6)
    bref = mr.heads_k_bwd(i2["dout"], i2["hs"], i2["ws"], rp2)
    lens = np.diff(rp2)
    shifted = np.repeat(np.arange(int((lens > 0).sum())), lens[lens > 0])
    wrong = mr.heads_k_bwd(i2["dout"][shifted], i2["hs"], i2["ws"])
    for g in range(G):
        assert _outside("heads_k", wrong[g]["dh"][0], bref[g]["dh"])
        assert _outside("heads_k_seg", wrong[g]["dw"][0], bref[g]["dw"])
        assert _outside("heads_k_seg", wrong[g]["db"][0], bref[g]["db"])
    # one of the 256 splits' slabs left out of dw / db at 8193 rows (33 per split), per row and per segment
    rows, per = 8193, 33
    for fam, rp3 in (("heads_k", None), ("heads_k_seg", mr.seg_rowptr_for(D, rows))):
        i3 = mr.head_k_inputs(D, K, 1, rows, None if rp3 is None else len(rp3) - 1)
        d = i3["dout"] if rp3 is None else i3["dout"][rr.owner_of(rp3)]
        bref = mr.heads_k_bwd(d, i3["hs"], i3["ws"])[0]
        keep = np.ones(rows, bool)
        keep[248 * per:] = False  # (the last split that owns rows: 9 of them)
        wrong = mr.heads_k_bwd(d[keep], [i3["hs"][0][keep]], i3["ws"])[0]
        assert _outside(fam, wrong["dw"][0], bref["dw"]) and _outside(fam, wrong["db"][0], bref["db"])


# ------------------------------------------------------------------------------ data
def test_prepare_targets_columns_equal_prepare_target():
    from x2gnn import datasets as ds

    path = os.path.join(GOLDEN, "pyg_inmemory_v21.pt")
    targets = list(range(12))
    raw = ds.CollatedDataset.load(path)
    scales = ds.prepare_targets(raw, targets, standardize=False)
    std = ds.CollatedDataset.load(path)
    scales_std = ds.prepare_targets(std, targets, standardize=True)
    assert raw.data.y.shape == std.data.y.shape == (len(raw), 12)
    for k, t in enumerate(targets):
        one = ds.CollatedDataset.load(path)
        calib = ds.prepare_target(one, t)
        assert torch.equal(raw.data.y[:, k], one.data.y)  # the same arithmetic: the same bits
        assert scales[k] == calib
        y64 = one.data.y.double().numpy()
        sd = float(np.sqrt(np.mean((y64 - y64.mean()) ** 2)))
        assert scales_std[k] == pytest.approx(sd * calib, rel=1e-12)
        np.testing.assert_allclose(std.data.y[:, k].double().numpy() * sd, y64, rtol=2e-7)
    # a subset, in another order
    sub = ds.CollatedDataset.load(path)
    ds.prepare_targets(sub, [7, 0], standardize=False)
    assert torch.equal(sub.data.y, raw.data.y[:, [7, 0]])


def test_prepare_targets_standard_deviation_known_answer():
    """Targets 0 and 1 take no atom reference and no conversion.  The dataset's three molecules given y = 1, 3, 8:
    mean 4, population variance (9 + 1 + 16) / 3, standard deviation sqrt(26 / 3); a column three times as large has
    three times that, and both standardise to the same values."""
    from x2gnn import datasets as ds

    data = ds.CollatedDataset.load(os.path.join(GOLDEN, "pyg_inmemory_v21.pt"))
    assert len(data) == 3
    y = torch.zeros(3, 12, dtype=data.data.y.dtype)
    y[:, 0] = torch.tensor([1.0, 3.0, 8.0])
    y[:, 1] = 3 * y[:, 0]
    data.data.y = y
    scales = ds.prepare_targets(data, [0, 1], standardize=True)
    want = (26.0 / 3.0) ** 0.5
    assert scales[0] == pytest.approx(want, rel=1e-15) and scales[1] == pytest.approx(3 * want, rel=1e-15)
    np.testing.assert_allclose(data.data.y[:, 0].numpy(), np.array([1.0, 3.0, 8.0]) / want, rtol=1e-6)
    np.testing.assert_allclose(data.data.y[:, 1].numpy(), data.data.y[:, 0].numpy(), rtol=1e-6)


def test_collate_with_wide_targets():
    from device_dataset_cases import mixed_molecules
    from x2gnn.data import Batch, collate, molecule_to_data

    mols = mixed_molecules()
    ys = np.random.default_rng(0).standard_normal((len(mols), 3)).astype(np.float32)
    wide = [dict(m, y=ys[i]) for i, m in enumerate(mols)]
    b = collate(wide)
    assert b.y.dtype == torch.float32 and tuple(b.y.shape) == (len(mols), 3)
    np.testing.assert_array_equal(b.y.numpy(), ys)
    ref = Batch.from_data_list([molecule_to_data(m) for m in wide])
    assert torch.equal(ref.y, b.y)
    # scalars still collate to [B], bit for bit what float(y) gave
    narrow = [dict(m, y=float(ys[i, 0])) for i, m in enumerate(mols)]
    assert torch.equal(collate(narrow).y, torch.from_numpy(ys[:, 0].copy()))
    assert tuple(collate([{k: v for k, v in m.items() if k != "y"} for m in mols]).y.shape) == (len(mols),)
    with pytest.raises(ValueError):
        collate([wide[0], dict(wide[1], y=ys[1, :2])])


# ------------------------------------------------------------------------------ the binding tables
def test_multi_binding_tables():
    from x2gnn import _lib

    with open(_lib.MULTI_HEADER_PATH) as f:
        sig, res, structs, consts = _lib.parse_header(f.read())
    assert not structs and not consts
    assert _lib.MULTI_SIGNATURES == sig and _lib.MULTI_RESTYPES == res
    assert set(sig) == {"x2g_readout_heads_k_max_targets", "x2g_readout_heads_k_fwd", "x2g_readout_heads_k_bwd",
                        "x2g_readout_heads_k_bwd_workspace", "x2g_readout_heads_k_bwd_splits", "x2g_error_accum_cols"}
    assert not set(sig) & set(_lib.SIGNATURES) and not set(sig) & set(_lib.STAGED_SIGNATURES)
    with open(_lib.HEADER_PATH) as f:
        assert _lib.parse_header(f.read())[0] == _lib.SIGNATURES
    with open(_lib.STAGED_HEADER_PATH) as f:
        assert _lib.parse_header(f.read())[0] == _lib.STAGED_SIGNATURES
    import ctypes

    assert len(sig["x2g_readout_heads_k_fwd"]) == 11 and len(sig["x2g_readout_heads_k_bwd"]) == 16
    assert sig["x2g_readout_heads_k_fwd"][0] is ctypes.c_void_p and res["x2g_readout_heads_k_bwd_workspace"] is ctypes.c_size_t


# ------------------------------------------------------------------------------ the models on the host
CFG = dict(conv_layers=1, sbf_dim=7, rbf_dim=6, in_channels=16, heads=2, embedding_size=16)


def test_models_carry_num_target_and_the_reference_keys():
    import x2gnn

    one = x2gnn.xgnn_poly(**CFG)
    three = x2gnn.xgnn_poly(num_target=3, **CFG)
    assert one.num_target == 1 and three.num_target == three.fin_model.num_target == 3
    assert list(one.state_dict()) == list(three.state_dict())
    assert tuple(three.state_dict()["fin_model.readouts.1.mlp.4.weight"].shape) == (3, 16)
    assert tuple(three.state_dict()["fin_model.readouts.1.mlp.4.bias"].shape) == (3,)
    g = x2gnn.xgnn_poly_global(num_target=2, pool_option="add", **CFG)
    assert g.num_target == 2 and tuple(g.state_dict()["fin_model.readouts.0.mlp.4.weight"].shape) == (2, 16)
    m = x2gnn.xgnn_poly_multi(atom_targets=2, mol_targets=3, **CFG)
    assert m.num_target == 5 and isinstance(m.fin_model, x2gnn.SBFTransformerMulti)
    sd = m.state_dict()
    assert tuple(sd["fin_model.readouts.0.mlp.4.weight"].shape) == (2, 16)
    assert tuple(sd["fin_model.mol_readouts.0.mlp.4.weight"].shape) == (3, 16)
    only_atoms = x2gnn.xgnn_poly_multi(atom_targets=2, mol_targets=0, **CFG)
    assert not any(k.startswith("fin_model.mol_readouts") for k in only_atoms.state_dict())
    only_mols = x2gnn.xgnn_poly_multi(atom_targets=0, mol_targets=1, **CFG)
    assert not any(k.startswith("fin_model.readouts") for k in only_mols.state_dict())
    for bad in (dict(atom_targets=0, mol_targets=0), dict(atom_targets=17, mol_targets=1)):
        with pytest.raises(ValueError):
            x2gnn.xgnn_poly_multi(**bad, **CFG)
    with pytest.raises(ValueError):
        x2gnn.xgnn_poly(num_target=0, **CFG)
