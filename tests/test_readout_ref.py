"""The fp64 reference of the rbf gate / pool, the readout heads and the loss (tests/readout_ref.py) made
trustworthy on the CPU: equal to the oracle's operations (oracle/ref_cpu.py) and to torch's smooth_l1_loss, every
hand-written backward equal to torch.autograd on the forward, the numpy-float32 emulation inside every bound with
the margin the constants K were fixed for, and the bound narrow enough to catch each of a list of wrong variants."""
import numpy as np
import pytest
import torch

import readout_ref as rr

from oracle import ref_cpu

D64 = torch.float64


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if b.size else 0.0


def _small(D=64, R=6, tile=None, jobs=1):
    rp = rr.ragged_rowptr(tile or rr.pool_tile(D))
    i = rr.gate_inputs(D, R, int(rp[-1]), len(rp) - 1, jobs=jobs)
    return rp, i, i["jobs"][0]


# ------------------------------------------------------------------------------ the reference is the oracle's
@pytest.mark.parametrize("D,R", [(64, 6), (128, 1), (256, 8)])
def test_gate_and_pool_equal_the_oracle(D, R):
    """pool == AtomWise.pool (scatter_sum(lin_rbf(rbf) * x, ei0, n)) in float64 with the owner index of a
    shuffled-then-sorted edge list; gate == the x * lin_rbf(rbf) line of SBFTransformerConv.forward (no bias)."""
    rp, i, j = _small(D, R)
    n = len(rp) - 1
    aw = ref_cpu.AtomWise(D, R).double()
    with torch.no_grad():
        aw.lin_rbf.weight.copy_(_t(j["w"]))
        aw.lin_rbf.bias.copy_(_t(j["b"]))
    ei0 = rr.owner_of(rp)
    perm = np.random.default_rng(3).permutation(ei0.shape[0])
    ei0_sorted = np.sort(ei0[perm], kind="stable")  # the dataset's order: any edge list, sorted by atom
    assert np.array_equal(ei0_sorted, ei0)
    with torch.no_grad():
        theirs = aw.pool(_t(j["x"]), _t(i["rbf"]), n, torch.from_numpy(ei0_sorted)).numpy()
    assert _rel(rr.pool(j["x"], i["rbf"], j["w"], j["b"], rp)[0], theirs) < 1e-12
    conv = ref_cpu.SBFTransformerConv(D, 16, 42, R, D).double()
    with torch.no_grad():
        conv.lin_rbf.weight.copy_(_t(j["w"]))
        theirs = (_t(j["x"]) * conv.lin_rbf(_t(i["rbf"]))).numpy()
    assert _rel(rr.gate(j["x"], i["rbf"], j["w"], None)[0], theirs) < 1e-12


@pytest.mark.parametrize("D,G", [(4, 1), (128, 3), (256, 8)])
def test_heads_equal_the_oracle(D, G):
    """heads == the sum of the last Linear(D, 1) layers of the oracle's readout MLPs (a group without a bias: 0)."""
    rp = rr.ragged_rowptr(rr.head_tile(D), big=300)
    i = rr.head_inputs(D, G, int(rp[-1]))
    total = 0.0
    for h, w, b in zip(i["hs"], i["ws"], i["bs"]):
        last = ref_cpu.AtomWise(D, 6).double().mlp[-1]
        with torch.no_grad():
            last.weight.copy_(_t(w)[None, :])
            last.bias.fill_(0.0 if b is None else b)
            total = total + last(_t(h))
    assert _rel(rr.heads(i["hs"], i["ws"], i["bs"])[0], total.view(-1).numpy()) < 1e-12
    pooled = ref_cpu.scatter_sum(total, torch.from_numpy(rr.owner_of(rp)), len(rp) - 1).view(-1).numpy()
    assert _rel(rr.heads_pool(i["hs"], i["ws"], i["bs"], rp)[0], pooled) < 1e-12


@pytest.mark.parametrize("n", [1, 3, 257, 1000])
@pytest.mark.parametrize("beta", rr.LOSS_BETA)
def test_loss_equals_torch(n, beta):
    """smooth_l1_mean == torch.nn.functional.smooth_l1_loss in float64, in value and in gradient (x gout)."""
    p, t = rr.loss_inputs(n, beta)
    pt = _t(p).requires_grad_()
    loss = torch.nn.functional.smooth_l1_loss(pt, _t(t), beta=beta)
    for gout in rr.LOSS_GOUT:
        (l, _), (dp, _) = rr.smooth_l1_mean(p, t, beta, gout)
        g, = torch.autograd.grad(loss, pt, torch.tensor(float(np.float32(gout)), dtype=D64), retain_graph=True)
        assert abs(l - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
        assert _rel(dp, g.numpy()) < 1e-12


# ------------------------------------------------------------------------------ backwards against autograd
@pytest.mark.parametrize("mode", ["gate", "pool"])
@pytest.mark.parametrize("D,R", [(64, 3), (128, 8)])
def test_gate_bwd_equals_autograd(D, R, mode):
    rp, i, j = _small(D, R)
    owner = rr.owner_of(rp) if mode == "pool" else None
    if mode == "gate":
        j = dict(j, g=rr.gate_inputs(D, R, int(rp[-1]))["jobs"][0]["g"])
    x, rbf, w, b = (_t(a).requires_grad_() for a in (j["x"], i["rbf"], j["w"], j["b"]))
    out = x * (rbf @ w.T + b)
    if owner is not None:
        out = ref_cpu.scatter_sum(out, torch.from_numpy(owner), len(rp) - 1)
    dx, drbf, dw, db = torch.autograd.grad((out * _t(j["g"])).sum(), (x, rbf, w, b))
    ours = rr.gate_bwd(j["g"], owner, j["x"], i["rbf"], j["w"], j["b"], j["dx_add"], i["drbf_old"])
    assert _rel(ours["dx"][0], (dx + _t(j["dx_add"])).numpy()) < 1e-12
    assert _rel(ours["drbf"][0], (drbf + _t(i["drbf_old"])).numpy()) < 1e-12
    assert _rel(ours["dw"][0], dw.numpy()) < 1e-12
    assert _rel(ours["db"][0], db.numpy()) < 1e-12
    plain = rr.gate_bwd(j["g"], owner, j["x"], i["rbf"], j["w"], j["b"])
    assert _rel(plain["dx"][0], dx.numpy()) < 1e-12 and _rel(plain["drbf"][0], drbf.numpy()) < 1e-12
    # the batch form: drbf summed over the jobs
    jobs = rr.gate_inputs(D, R, int(rp[-1]), None if owner is None else len(rp) - 1, jobs=3)["jobs"]
    outs, (dr, _) = rr.gate_bwd_batch(jobs, owner, i["rbf"], i["drbf_old"])
    want = sum(rr.gate_bwd(q["g"], owner, q["x"], i["rbf"], q["w"], q["b"])["drbf"][0] for q in jobs)
    assert _rel(dr, want + i["drbf_old"].astype(np.float64)) < 1e-12 and len(outs) == 3


@pytest.mark.parametrize("per_segment", [False, True])
@pytest.mark.parametrize("D,G", [(8, 3), (128, 8)])
def test_heads_bwd_equals_autograd(D, G, per_segment):
    rp = rr.ragged_rowptr(rr.head_tile(D), big=300)
    i = rr.head_inputs(D, G, int(rp[-1]), len(rp) - 1 if per_segment else None)
    hs, ws = [_t(h).requires_grad_() for h in i["hs"]], [_t(w).requires_grad_() for w in i["ws"]]
    bs = [torch.tensor(0.0 if b is None else b, dtype=D64).requires_grad_() for b in i["bs"]]
    out = sum(h @ w + b for h, w, b in zip(hs, ws, bs))
    if per_segment:
        out = ref_cpu.scatter_sum(out, torch.from_numpy(rr.owner_of(rp)), len(rp) - 1)
    grads = torch.autograd.grad((out * _t(i["dout"])).sum(), hs + ws + bs)
    ours = rr.heads_bwd(i["dout"], i["hs"], i["ws"], rp if per_segment else None)
    for g in range(G):
        assert _rel(ours[g]["dh"][0], grads[g].numpy()) < 1e-12
        assert _rel(ours[g]["dw"][0], grads[G + g].numpy()) < 1e-12
        assert _rel(ours[g]["db"][0], grads[2 * G + g].numpy()) < 1e-12


# ------------------------------------------------------------------------------ the emulation and the constants
def test_emulation_stays_inside_the_bounds():
    """Per family the float32 emulation's worst error / (2^-24 unit) over the GPU test's shapes is at most
    EMULATION_RATIO (the figure in readout_ref's docstring), K is a power of two, at least 4x that figure and less
    than 8x it (the smallest such power)."""
    rep = rr.emulation_report()
    print("worst |emulation - ref64| / (2^-24 unit):", {k: (round(v[0], 3),) + v[1:] for k, v in rep.items()})
    assert set(rep) == set(rr.EMULATION_RATIO) == set(rr.K)
    for fam, (ratio, output, case) in rep.items():
        assert ratio <= rr.EMULATION_RATIO[fam], (fam, ratio, output, case)
        assert ratio <= rr.K[fam] / 4
        k = rr.K[fam]
        assert k == 2.0 ** round(np.log2(k)) and 4 * ratio <= k < 8 * ratio, (fam, k, ratio)


# ------------------------------------------------------------------------------ the bound has teeth
def _outside(fam, got, ref_unit):
    return rr._ratio(got, *ref_unit) > rr.K[fam]


def _perturbed(fam, ref_unit):
    """The reference itself off by 1e-5 relative: outside the bound on at least one element."""
    return _outside(fam, np.asarray(ref_unit[0]) * (1.0 + 1e-5), ref_unit)


def test_wrong_pool_variants_leave_the_bound():
    D, R = 64, 6
    rp, i, j = _small(D, R)
    ref = rr.pool(j["x"], i["rbf"], j["w"], j["b"], rp)
    assert rr._ratio(ref[0], *ref) == 0.0 and _perturbed("gate_fwd", ref)
    # the last row of one segment dropped (the 400-row segment: the smallest share of a sum)
    seg = int(np.argmax(np.diff(rp)))
    keep = np.ones(int(rp[-1]), bool)
    keep[rp[seg + 1] - 1] = False
    v = rr.gate(j["x"], i["rbf"], j["w"], j["b"])[0] * keep[:, None]
    assert _outside("gate_fwd", rr.seg_sum(v, rp), ref)
    # w read as [R, D]; the bias left out
    gref = rr.gate(j["x"], i["rbf"], j["w"], j["b"])
    assert _perturbed("gate_fwd", gref)
    assert _outside("gate_fwd", rr.gate(j["x"], i["rbf"], j["w"].reshape(R, D).T, j["b"])[0], gref)
    assert _outside("gate_fwd", rr.gate(j["x"], i["rbf"], j["w"], None)[0], gref)
    assert _outside("gate_fwd", rr.pool(j["x"], i["rbf"], j["w"], None, rp)[0], ref)


def test_wrong_gate_bwd_variants_leave_the_bound():
    D, R = 64, 6
    # g[e] instead of g[owner[e]]: the smallest ragged segments in which every row index is a segment index too
    rp = np.array([0, 0, 1, 3, 3, 4], np.int32)
    i = rr.gate_inputs(D, R, 4, 5)
    j = i["jobs"][0]
    owner = rr.owner_of(rp)
    ref = rr.gate_bwd(j["g"], owner, j["x"], i["rbf"], j["w"], j["b"], j["dx_add"], i["drbf_old"])
    wrong = rr.gate_bwd(j["g"], np.arange(4), j["x"], i["rbf"], j["w"], j["b"], j["dx_add"], i["drbf_old"])
    for k in ref:
        assert _outside("gate_bwd", wrong[k][0], ref[k]), k
        assert _perturbed("gate_bwd", ref[k]), k
    # the old contents forgotten under X2G_GATE_DRBF_ACCUM; dx_add forgotten
    plain = rr.gate_bwd(j["g"], owner, j["x"], i["rbf"], j["w"], j["b"])
    assert _outside("gate_bwd", plain["drbf"][0], ref["drbf"]) and _outside("gate_bwd", plain["dx"][0], ref["dx"])
    # w read as [R, D] and the bias left out (dx), at one row
    assert _outside("gate_bwd", rr.gate_bwd(j["g"], owner, j["x"], i["rbf"], j["w"].reshape(R, D).T, j["b"],
                                            j["dx_add"])["dx"][0], ref["dx"])
    assert _outside("gate_bwd", rr.gate_bwd(j["g"], owner, j["x"], i["rbf"], j["w"], None, j["dx_add"])["dx"][0],
                    ref["dx"])
    # one of the 128 splits' slabs left out of dw / db: 1025 rows, 9 per split (the smallest row count with 128)
    rows, per = 1025, 9
    i = rr.gate_inputs(D, R, rows)
    j = i["jobs"][0]
    ref = rr.gate_bwd(j["g"], None, j["x"], i["rbf"], j["w"], j["b"])
    for split in (0, 57, 113):  # (113: the last one that owns rows, 8 of them)
        keep = np.ones(rows, bool)
        keep[split * per:(split + 1) * per] = False
        wrong = rr.gate_bwd(j["g"][keep], None, j["x"][keep], i["rbf"][keep], j["w"], j["b"])
        assert _outside("gate_bwd", wrong["dw"][0], ref["dw"]) and _outside("gate_bwd", wrong["db"][0], ref["db"])
    # the smallest case with more than one slab: 9 rows, 2 splits of 5 and 4 (there the 1e-5 perturbation too; over
    # 1025 random rows a sum is ~ 1 / 32 of its unit, and 1e-5 of it is inside any float32 bound)
    rows, per = 9, 5
    i = rr.gate_inputs(D, R, rows)
    j = i["jobs"][0]
    ref = rr.gate_bwd(j["g"], None, j["x"], i["rbf"], j["w"], j["b"])
    for keep in (slice(0, per), slice(per, rows)):
        wrong = rr.gate_bwd(j["g"][keep], None, j["x"][keep], i["rbf"][keep], j["w"], j["b"])
        assert _outside("gate_bwd", wrong["dw"][0], ref["dw"]) and _outside("gate_bwd", wrong["db"][0], ref["db"])
    assert _perturbed("gate_bwd", ref["dw"]) and _perturbed("gate_bwd", ref["db"])


def test_wrong_head_variants_leave_the_bound():
    D, G = 4, 3
    rp = rr.ragged_rowptr(rr.head_tile(D), big=300)
    i = rr.head_inputs(D, G, int(rp[-1]), len(rp) - 1)
    assert sum(b is not None for b in i["bs"]) >= 2
    ref, pref = rr.heads(i["hs"], i["ws"], i["bs"]), rr.heads_pool(i["hs"], i["ws"], i["bs"], rp)
    assert _perturbed("heads", ref) and _perturbed("heads", pref)
    for g in range(G):  # one group's bias omitted
        if i["bs"][g] is not None:
            bs = [None if k == g else b for k, b in enumerate(i["bs"])]
            assert _outside("heads", rr.heads(i["hs"], i["ws"], bs)[0], ref)
            assert _outside("heads", rr.heads_pool(i["hs"], i["ws"], bs, rp)[0], pref)
    # the last row of the 300-row segment dropped
    seg = int(np.argmax(np.diff(rp)))
    keep = np.ones(int(rp[-1]))
    keep[rp[seg + 1] - 1] = 0.0
    assert _outside("heads", rr.seg_sum(ref[0] * keep, rp), pref)
    # an empty segment's dout put on the next segment's rows (segments numbered without the empty ones)
    # (the smallest ragged rowptr with empty segments first, in the middle and last: 4 rows in 6 segments)
    rp = np.array([0, 0, 1, 3, 3, 4, 4], np.int32)
    i = rr.head_inputs(D, G, 4, 6)
    bref = rr.heads_bwd(i["dout"], i["hs"], i["ws"], rp)
    lens = np.diff(rp)
    shifted = np.repeat(np.arange(int((lens > 0).sum())), lens[lens > 0])
    assert not np.array_equal(shifted, rr.owner_of(rp))
    wrong = rr.heads_bwd(i["dout"][shifted], i["hs"], i["ws"])
    for g in range(G):
        for k in ("dh", "dw", "db"):
            assert _outside("heads", wrong[g][k][0], bref[g][k]), (g, k)
            assert _perturbed("heads", bref[g][k]), (g, k)
    # one of the 256 splits' slabs left out of dw / db: 8193 rows, 33 per split
    rows, per = 8193, 33
    i = rr.head_inputs(D, 1, rows)
    bref = rr.heads_bwd(i["dout"], i["hs"], i["ws"])[0]
    keep = np.ones(rows, bool)
    keep[248 * per:] = False  # (the last split that owns rows: 9 of them)
    wrong = rr.heads_bwd(i["dout"][keep], [i["hs"][0][keep]], i["ws"])[0]
    assert _outside("heads", wrong["dw"][0], bref["dw"]) and _outside("heads", wrong["db"][0], bref["db"])
    # the smallest case with two slabs (D = 128: 1e-5 of a value shows where |value| > K 2^-24 1e5 = 0.19 unit, and
    # one of 128 sums of 33 random terms is that little cancelled, one of 4 need not be)
    rows, per = 33, 17
    i = rr.head_inputs(128, 1, rows)
    bref = rr.heads_bwd(i["dout"], i["hs"], i["ws"])[0]
    for keep in (slice(0, per), slice(per, rows)):
        wrong = rr.heads_bwd(i["dout"][keep], [i["hs"][0][keep]], i["ws"])[0]
        assert _outside("heads", wrong["dw"][0], bref["dw"]) and _outside("heads", wrong["db"][0], bref["db"])
    assert _perturbed("heads", bref["dw"])
    i = rr.head_inputs(128, 1, 1)  # (db is one sum per group: its perturbation at one row, where nothing cancels)
    assert _perturbed("heads", rr.heads_bwd(i["dout"], i["hs"], i["ws"])[0]["db"])


@pytest.mark.parametrize("beta", [0.5, 2.0])
def test_wrong_loss_variant_leaves_the_bound(beta):
    """|d| <= beta with the linear branch's gradient scaled by beta (right only at beta = 1), at the smallest n of
    the GPU test that holds an element with |d| > beta; and the 1e-5 perturbation at every n."""
    n = 255
    p, t = rr.loss_inputs(n, beta)
    assert (np.abs(p.astype(np.float64) - t) > beta).any()
    (_, _), dref = rr.smooth_l1_mean(p, t, beta, 1.0)
    d = p.astype(np.float64) - t
    wrong = np.where(np.abs(d) <= beta, d / beta, np.sign(d) * beta) / n
    assert _outside("loss", wrong, dref)
    for n in rr.LOSS_N:
        p, t = rr.loss_inputs(n, beta)
        lref, dref = rr.smooth_l1_mean(p, t, beta, -0.37)
        assert _perturbed("loss", lref) and _perturbed("loss", dref), n  # (n = 1 sits on d = +beta)
