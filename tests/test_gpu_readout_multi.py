"""The K-target readout heads and the per-target error statistics (csrc/readout_multi.hip, include/x2g_multi.h)
through the raw ABI against the fp64 statement of tests/readout_multi_ref.py, element by element.

Bound (nothing taken from the code under test): every element finite and within K_BOUND[family] * 2^-24 * unit of
the fp64 value (readout_multi_ref: fixed against a numpy-float32 emulation on the CPU, asserted by
tests/test_readout_multi_ref.py); a zero unit requires an exact zero.  Shapes are that module's case lists: K in
1, 2, 5, 12, 16; D in 4, 16, 128, 256 (1, 4, 32, 64 lanes per row); 1, 5, 8 readouts; rows around a workgroup's
pass, past the grid cap, and readout_ref.HEAD_BWD_ROWS for the backward's split boundaries and empty workgroups;
readout_ref.ragged_rowptr segments (empty ones, one of 300 rows) for the pooled forms.  Every output buffer is
prefilled with NaN and carries a guard row that has to stay untouched; workspaces likewise."""
import ctypes

import numpy as np
import pytest
import torch

import readout_multi_ref as mr
import readout_ref as rr

pytestmark = pytest.mark.gpu

ACCUM, DEFER = 1, 2  # X2G_ACCUM_WGRAD, X2G_DEFER_SLAB_SUM
OK, EINVAL, EUNSUPPORTED = 0, 1001, 1002
WS_GUARD = 64
F = np.float32


def _dev(a, cuda):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _nan(cuda, *shape):
    return torch.full(shape, float("nan"), device=cuda, dtype=torch.float32)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


_NAN_BITS = int(_bits(torch.full((1,), float("nan"), dtype=torch.float32))[0])


def _untouched(t):
    return bool((_bits(t) == _NAN_BITS).all())


def _lib():
    from x2gnn import _lib as lib

    return lib


def _st():
    return _lib().stream_ptr()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _ptrs(ts, off=0):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() + off for t in ts])


class _Checker:
    """Compares the outputs of one case with the reference; collects every figure before failing."""

    def __init__(self, case):
        self.case, self.bad, self.worst = case, [], {}

    def check(self, fam, output, buf, rows, ref_unit):
        """``buf``: rows + 1 leading entries, the last one the guard; ``ref_unit``: float64 (value, unit)."""
        ref = np.asarray(ref_unit[0], np.float64).reshape(rows, -1)
        unit = np.asarray(ref_unit[1], np.float64).reshape(rows, -1)
        assert buf.shape[0] == rows + 1, (buf.shape, rows)
        if not _untouched(buf[rows:]):
            self.bad.append((output, "guard written"))
        got = buf[:rows].detach().cpu().double().numpy().reshape(rows, -1)
        assert got.shape == ref.shape, (got.shape, ref.shape)
        r = rr._ratio(got, ref, unit) / mr.K_BOUND[fam]
        self.worst[output] = max(self.worst.get(output, 0.0), r)
        if not r <= 1.0:
            self.bad.append((output, f"error / bound = {r}"))

    def same(self, what, a, b):
        if not torch.equal(_bits(a), _bits(b)):
            self.bad.append((what, "not bitwise equal"))

    def untouched(self, what, t):
        if not _untouched(t):
            self.bad.append((what, "written"))

    def status(self, what, rc, want):
        if rc != want:
            self.bad.append((what, f"status {rc}, expected {want}"))

    def done(self):
        print(self.case, "worst error / bound:", {k: round(v, 4) for k, v in self.worst.items()})
        assert not self.bad, self.case + "\n" + "\n".join(f"{what}: {why}" for what, why in self.bad)


def _tensors(cuda, i):
    return dict(hs=[_dev(h, cuda) for h in i["hs"]], ws=[_dev(w, cuda) for w in i["ws"]],
                bs=[_dev(b, cuda) for b in i["bs"]], dout=_dev(i["dout"], cuda),
                dw_old=[_dev(a, cuda) for a in i["dw_old"]], db_old=[_dev(a, cuda) for a in i["db_old"]])


def _plus(ref_unit, old):
    old = np.asarray(old, np.float64)
    return ref_unit[0] + old, ref_unit[1] + np.abs(old)


def _ids(cases, fmt):
    return [pytest.param(*c, id=fmt(*c)) for c in cases]


# ------------------------------------------------------------------------------ the library has the entries
def test_entries_are_bound(cuda):
    lib = _lib()
    so = lib.load()
    for name, args in lib.MULTI_SIGNATURES.items():
        fn = getattr(so, name)
        assert fn.argtypes == args and fn.restype is lib.MULTI_RESTYPES[name]
    assert so.x2g_readout_heads_k_max_targets() == 16
    assert so.x2g_abi_version() == 18


# ------------------------------------------------------------------------------ forward
def _fwd(cuda, t, G, rows, D, K, out, bias=True, rpd=None, n_seg=0):
    return _lib().load().x2g_readout_heads_k_fwd(_ptrs(t["hs"][:G]), _ptrs(t["ws"][:G]),
                                                 _ptrs(t["bs"][:G]) if bias else None, G, rows, D, K, _p(rpd), n_seg,
                                                 _p(out), _st())


@pytest.mark.parametrize("D,K,G,rows,why", _ids(mr.fwd_cases(), lambda D, K, G, r, w: f"D{D}-K{K}-G{G}-{w}-{r}"))
def test_heads_k_fwd(cuda, D, K, G, rows, why):
    """out[r, k] = sum_g (h_g[r] . w_g[k] + b_g[k]); every second case with every bias NULL as well; two runs equal."""
    i = mr.head_k_inputs(D, K, G, rows)
    t = _tensors(cuda, i)
    ck = _Checker(f"fwd D={D} K={K} G={G} rows={rows} {why}")
    out = _nan(cuda, rows + 1, K)
    ck.status("status", _fwd(cuda, t, G, rows, D, K, out), OK)
    ck.check("heads_k", "out", out, rows, mr.heads_k(i["hs"], i["ws"], i["bs"]))
    again = _nan(cuda, rows + 1, K)
    ck.status("status again", _fwd(cuda, t, G, rows, D, K, again), OK)
    ck.same("run to run", again, out)
    if (K + G) % 2:
        nb = _nan(cuda, rows + 1, K)
        ck.status("status b=NULL", _fwd(cuda, t, G, rows, D, K, nb, bias=False), OK)
        ck.check("heads_k", "out[b=NULL]", nb, rows, mr.heads_k(i["hs"], i["ws"], [None] * G))
    ck.done()


@pytest.mark.parametrize("D,K,G", _ids(mr.pool_cases(), lambda D, K, G: f"D{D}-K{K}-G{G}"))
def test_heads_k_pool_fwd(cuda, D, K, G):
    """The heads summed per segment over the ragged rowptr (empty segments first, in the middle and last, 1 row,
    around 4 RPW rows, 300 rows); 0 segments leave the output untouched."""
    rp = mr.seg_rowptr_for(D)
    rows, n_seg = int(rp[-1]), len(rp) - 1
    i = mr.head_k_inputs(D, K, G, rows)
    t = _tensors(cuda, i)
    rpd = _dev(rp, cuda)
    ck = _Checker(f"pool fwd D={D} K={K} G={G} rows={rows}")
    out = _nan(cuda, n_seg + 1, K)
    ck.status("status", _fwd(cuda, t, G, rows, D, K, out, rpd=rpd, n_seg=n_seg), OK)
    ck.check("heads_k", "out_seg", out, n_seg, mr.heads_k_pool(i["hs"], i["ws"], i["bs"], rp))
    again = _nan(cuda, n_seg + 1, K)
    ck.status("status again", _fwd(cuda, t, G, rows, D, K, again, rpd=rpd, n_seg=n_seg), OK)
    ck.same("run to run", again, out)
    out0 = _nan(cuda, 2, K)
    ck.status("n_seg=0 status", _fwd(cuda, t, G, rows, D, K, out0, rpd=rpd, n_seg=0), OK)
    ck.untouched("n_seg=0 out", out0)
    ck.done()


def test_heads_k_fwd_no_rows(cuda):
    i = mr.head_k_inputs(16, 5, 3, 4)
    t = _tensors(cuda, i)
    out = _nan(cuda, 2, 5)
    assert _fwd(cuda, t, 3, 0, 16, 5, out) == OK and _untouched(out)


def test_refusals_from_pointers_never_dereferenced(cuda):
    """K = 0, K = 17, D = 12, 9 groups, a misaligned h: X2G_EUNSUPPORTED; NULL arrays or entries, negative sizes:
    X2G_EINVAL; all decided on the host (the pointers are made-up addresses), nothing written."""
    so = _lib().load()
    fake = (ctypes.c_void_p * 9)(*[0x10000 * (g + 1) for g in range(9)])
    off = (ctypes.c_void_p * 9)(*[0x10000 * (g + 1) + 4 for g in range(9)])
    hole = (ctypes.c_void_p * 9)(*[None if g == 1 else 0x10000 * (g + 1) for g in range(9)])
    out, st = ctypes.c_void_p(0x900000), _st()
    ws = ctypes.c_void_p(0xA00000)

    def fwd(h=fake, w=fake, G=3, rows=8, D=16, K=5, o=out, rp=None, n_seg=0):
        return so.x2g_readout_heads_k_fwd(h, w, None, G, rows, D, K, rp, n_seg, o, st)

    def bwd(h=fake, w=fake, dh=None, dw=fake, G=3, rows=8, D=16, K=5, dout=out, flags=0, wsb=1 << 30, n_seg=0):
        return so.x2g_readout_heads_k_bwd(dout, None, n_seg, h, w, dh, dw, None, G, rows, D, K, flags, ws, wsb, st)

    for f in (fwd, bwd):
        for kw in (dict(K=0), dict(K=17), dict(D=12), dict(D=0), dict(D=512), dict(G=9), dict(G=0), dict(h=off),
                   dict(w=off)):
            assert f(**kw) == EUNSUPPORTED, (f.__name__, kw)
        for kw in (dict(h=None), dict(w=None), dict(h=hole), dict(w=hole), dict(rows=-1), dict(n_seg=-1)):
            assert f(**kw) == EINVAL, (f.__name__, kw)
    assert fwd(o=None) == EINVAL
    assert bwd(dh=off) == EUNSUPPORTED
    assert bwd(dw=None) == EINVAL and bwd(dw=hole) == EINVAL and bwd(dout=None) == EINVAL
    assert bwd(wsb=16) == 1003  # X2G_EWORKSPACE
    assert bwd(rows=0, flags=DEFER) == EINVAL and bwd(rows=0, flags=ACCUM) == OK
    assert so.x2g_readout_heads_k_bwd_workspace(0, 16, 5, 3) == 0 and so.x2g_readout_heads_k_bwd_splits(0) == 0
    p = ctypes.c_void_p(0x10000)
    assert so.x2g_error_accum_cols(p, p, 8, 0, p, st) == EUNSUPPORTED
    assert so.x2g_error_accum_cols(p, p, 8, 17, p, st) == EUNSUPPORTED
    assert so.x2g_error_accum_cols(p, p, 0, 2, p, st) == EINVAL
    assert so.x2g_error_accum_cols(None, p, 8, 2, p, st) == EINVAL
    assert so.x2g_error_accum_cols(p, p, 8, 2, ctypes.c_void_p(0x10004), st) == EINVAL


# ------------------------------------------------------------------------------ backward
def _bwd(cuda, ck, t, G, rows, D, K, rpd, n_seg, *, mode, dh_null=(), db_null=()):
    """One x2g_readout_heads_k_bwd call; DEFER: then one x2g_slab_sum_batch over the slabs where the header places
    them (n_w = K*D, n_b = K)."""
    from x2gnn.ops import SlabJob

    so = _lib().load()
    dh = [None if g in dh_null else _nan(cuda, rows + 1, D) for g in range(G)]
    dw = [_nan(cuda, 2, K, D) for _ in range(G)]
    db = [None if g in db_null else _nan(cuda, 2, K) for g in range(G)]
    if mode & ACCUM:
        for g in range(G):
            dw[g][0] = t["dw_old"][g]
            if db[g] is not None:
                db[g][0] = t["db_old"][g]
    ws_b = int(so.x2g_readout_heads_k_bwd_workspace(rows, D, K, G))
    splits = int(so.x2g_readout_heads_k_bwd_splits(rows))
    per = K * D + K
    assert ws_b == G * splits * per * 4 and splits == min(max((rows + 31) // 32, 1), 256)
    ws = _nan(cuda, ws_b // 4 + WS_GUARD)
    rc = so.x2g_readout_heads_k_bwd(_p(t["dout"]), _p(rpd), n_seg or 0, _ptrs(t["hs"][:G]), _ptrs(t["ws"][:G]),
                                    _ptrs(dh) if len(dh_null) < G else None, _ptrs(dw), _ptrs(db), G, rows, D, K,
                                    mode & (ACCUM | DEFER), _p(ws), ws_b, _st())
    ck.status(f"status mode={mode}", rc, OK)
    if mode & DEFER:
        base = ws.data_ptr()
        jobs = (SlabJob * G)(*[SlabJob(base + 4 * g * splits * per,
                                       None if db[g] is None else base + 4 * (g * splits * per + splits * K * D),
                                       dw[g].data_ptr(), None if db[g] is None else db[g].data_ptr(), K * D,
                                       0 if db[g] is None else K, splits, 0, 0) for g in range(G)])
        ck.status("slab sum status", so.x2g_slab_sum_batch(jobs, G, 1 if mode & ACCUM else 0, _st()), OK)
    ck.untouched("workspace guard", ws[ws_b // 4:])
    return dh, dw, db


def _bwd_case(cuda, D, K, G, rows, rp=None):
    n_seg = None if rp is None else len(rp) - 1
    i = mr.head_k_inputs(D, K, G, rows, n_seg)
    t = _tensors(cuda, i)
    rpd = _dev(rp, cuda)
    ck = _Checker(f"bwd D={D} K={K} G={G} rows={rows} {'per-row' if rp is None else 'per-segment'}")
    null = dict(dh_null=tuple(range(1, G, 2)), db_null=tuple(range(2, G, 3)))
    ref = mr.heads_k_bwd(i["dout"], i["hs"], i["ws"], rp)
    wfam = "heads_k" if rp is None else "heads_k_seg"
    res = {}
    for mode in (0, ACCUM, DEFER, DEFER | ACCUM):
        dh, dw, db = res[mode] = _bwd(cuda, ck, t, G, rows, D, K, rpd, n_seg, mode=mode, **null)
        tag = {0: "", ACCUM: "[accum]", DEFER: "[defer]", DEFER | ACCUM: "[defer+accum]"}[mode]
        for g in range(G):
            rw, rb = ref[g]["dw"], ref[g]["db"]
            if mode & ACCUM:
                rw, rb = _plus(rw, i["dw_old"][g]), _plus(rb, i["db_old"][g])
            if dh[g] is not None:
                ck.check("heads_k", "dh" + tag, dh[g], rows, ref[g]["dh"])
            ck.check(wfam, "dw" + tag, dw[g], 1, rw)
            if db[g] is not None:
                ck.check(wfam, "db" + tag, db[g], 1, rb)
    again = _bwd(cuda, ck, t, G, rows, D, K, rpd, n_seg, mode=0, **null)
    for g in range(G):
        for k, name in enumerate(("dh", "dw", "db")):
            if res[0][k][g] is not None:
                ck.same(f"group {g} {name} run to run", again[k][g], res[0][k][g])
                ck.same(f"group {g} {name} deferred vs immediate", res[DEFER][k][g], res[0][k][g])
                ck.same(f"group {g} {name} deferred + accum vs accum", res[DEFER | ACCUM][k][g], res[ACCUM][k][g])
    if G == 1:  # dh == NULL as a whole (the array itself), once per case list entry with one group
        _bwd(cuda, ck, t, G, rows, D, K, rpd, n_seg, mode=0, dh_null=(0,))
    ck.done()


@pytest.mark.parametrize("D,K,G,rows", _ids(mr.bwd_cases(), lambda D, K, G, r: f"D{D}-K{K}-G{G}-rows{r}"))
def test_heads_k_bwd(cuda, D, K, G, rows):
    """dh_g = dout w_g, dw_g = dout^T h_g, db_g from per-row dout around the 32-rows-per-workgroup split and its
    256-workgroup cap (8193: the last 7 workgroups own no row and still write zero slabs into the NaN workspace); dh
    NULL for every second group, db NULL for every third; flags 0 (twice), accumulated onto old contents,
    deferred + x2g_slab_sum_batch."""
    _bwd_case(cuda, D, K, G, rows)


@pytest.mark.parametrize("D,K,G,rows", _ids(mr.bwd_seg_cases(), lambda D, K, G, r: f"D{D}-K{K}-G{G}-rows{r}"))
def test_heads_k_bwd_per_segment(cuda, D, K, G, rows):
    """dout per segment over the ragged rowptr: every dh row carries its own segment's dout row."""
    rp = mr.seg_rowptr_for(D, rows)
    _bwd_case(cuda, D, K, G, int(rp[-1]), rp)


def test_heads_k_bwd_no_rows(cuda):
    """R = 0: dw / db zeroed without X2G_ACCUM_WGRAD, untouched with it, X2G_EINVAL with X2G_DEFER_SLAB_SUM."""
    so = _lib().load()
    D, K, G = 16, 5, 3
    t = _tensors(cuda, mr.head_k_inputs(D, K, G, 4))
    ws = _nan(cuda, 1024)
    for flags, want in ((0, OK), (ACCUM, OK), (DEFER, EINVAL)):
        dw, db = [_nan(cuda, 2, K, D) for _ in range(G)], [_nan(cuda, 2, K) for _ in range(G)]
        rc = so.x2g_readout_heads_k_bwd(_p(t["dout"]), None, 0, _ptrs(t["hs"]), _ptrs(t["ws"]), None, _ptrs(dw),
                                        _ptrs(db), G, 0, D, K, flags, _p(ws), 4096, _st())
        assert rc == want, (flags, rc)
        for g in range(G):
            if flags == 0:
                assert float(dw[g][0].abs().max()) == 0.0 and float(db[g][0].abs().max()) == 0.0
                assert _untouched(dw[g][1]) and _untouched(db[g][1])
            else:
                assert _untouched(dw[g]) and _untouched(db[g])
    assert _untouched(ws)


# ------------------------------------------------------------------------------ the error statistics
SENTINEL = -12345.678
EPS = 2.0 ** -52


def _accumulate(cuda, calls, K, seed_acc=None):
    so = _lib().load()
    buf = torch.full((K + 1, 4), SENTINEL, dtype=torch.float64, device=cuda)
    buf[:K] = 0.0 if seed_acc is None else torch.tensor(seed_acc, dtype=torch.float64)
    keep = []
    for pred, target in calls:
        p, t = _dev(pred, cuda), _dev(target, cuda)
        keep.append((p, t))
        assert so.x2g_error_accum_cols(_p(p), _p(t), p.shape[0], K, _p(buf), _st()) == OK
    return buf.cpu().numpy()


@pytest.mark.parametrize("K", mr.ERR_K)
@pytest.mark.parametrize("n", mr.ERR_N)
def test_error_accum_cols_against_fp64(cuda, n, K):
    """Per target the two sums within n * 2^-52 of the fp64 reference (tests/test_gpu_metrics.py's bound), the
    maximum and the count exact, the doubles behind the accumulator untouched, two runs the same bits; K = 1: the
    bits of x2g_error_accum."""
    pred, target = mr.error_inputs(n, K)
    ref = mr.error_cols(pred, target)
    got = _accumulate(cuda, [(pred, target)], K)
    print(f"n={n} K={K}: worst sum error / bound",
          float((np.abs(got[:K, :2] - ref[:, :2]) / np.maximum(n * EPS * ref[:, :2], 1e-300)).max()))
    assert (np.abs(got[:K, :2] - ref[:, :2]) <= n * EPS * ref[:, :2]).all()
    assert (got[:K, 2] == ref[:, 2]).all() and (got[:K, 3] == n).all()
    assert (got[K:] == SENTINEL).all()
    assert got.tobytes() == _accumulate(cuda, [(pred, target)], K).tobytes()
    if K == 1:
        one = torch.zeros(4, dtype=torch.float64, device=cuda)
        p, t = _dev(pred, cuda), _dev(target, cuda)
        assert _lib().load().x2g_error_accum(_p(p), _p(t), n, _p(one), _st()) == OK
        assert one.cpu().numpy().tobytes() == got[0].tobytes()


def test_error_accum_cols_adds_over_two_calls(cuda):
    K = 12
    calls = [mr.error_inputs(n, K, seed=5) for n in (257, 4099)]
    refs = [mr.error_cols(p, t) for p, t in calls]
    seed_acc = np.tile(np.array([1.5, 2.25, 0.125, 3.0]), (K, 1))
    seed_acc[3, 2] = 1e9  # a running maximum larger than every batch's is kept
    got = _accumulate(cuda, calls, K, seed_acc)[:K]
    n = 257 + 4099
    want = seed_acc + refs[0] + refs[1]
    assert (np.abs(got[:, :2] - want[:, :2]) <= n * EPS * want[:, :2]).all()
    assert (got[:, 2] == np.maximum(seed_acc[:, 2], np.maximum(refs[0][:, 2], refs[1][:, 2]))).all()
    assert got[3, 2] == 1e9 and (got[:, 3] == 3.0 + n).all()


# ------------------------------------------------------------------------------ the wrappers
@pytest.mark.parametrize("bucket", [False, True], ids=["plain", "bucket-deferred"])
@pytest.mark.parametrize("pooled", [False, True], ids=["per-row", "pool"])
@pytest.mark.parametrize("D", [32, 128])
def test_wrapper_readout_mlps_k_targets(cuda, D, pooled, bucket):
    """ops.readout_mlps with Linear(D, 3) last layers (D = 128: the row-chain hidden layers; 32: the batched dense
    ones) against the same MLPs in float64 on the CPU: values and every gradient within 1e-4 of the largest
    reference magnitude (three fp32 layers of at most 128 terms per sum: some 1e-6); into a gradient bucket with the
    slab sums deferred: the same, and the heads' gradients the bits of plain autograd."""
    from x2gnn import ops
    from x2gnn.dist import GradBucket
    from x2gnn.layers import _mlp

    G, K = 3, 3
    rp = np.array([0, 0, 1, 6, 6, 18, 19, 37, 37], np.int32)
    rows, n_seg = 37, 8
    torch.manual_seed(11)
    mlps = [_mlp(D, K, 3).to(cuda) for _ in range(G)]
    feats = [torch.randn(rows, D, device=cuda).requires_grad_() for _ in range(G)]
    dout = torch.randn(n_seg if pooled else rows, K, device=cuda)
    pool = (_dev(rp, cuda), n_seg) if pooled else None
    assert ops.readout_mlps_supported(feats, mlps)
    params = [p for m in mlps for p in m.parameters()]

    def run(defer):
        for p in params:
            p.grad = None
        for f in feats:
            f.grad = None
        b = GradBucket(params) if defer else None
        if b is not None:
            b.zero()
        out = ops.readout_mlps(feats, mlps, pool=pool)
        if defer:
            with ops.deferred_wgrad():
                out.backward(dout)
        else:
            out.backward(dout)
        return out.detach().clone(), [f.grad.clone() for f in feats], [p.grad.clone() for p in params]

    out, dfeat, dpar = run(False)
    assert tuple(out.shape) == ((n_seg if pooled else rows), K)
    # float64 on the CPU
    ref_mlps = [torch.nn.Sequential(*[torch.nn.Linear(D, D if j < 4 else K) if j % 2 == 0 else torch.nn.SiLU()
                                      for j in range(5)]).double() for _ in range(G)]
    for rm, m in zip(ref_mlps, mlps):
        rm.load_state_dict({k: v.detach().cpu().double() for k, v in m.state_dict().items()})
    rfeats = [f.detach().cpu().double().requires_grad_() for f in feats]
    rout = sum(rm(f) for rm, f in zip(ref_mlps, rfeats))
    if pooled:
        rout = torch.zeros(n_seg, K, dtype=torch.float64).index_add_(0, torch.from_numpy(rr.owner_of(rp)), rout)
    rout.backward(dout.cpu().double())
    rpar = [p.grad for rm in ref_mlps for p in rm.parameters()]

    def close(a, b):
        assert float((a.cpu().double() - b).abs().max()) <= 1e-4 * float(b.abs().max())

    close(out, rout.detach())
    for a, b in zip(dfeat, rfeats):
        close(a, b.grad)
    for a, b in zip(dpar, rpar):
        close(a, b)
    if bucket:  # the hidden layers' deferred weight gradients take another row split: to the reference again; the
        out2, dfeat2, dpar2 = run(True)  # heads' slabs are the same ones, summed onto zeros: the same bits
        assert torch.equal(out2, out)
        for a, b in zip(dfeat2, rfeats):
            close(a, b.grad)
        for a, b in zip(dpar2, rpar):
            close(a, b)
        for g in range(G):
            assert torch.equal(dpar2[6 * g + 4], dpar[6 * g + 4]) and torch.equal(dpar2[6 * g + 5], dpar[6 * g + 5])


def test_wrapper_error_accum_cols(cuda):
    from x2gnn import ops

    pred, target = mr.error_inputs(65, 3)
    p, t = _dev(pred, cuda), _dev(target, cuda)
    acc = torch.zeros(3, 4, dtype=torch.float64, device=cuda)
    ops.error_accum_cols(p, t, acc)
    assert acc.cpu().numpy().tobytes() == _accumulate(cuda, [(pred, target)], 3)[:3].tobytes()
    for bad in ((p, t, acc.float()), (p, t, acc[:2]), (p, t[:64], acc), (p.double(), t, acc), (p[:, 0], t[:, 0], acc)):
        with pytest.raises(ValueError):
            ops.error_accum_cols(*bad)


def test_smooth_l1_loss_takes_wide_targets(cuda):
    """ops.smooth_l1_loss on [B, K] against [B, K]: F.smooth_l1_loss's own mean over B * K elements (reference
    trainer.py:41), value and gradient, under readout_ref's loss bound."""
    from x2gnn import ops

    B, K = 37, 12
    p, t = rr.loss_inputs(B * K, 1.0)
    pred = _dev(p.reshape(B, K), cuda).requires_grad_()
    loss = ops.smooth_l1_loss(pred, _dev(t.reshape(B, K), cuda))
    loss.backward()
    (l, lu), (dp, dpu) = rr.smooth_l1_mean(p, t, 1.0)
    assert tuple(pred.grad.shape) == (B, K)
    assert abs(float(loss.detach()) - l) <= rr.K["loss"] * rr.E32 * lu
    assert rr._ratio(pred.grad.cpu().numpy().reshape(-1), dp, dpu) <= rr.K["loss"]
    want = torch.nn.functional.smooth_l1_loss(torch.from_numpy(p.reshape(B, K)).double(),
                                              torch.from_numpy(t.reshape(B, K)).double())
    assert abs(l - float(want)) <= 1e-12 * abs(float(want))
