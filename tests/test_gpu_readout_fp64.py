"""Every entry point of the rbf gate / pool (csrc/rbf_gate.hip), the readout heads and the smooth-L1 loss
(csrc/readout.hip) against the fp64 statement of the operation (tests/readout_ref.py), element by element, at the
smallest shapes at which each loop structure changes.

Bound (nothing taken from the code under test): every element has to be finite and within K * 2^-24 * unit of the
fp64 value, the unit being the fp64 sum of the magnitudes of the terms that make the value up (readout_ref); where
the unit is 0 the kernel has to return exactly 0.  K per family (gate / pool forward, gate backward, heads, loss) was
fixed against a numpy-float32 emulation on the CPU (tests/test_readout_ref.py).  Calls go through the raw ABI
(x2gnn._lib).  Every output buffer is prefilled with NaN and carries one guard row (or element) that has to stay
untouched bit for bit; every workspace is prefilled with NaN and followed by guard floats; inputs are seeded on the
CPU.  Tiles (rows per workgroup or wave pass) are readout_ref's ``*_tile`` functions, read from the kernels' RPB /
RPI / RPW / UNROLL; a case id names the boundary it sits on.

``python tests/test_gpu_readout_fp64.py --write profiles/readout_fp64_err.json`` runs every case once and writes,
per (entry point, output, shape), the number of comparisons and the worst error / bound with the case it occurred
in, each family's K with the emulation's ratio, and the run's wall time.
"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

if __name__ == "__main__":  # (run as a script: the paths conftest.py sets up for pytest)
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "x2-gnn_amd"), os.path.join(_root, "tests")]

import readout_ref as rr

pytestmark = pytest.mark.gpu

RECORD = []  # one dict per comparison made (the --write entry dumps it)
ACCUM, DEFER, DRBF_ACCUM = 1, 2, 4  # X2G_ACCUM_WGRAD, X2G_DEFER_SLAB_SUM, X2G_GATE_DRBF_ACCUM
OK, EINVAL, EUNSUPPORTED = 0, 1001, 1002
WS_GUARD = 64  # NaN floats after every workspace
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


def _addr(t):
    return None if t is None else t.data_ptr()


class _Checker:
    """Compares the outputs of one case with the reference; collects every figure before failing."""

    def __init__(self, entry, shape, case):
        self.key = dict(entry=entry, shape=shape, case=case)
        self.bad = []

    def check(self, fam, output, buf, rows, ref_unit, entry=None):
        """``buf``: the device buffer of rows + 1 leading entries, the last one the guard; ``ref_unit``: (value,
        unit) float64 of ``rows`` leading entries."""
        rec = dict(self.key, output=output, rows=int(rows), family=fam)
        if entry:
            rec["entry"] = entry
        if rows == 0:  # nothing to compare: the guard alone
            if not _untouched(buf):
                self.bad.append((rec, "guard written"))
            return
        ref = np.asarray(ref_unit[0], np.float64).reshape(rows, -1)
        unit = np.asarray(ref_unit[1], np.float64).reshape(rows, -1)
        assert buf.shape[0] == rows + 1, (buf.shape, rows)
        if not _untouched(buf[rows:]):
            self.bad.append((rec, "guard written"))
        got = buf[:rows].detach().cpu().double().numpy().reshape(rows, -1)
        assert got.shape == ref.shape, (got.shape, ref.shape)
        if not np.isfinite(got).all():
            self.bad.append((rec, f"{int((~np.isfinite(got)).sum())} non-finite elements"))
            return
        if not got.size:
            return
        err = np.abs(got - ref)
        bound = rr.K[fam] * rr.E32 * unit
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(unit > 0, err / bound, np.where(err > 0, np.inf, 0.0))
        w = np.unravel_index(np.argmax(ratio), ratio.shape)
        rec.update(ratio=float(ratio[w]), abs_err=float(err[w]), bound=float(bound[w]), elements=int(got.size))
        RECORD.append(rec)
        if not rec["ratio"] <= 1.0:
            self.bad.append((rec, "error above bound"))

    def same(self, what, a, b):
        if not torch.equal(_bits(a), _bits(b)):
            self.bad.append((dict(self.key, output=what), "not bitwise equal"))

    def untouched(self, what, t):
        if not _untouched(t):
            self.bad.append((dict(self.key, output=what), "written"))

    def status(self, what, rc, want):
        if rc != want:
            self.bad.append((dict(self.key, output=what), f"status {rc}, expected {want}"))

    def done(self):
        assert not self.bad, "\n".join(f"{why}: {rec}" for rec, why in self.bad)


def _ids(params, fmt):
    return [pytest.param(*p, id=fmt(*p)) for p in params]


def _plus(ref_unit, old):
    """(value, unit) of a result added onto old contents."""
    old = np.asarray(old, np.float64)
    return ref_unit[0] + old, ref_unit[1] + np.abs(old)


# ------------------------------------------------------------------------------ a. x2g_rbf_gate_fwd
def _gate_fwd(cuda, x, rbf, w, b, rows, D, R):
    out = _nan(cuda, rows + 1, D)
    t = [_dev(a, cuda) for a in (x, rbf, w, b)]
    rc = _lib().load().x2g_rbf_gate_fwd(_p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), rows, D, R, _p(out), _st())
    return rc, out


def _gate_fwd_case(cuda, D, R, rows, why):
    i = rr.gate_inputs(D, R, rows)
    j = i["jobs"][0]
    ck = _Checker("x2g_rbf_gate_fwd", f"D={D} R={R}", f"rows={rows} {why}")
    for b in (j["b"], None):
        rc, out = _gate_fwd(cuda, j["x"], i["rbf"], j["w"], b, rows, D, R)
        ck.status("status", rc, OK)
        ck.check("gate_fwd", "out" if b is not None else "out[b NULL]", out, rows, rr.gate(j["x"], i["rbf"], j["w"], b))
    ck.done()


@pytest.mark.parametrize("R", rr.GATE_R)
@pytest.mark.parametrize("D", rr.GATE_D)
def test_gate_fwd_every_shape(cuda, D, R):
    """out = x * (rbf @ w.T + b) at every compiled (D, R), three workgroup tiles + 5 rows, b present and NULL."""
    _gate_fwd_case(cuda, D, R, 3 * rr.gate_fwd_tile(D) + 5, "3tiles+5")


@pytest.mark.parametrize("D,rows,why", _ids([(D, r, w) for D in rr.GATE_D for r, w in rr.gate_fwd_rows(D)],
                                            lambda D, r, w: f"D{D}-{w}-{r}"))
def test_gate_fwd_rows(cuda, D, rows, why):
    """0 rows (nothing written), 1 row, and one less than / exactly / one more than the workgroup's RPB x UNROLL
    tile of rows, R = 6 and 7."""
    for R in (6, 7):
        _gate_fwd_case(cuda, D, R, rows, why)


@pytest.mark.parametrize("D,R", [(32, 6), (128, 9), (128, 0), (12, 3)])
def test_gate_fwd_unsupported(cuda, D, R):
    """Shapes outside the compiled set: X2G_EUNSUPPORTED, the output untouched."""
    i = rr.gate_inputs(D, max(R, 1), 5)
    j = i["jobs"][0]
    rc, out = _gate_fwd(cuda, j["x"], i["rbf"], j["w"], j["b"], 5, D, R)
    assert rc == EUNSUPPORTED and _untouched(out)


# ------------------------------------------------------------------------------ b. x2g_rbf_pool_fwd(_batch)
def _pool_fwd(cuda, x, rbf, w, b, rp, D, R):
    n_seg = len(rp) - 1
    out = _nan(cuda, n_seg + 1, D)
    t = [_dev(a, cuda) for a in (x, rbf, w, b, rp)]
    rc = _lib().load().x2g_rbf_pool_fwd(_p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), _p(t[4]), n_seg, D, R, _p(out), _st())
    return rc, out


def _pool_batch(cuda, i, biases, rp, D, R, n_jobs):
    from x2gnn.ops import GateJob

    n_seg = len(rp) - 1
    outs = [_nan(cuda, n_seg + 1, D) for _ in range(n_jobs)]
    keep = [[_dev(a, cuda) for a in (j["x"], j["w"], b)] for j, b in zip(i["jobs"], biases)]
    rbf, rpd = _dev(i["rbf"], cuda), _dev(rp, cuda)
    jobs = (GateJob * n_jobs)(*[GateJob(_addr(k[0]), _addr(k[1]), _addr(k[2]), _addr(o), None, None, None, None, None)
                                for k, o in zip(keep, outs)])
    rc = _lib().load().x2g_rbf_pool_fwd_batch(jobs, n_jobs, _p(rbf), _p(rpd), n_seg, D, R, _st())
    return rc, outs


@pytest.mark.parametrize("R", rr.GATE_R)
@pytest.mark.parametrize("D", rr.GATE_D)
def test_pool_fwd_ragged(cuda, D, R):
    """Segment sums of x * f over one rowptr with empty segments first, in the middle and last, 1 row, one less
    than / exactly / one more than the wave's UNROLL x RPI tile and 400 rows; b present and NULL; then the batch
    entry with 1, 3 and 8 jobs (NULL and present biases mixed): each job bitwise the single-job kernel's."""
    rp = rr.ragged_rowptr(rr.pool_tile(D))
    rows = int(rp[-1])
    i = rr.gate_inputs(D, R, rows, jobs=8)
    ck = _Checker("x2g_rbf_pool_fwd", f"D={D} R={R}", f"ragged tile={rr.pool_tile(D)} rows={rows}")
    single = []
    for k, j in enumerate(i["jobs"]):
        b = None if k % 2 else j["b"]
        rc, out = _pool_fwd(cuda, j["x"], i["rbf"], j["w"], b, rp, D, R)
        ck.status("status", rc, OK)
        ck.check("gate_fwd", "pooled" if b is not None else "pooled[b NULL]", out, len(rp) - 1,
                 rr.pool(j["x"], i["rbf"], j["w"], b, rp))
        single.append(out)
    for n_jobs in (1, 3, 8):
        rc, outs = _pool_batch(cuda, i, [None if k % 2 else j["b"] for k, j in enumerate(i["jobs"])], rp, D, R, n_jobs)
        ck.status(f"batch[{n_jobs}] status", rc, OK)
        for k in range(n_jobs):
            ck.same(f"x2g_rbf_pool_fwd_batch[{n_jobs}] job {k}", outs[k], single[k])
        j = i["jobs"][n_jobs - 1]
        ck.check("gate_fwd", "pooled", outs[-1], len(rp) - 1,
                 rr.pool(j["x"], i["rbf"], j["w"], None if (n_jobs - 1) % 2 else j["b"], rp),
                 entry="x2g_rbf_pool_fwd_batch")
    ck.done()


@pytest.mark.parametrize("D", rr.GATE_D)
def test_pool_fwd_edges(cuda, D):
    """n_seg = 0 (nothing written, single and batch), n_seg = 1 (one segment of tile + 1 rows), 9 jobs ->
    X2G_EINVAL, R = 9 -> X2G_EUNSUPPORTED."""
    R, t = 6, rr.pool_tile(D)
    i = rr.gate_inputs(D, R, t + 1, jobs=8)
    j = i["jobs"][0]
    ck = _Checker("x2g_rbf_pool_fwd", f"D={D} R={R}", "edges")
    rp0, rp1 = np.array([0], np.int32), np.array([0, t + 1], np.int32)
    rc, out = _pool_fwd(cuda, j["x"], i["rbf"], j["w"], j["b"], rp0, D, R)
    ck.status("n_seg=0 status", rc, OK)
    ck.untouched("n_seg=0 out", out)
    rc, outs = _pool_batch(cuda, i, [q["b"] for q in i["jobs"]], rp0, D, R, 3)
    ck.status("batch n_seg=0 status", rc, OK)
    for o in outs:
        ck.untouched("batch n_seg=0 out", o)
    rc, out = _pool_fwd(cuda, j["x"], i["rbf"], j["w"], j["b"], rp1, D, R)
    ck.status("n_seg=1 status", rc, OK)
    ck.check("gate_fwd", "pooled", out, 1, rr.pool(j["x"], i["rbf"], j["w"], j["b"], rp1))
    i9 = dict(i, jobs=i["jobs"] + i["jobs"][:1])
    rc, outs = _pool_batch(cuda, i9, [q["b"] for q in i9["jobs"]], rp1, D, R, 9)
    ck.status("9 jobs status", rc, EINVAL)
    for o in outs:
        ck.untouched("9 jobs out", o)
    rc, out = _pool_fwd(cuda, j["x"], np.zeros((t + 1, 9), F), np.zeros((D, 9), F), j["b"], rp1, D, 9)
    ck.status("R=9 status", rc, EUNSUPPORTED)
    ck.untouched("R=9 out", out)
    ck.done()


# ------------------------------------------------------------------------------ c. x2g_rbf_gate_bwd(_batch)
def _gate_bwd_outputs(cuda, rows, D, R, tj, *, dx, drbf, db, mode, drbf_old):
    """NaN-prefilled outputs with guards (dx 'alias': prefilled with dx_add; accumulating ones: with the old values)."""
    o = dict(dx=None if dx is None else _nan(cuda, rows + 1, D), drbf=None if drbf is None else _nan(cuda, rows + 1, R),
             dw=_nan(cuda, D + 1, R), db=_nan(cuda, D + 1) if db else None)
    if dx == "alias":
        o["dx"][:rows] = tj["dx_add"]
    if drbf == "accum":
        o["drbf"][:rows] = drbf_old
    if mode & ACCUM:
        o["dw"][:D] = tj["dw_old"]
        if db:
            o["db"][:D] = tj["db_old"]
    return o


def _workspace(cuda, n_bytes):
    assert n_bytes % 4 == 0
    return _nan(cuda, n_bytes // 4 + WS_GUARD)


def _gate_bwd(cuda, ck, t, owner_d, rows, D, R, *, dx="plain", drbf="plain", db=True, bias=True, mode=0):
    """One x2g_rbf_gate_bwd call.  dx: None | 'plain' | 'add' | 'alias'; drbf: None | 'plain' | 'accum'; mode: 0,
    ACCUM, DEFER (then one x2g_slab_sum_batch over the slabs the header places at the start of the workspace) or
    DEFER | ACCUM."""
    from x2gnn.ops import SlabJob

    lib = _lib().load()
    tj = t["jobs"][0]
    o = _gate_bwd_outputs(cuda, rows, D, R, tj, dx=dx, drbf=drbf, db=db, mode=mode, drbf_old=t["drbf_old"])
    ws_b = int(lib.x2g_rbf_gate_bwd_workspace(rows, D, R))
    splits = int(lib.x2g_rbf_gate_bwd_splits(rows))
    assert ws_b == splits * D * (R + 1) * 4 and splits == min(max((rows + 7) // 8, 1), rr.GATE_BWD_SPLITS)
    ws = _workspace(cuda, ws_b)
    add = {None: None, "plain": None, "add": tj["dx_add"], "alias": o["dx"]}[dx]
    flags = (mode & (ACCUM | DEFER)) | (DRBF_ACCUM if drbf == "accum" else 0)
    rc = lib.x2g_rbf_gate_bwd(_p(tj["g"]), _p(owner_d), _p(tj["x"]), _p(t["rbf"]), _p(tj["w"]),
                              _p(tj["b"]) if bias else None, rows, D, R, _p(o["dx"]), _p(add), _p(o["drbf"]), _p(o["dw"]),
                              _p(o["db"]), flags, _p(ws), ws_b, _st())
    ck.status(f"status mode={mode}", rc, OK)
    if mode & DEFER:
        job = (SlabJob * 1)(SlabJob(ws.data_ptr(), ws.data_ptr() + 4 * splits * D * R if db else None, _addr(o["dw"]),
                                    _addr(o["db"]), D * R, D if db else 0, splits, 0, 0))
        ck.status("slab sum status", lib.x2g_slab_sum_batch(job, 1, 1 if mode & ACCUM else 0, _st()), OK)
    ck.untouched("workspace guard", ws[ws_b // 4:])
    return o


def _gate_tensors(cuda, i):
    t = dict(rbf=_dev(i["rbf"], cuda), drbf_old=_dev(i["drbf_old"], cuda), jobs=[])
    for j in i["jobs"]:
        t["jobs"].append({k: _dev(v, cuda) for k, v in j.items()})
    return t


def _gate_bwd_ref(i, j, owner, *, dx, drbf, bias, mode):
    ref = rr.gate_bwd(j["g"], owner, j["x"], i["rbf"], j["w"], j["b"] if bias else None,
                      j["dx_add"] if dx in ("add", "alias") else None, i["drbf_old"] if drbf == "accum" else None)
    if mode & ACCUM:
        ref["dw"], ref["db"] = _plus(ref["dw"], j["dw_old"]), _plus(ref["db"], j["db_old"])
    return ref


def _check_gate_bwd(ck, o, ref, rows, D, tag=""):
    for k, n in (("dx", rows), ("drbf", rows), ("dw", D), ("db", D)):
        if o[k] is not None:
            ck.check("gate_bwd", k + tag, o[k], n, ref[k])


def _owner(D, rows, pool_mode):
    if not pool_mode:
        return None, None
    rp = rr.ragged_rowptr(rr.pool_tile(D), rows)
    return rr.owner_of(rp).astype(np.int32), len(rp) - 1


def _gate_bwd_case(cuda, D, R, rows, why, pool_mode):
    """flags 0 (twice: equal bits), X2G_ACCUM_WGRAD onto known values, X2G_DEFER_SLAB_SUM + x2g_slab_sum_batch
    (written and added): each against the reference, the deferred results bitwise the immediate ones and the
    accumulated ones bitwise old + the written ones."""
    owner, n_seg = _owner(D, rows, pool_mode)
    i = rr.gate_inputs(D, R, rows, n_seg)
    j = i["jobs"][0]
    t = _gate_tensors(cuda, i)
    owner_d = _dev(owner, cuda)
    ck = _Checker("x2g_rbf_gate_bwd", f"D={D} R={R}", f"rows={rows} {why} {'pool' if pool_mode else 'gate'}")
    opt = dict(dx="add", drbf="accum", db=True, bias=True)
    res = {}
    for mode in (0, ACCUM, DEFER, DEFER | ACCUM):
        res[mode] = _gate_bwd(cuda, ck, t, owner_d, rows, D, R, mode=mode, **opt)
        tag = {0: "", ACCUM: "[accum]", DEFER: "[defer]", DEFER | ACCUM: "[defer+accum]"}[mode]
        _check_gate_bwd(ck, res[mode], _gate_bwd_ref(i, j, owner, mode=mode, dx="add", drbf="accum", bias=True), rows, D,
                        tag)
    again = _gate_bwd(cuda, ck, t, owner_d, rows, D, R, mode=0, **opt)
    for k in ("dx", "drbf", "dw", "db"):
        ck.same(f"{k} run to run", again[k], res[0][k])
        ck.same(f"{k} deferred vs immediate", res[DEFER][k], res[0][k])
        ck.same(f"{k} deferred + accum vs accum", res[DEFER | ACCUM][k], res[ACCUM][k])
    tj = t["jobs"][0]
    ck.same("dw accum vs old + dw", res[ACCUM]["dw"][:D], tj["dw_old"] + res[0]["dw"][:D])
    ck.same("db accum vs old + db", res[ACCUM]["db"][:D], tj["db_old"] + res[0]["db"][:D])
    ck.same("dx accum vs written", res[ACCUM]["dx"], res[0]["dx"])
    ck.done()


@pytest.mark.parametrize("pool_mode", [False, True], ids=["gate", "pool"])
@pytest.mark.parametrize("R", rr.GATE_R)
@pytest.mark.parametrize("D", rr.GATE_D)
def test_gate_bwd_every_shape(cuda, D, R, pool_mode):
    """Every compiled (D, R) (transpose_sum and its j < R write mask differ at each) at 1025 rows: 128 workgroups
    of 9 rows, the last 14 of which own no row and still have to write a zero slab into the NaN workspace."""
    _gate_bwd_case(cuda, D, R, 1025, "empty-workgroups", pool_mode)


@pytest.mark.parametrize("pool_mode", [False, True], ids=["gate", "pool"])
@pytest.mark.parametrize("D,rows,why", _ids([(D, r, w) for D in rr.GATE_D for r, w in rr.gate_bwd_rows(D) if r != 1025],
                                            lambda D, r, w: f"D{D}-{w}-{r}"))
def test_gate_bwd_rows(cuda, D, rows, why, pool_mode):
    """Row counts around the 8-rows-per-workgroup split, its 128-workgroup cap and a second UNROLL pass, R = 6."""
    _gate_bwd_case(cuda, D, 6, rows, why, pool_mode)


GATE_OPTIONS = [("dx-null", dict(dx=None)), ("drbf-null", dict(drbf=None)), ("db-null", dict(db=False)),
                ("b-null", dict(bias=False)), ("dx-add-separate", dict(dx="add")), ("dx-add-alias", dict(dx="alias")),
                ("drbf-accum", dict(drbf="accum")), ("only-dw", dict(dx=None, drbf=None, db=False))]


@pytest.mark.parametrize("name,opt", GATE_OPTIONS, ids=[n for n, _ in GATE_OPTIONS])
@pytest.mark.parametrize("D", rr.GATE_D)
def test_gate_bwd_options(cuda, D, name, opt):
    """Each optional operand absent and present (dx, drbf, db, b NULL; dx_add separate and aliasing dx;
    X2G_GATE_DRBF_ACCUM onto known values, guard row untouched) at R = 5 and 8, 9 and 1025 rows, gate and pool
    mode: against the reference, and every output it shares with the plain call bitwise equal to that call's."""
    for R, rows, pool_mode in ((5, 9, True), (8, 1025, False), (5, 1025, True)):
        owner, n_seg = _owner(D, rows, pool_mode)
        i = rr.gate_inputs(D, R, rows, n_seg)
        t = _gate_tensors(cuda, i)
        owner_d = _dev(owner, cuda)
        ck = _Checker("x2g_rbf_gate_bwd", f"D={D} R={R}", f"rows={rows} {name} {'pool' if pool_mode else 'gate'}")
        full = dict(dx="plain", drbf="plain", db=True, bias=True)
        o = _gate_bwd(cuda, ck, t, owner_d, rows, D, R, **dict(full, **opt))
        k = dict(full, **opt)
        ref = _gate_bwd_ref(i, i["jobs"][0], owner, mode=0, dx=k["dx"], drbf=k["drbf"], bias=k["bias"])
        _check_gate_bwd(ck, o, ref, rows, D, f"[{name}]")
        if k["bias"]:
            plain = _gate_bwd(cuda, ck, t, owner_d, rows, D, R, **full)
            for out in ("dx", "drbf", "dw", "db"):
                if o[out] is not None and not (out == "dx" and k["dx"] != "plain") and not (
                        out == "drbf" and k["drbf"] != "plain"):
                    ck.same(f"{out} [{name}] vs plain", o[out], plain[out])
        ck.done()


def _gate_bwd_batch(cuda, ck, t, owner_d, rows, D, R, n_jobs, plan, *, drbf, mode):
    """One x2g_rbf_gate_bwd_batch call; plan[k] = dict(dx, db, bias) of job k."""
    from x2gnn.ops import GateJob, SlabJob

    lib = _lib().load()
    outs, jobs = [], []
    for k in range(n_jobs):
        tj, p = t["jobs"][k], plan[k]
        o = _gate_bwd_outputs(cuda, rows, D, R, tj, dx=p["dx"], drbf=None, db=p["db"], mode=mode, drbf_old=None)
        add = {None: None, "plain": None, "add": tj["dx_add"], "alias": o["dx"]}[p["dx"]]
        jobs.append(GateJob(_addr(tj["x"]), _addr(tj["w"]), _addr(tj["b"]) if p["bias"] else None, None, _addr(tj["g"]),
                            _addr(o["dx"]), _addr(add), _addr(o["dw"]), _addr(o["db"])))
        outs.append(o)
    drbf_b = None
    if drbf is not None:
        drbf_b = _nan(cuda, rows + 1, R)
        if drbf == "accum":
            drbf_b[:rows] = t["drbf_old"]
    ws_b = int(lib.x2g_rbf_gate_bwd_batch_workspace(rows, D, R, n_jobs))
    ws = _workspace(cuda, ws_b)
    slab = (SlabJob * n_jobs)()
    flags = (mode & (ACCUM | DEFER)) | (DRBF_ACCUM if drbf == "accum" else 0)
    rc = lib.x2g_rbf_gate_bwd_batch((GateJob * n_jobs)(*jobs), n_jobs, _p(owner_d), _p(t["rbf"]), rows, D, R, _p(drbf_b),
                                    flags, slab if mode & DEFER else None, _p(ws), ws_b, _st())
    ck.status(f"batch status mode={mode}", rc, OK)
    if mode & DEFER:
        ck.status("slab sum status", lib.x2g_slab_sum_batch(slab, n_jobs, 1 if mode & ACCUM else 0, _st()), OK)
    ck.untouched("workspace guard", ws[ws_b // 4:])
    return outs, drbf_b


@pytest.mark.parametrize("pool_mode", [False, True], ids=["gate", "pool"])
@pytest.mark.parametrize("n_jobs", [1, 3, 8])
@pytest.mark.parametrize("D,R,rows", [(64, 3, 1025), (128, 6, 9), (128, 6, 1025), (256, 8, 1025), (256, 1, 1541)])
def test_gate_bwd_batch(cuda, D, R, rows, n_jobs, pool_mode):
    """1, 3 and 8 jobs in one launch (NULL and present b / db / dx, dx_add separate and aliased mixed over the
    jobs): every job's dx, dw, db against the reference, drbf = the sum over the jobs in job order (written, and
    added onto known values with X2G_GATE_DRBF_ACCUM); flags 0 twice (equal bits), accumulated, and deferred with
    one x2g_slab_sum_batch over the returned jobs (bitwise the immediate results)."""
    owner, n_seg = _owner(D, rows, pool_mode)
    i = rr.gate_inputs(D, R, rows, n_seg, jobs=n_jobs)
    t = _gate_tensors(cuda, i)
    owner_d = _dev(owner, cuda)
    ck = _Checker("x2g_rbf_gate_bwd_batch", f"D={D} R={R}", f"rows={rows} jobs={n_jobs} {'pool' if pool_mode else 'gate'}")
    plan = [dict(dx=("plain", "add", None, "alias")[k % 4], db=k != 2, bias=k % 2 == 0) for k in range(n_jobs)]
    refjobs = [dict(g=j["g"], x=j["x"], w=j["w"], b=j["b"] if p["bias"] else None,
                    dx_add=j["dx_add"] if p["dx"] in ("add", "alias") else None) for j, p in zip(i["jobs"], plan)]
    refs, dref0 = rr.gate_bwd_batch(refjobs, owner, i["rbf"])
    res = {}
    for mode, drbf in ((0, "plain"), (0, "accum"), (ACCUM, "plain"), (DEFER, "plain"), (DEFER | ACCUM, "plain"),
                       (0, None)):
        outs, drbf_b = _gate_bwd_batch(cuda, ck, t, owner_d, rows, D, R, n_jobs, plan, drbf=drbf, mode=mode)
        res[(mode, drbf)] = (outs, drbf_b)
        dref = _plus(dref0, i["drbf_old"]) if drbf == "accum" else dref0
        tag = f"[mode={mode}" + ("" if drbf == "plain" else f" drbf {drbf}") + "]"
        for k in range(n_jobs):
            ref = dict(refs[k])
            if mode & ACCUM:
                ref["dw"], ref["db"] = _plus(ref["dw"], i["jobs"][k]["dw_old"]), _plus(ref["db"], i["jobs"][k]["db_old"])
            _check_gate_bwd(ck, dict(outs[k], drbf=None), ref, rows, D, tag)
        if drbf_b is not None:
            ck.check("gate_bwd", "drbf" + tag, drbf_b, rows, dref)
    again, drbf_again = _gate_bwd_batch(cuda, ck, t, owner_d, rows, D, R, n_jobs, plan, drbf="plain", mode=0)
    base, drbf_base = res[(0, "plain")]
    ck.same("drbf run to run", drbf_again, drbf_base)
    ck.same("drbf deferred vs immediate", res[(DEFER, "plain")][1], drbf_base)
    for k in range(n_jobs):
        for out in ("dx", "dw", "db"):
            if base[k][out] is not None:
                ck.same(f"job {k} {out} run to run", again[k][out], base[k][out])
                ck.same(f"job {k} {out} deferred vs immediate", res[(DEFER, "plain")][0][k][out], base[k][out])
                ck.same(f"job {k} {out} drbf NULL vs present", res[(0, None)][0][k][out], base[k][out])
                ck.same(f"job {k} {out} deferred + accum vs accum", res[(DEFER | ACCUM, "plain")][0][k][out],
                        res[(ACCUM, "plain")][0][k][out])
    ck.done()


def test_gate_bwd_invalid(cuda):
    """9 jobs -> X2G_EINVAL, D = 32 / R = 9 -> X2G_EUNSUPPORTED, rows = 0: dw / db zeroed (flags 0), untouched
    (X2G_ACCUM_WGRAD), X2G_EINVAL (X2G_DEFER_SLAB_SUM); nothing else written."""
    from x2gnn.ops import GateJob

    lib = _lib().load()
    D, R, rows = 64, 6, 9
    i = rr.gate_inputs(D, R, rows, jobs=1)
    t = _gate_tensors(cuda, i)
    tj = t["jobs"][0]
    ck = _Checker("x2g_rbf_gate_bwd", f"D={D} R={R}", "invalid")
    ws = _workspace(cuda, 1 << 20)

    def single(rows_, D_, R_, flags):
        o = _gate_bwd_outputs(cuda, rows, D, R, tj, dx="plain", drbf="plain", db=True, mode=0, drbf_old=None)
        rc = lib.x2g_rbf_gate_bwd(_p(tj["g"]), None, _p(tj["x"]), _p(t["rbf"]), _p(tj["w"]), _p(tj["b"]), rows_, D_, R_,
                                  _p(o["dx"]), None, _p(o["drbf"]), _p(o["dw"]), _p(o["db"]), flags, _p(ws), 1 << 20,
                                  _st())
        return rc, o

    for D_, R_ in ((32, 6), (64, 9)):
        rc, o = single(rows, D_, R_, 0)
        ck.status(f"D={D_} R={R_}", rc, EUNSUPPORTED)
        for k, v in o.items():
            ck.untouched(f"D={D_} R={R_} {k}", v)
    rc, o = single(0, D, R, 0)
    ck.status("rows=0", rc, OK)
    ck.check("gate_bwd", "dw[rows=0]", o["dw"], D, (np.zeros((D, R)), np.zeros((D, R))))
    ck.check("gate_bwd", "db[rows=0]", o["db"], D, (np.zeros(D), np.zeros(D)))
    ck.untouched("rows=0 dx", o["dx"])
    ck.untouched("rows=0 drbf", o["drbf"])
    rc, o = single(0, D, R, ACCUM)
    ck.status("rows=0 accum", rc, OK)
    rc2, o2 = single(0, D, R, DEFER)
    ck.status("rows=0 defer", rc2, EINVAL)
    for k in o:
        ck.untouched(f"rows=0 accum {k}", o[k])
        ck.untouched(f"rows=0 defer {k}", o2[k])
    dw = _nan(cuda, D + 1, R)
    jobs = (GateJob * 9)(*[GateJob(_addr(tj["x"]), _addr(tj["w"]), None, None, _addr(tj["g"]), None, None, _addr(dw), None)
                           for _ in range(9)])
    ck.status("9 jobs", lib.x2g_rbf_gate_bwd_batch(jobs, 9, None, _p(t["rbf"]), rows, D, R, None, 0, None, _p(ws), 1 << 20,
                                                   _st()), EINVAL)
    ck.untouched("9 jobs dw", dw)
    ck.untouched("workspace", ws)
    ck.done()


# ------------------------------------------------------------------------------ d. the readout heads
def _head_tensors(cuda, i):
    return dict(hs=[_dev(h, cuda) for h in i["hs"]], ws=[_dev(w, cuda) for w in i["ws"]],
                bs=[None if b is None else _dev(np.array([b], F), cuda) for b in i["bs"]], dout=_dev(i["dout"], cuda),
                dw_old=[_dev(a, cuda) for a in i["dw_old"]], db_old=[_dev(a, cuda) for a in i["db_old"]])


def _head_groups(t, G, dh=None, dw=None, db=None, h_off=0):
    from x2gnn.ops import HeadGroup

    none = [None] * G
    dh, dw, db = dh or none, dw or none, db or none
    return (HeadGroup * G)(*[HeadGroup(t["hs"][g % len(t["hs"])].data_ptr() + h_off, _addr(t["ws"][g % len(t["ws"])]),
                                       _addr(t["bs"][g % len(t["bs"])]), _addr(dh[g]), _addr(dw[g]), _addr(db[g]))
                             for g in range(G)])


def _head_fwd_case(cuda, D, G, rows, why):
    i = rr.head_inputs(D, G, max(rows, 1))  # (rows = 0: valid pointers all the same)
    t = _head_tensors(cuda, i)
    ck = _Checker("x2g_readout_head_fwd", f"D={D} G={G}", f"rows={rows} {why}")
    out = _nan(cuda, rows + 1)
    rc = _lib().load().x2g_readout_head_fwd(_head_groups(t, G), G, rows, D, _p(out), _st())
    ck.status("status", rc, OK)
    if rows:
        ck.check("heads", "out", out, rows, rr.heads(i["hs"], i["ws"], i["bs"]))
    else:
        ck.untouched("rows=0 out", out)
    ck.done()


@pytest.mark.parametrize("G", rr.HEAD_G)
@pytest.mark.parametrize("D,rows,why", _ids([(D, r, w) for D in rr.HEAD_D for r, w in rr.head_fwd_rows(D)[:-1]],
                                            lambda D, r, w: f"D{D}-{w}-{r}"))
def test_head_fwd(cuda, D, rows, why, G):
    """out[r] = sum_g (h_g[r] . w_g + b_g) at every compiled D, 1 / 3 / 8 groups (every third without a bias), 0
    rows, 1 row and one less than / exactly / one more than a workgroup's 4 x RPW rows."""
    _head_fwd_case(cuda, D, G, rows, why)


@pytest.mark.parametrize("D", rr.HEAD_D)
def test_head_fwd_past_grid_cap(cuda, D):
    """One row more than 2048 workgroups cover in one pass (the grid-stride loop's second pass), one group."""
    rows, why = rr.head_fwd_rows(D)[-1]
    _head_fwd_case(cuda, D, 1, rows, why)


def test_head_fwd_unsupported(cuda):
    """9 groups, D = 12 and an h pointer off by 4 bytes -> X2G_EUNSUPPORTED, the output untouched."""
    lib = _lib().load()
    i = rr.head_inputs(16, 3, 10)
    t = _head_tensors(cuda, i)
    for G, D, off in ((9, 16, 0), (3, 12, 0), (3, 16, 4)):
        out = _nan(cuda, 9)
        rc = lib.x2g_readout_head_fwd(_head_groups(t, G, h_off=off), G, 8, D, _p(out), _st())
        assert rc == EUNSUPPORTED and _untouched(out), (G, D, off, rc)
        rp = _dev(np.array([0, 8], np.int32), cuda)
        rc = lib.x2g_readout_head_pool_fwd(_head_groups(t, G, h_off=off), G, 8, D, _p(rp), 1, _p(out), _st())
        assert rc == EUNSUPPORTED and _untouched(out), (G, D, off, rc)


@pytest.mark.parametrize("G", rr.HEAD_G)
@pytest.mark.parametrize("D", rr.HEAD_D)
def test_head_pool_fwd(cuda, D, G):
    """The heads summed per segment: empty segments first, in the middle and last, 1 row, 4 RPW - 1 / 4 RPW /
    4 RPW + 1 rows and 300; n_seg = 0 leaves the output untouched."""
    rp = rr.ragged_rowptr(rr.head_tile(D), big=300)
    rows, n_seg = int(rp[-1]), len(rp) - 1
    i = rr.head_inputs(D, G, rows)
    t = _head_tensors(cuda, i)
    rpd = _dev(rp, cuda)
    lib = _lib().load()
    ck = _Checker("x2g_readout_head_pool_fwd", f"D={D} G={G}", f"ragged tile={rr.head_tile(D)} rows={rows}")
    out = _nan(cuda, n_seg + 1)
    ck.status("status", lib.x2g_readout_head_pool_fwd(_head_groups(t, G), G, rows, D, _p(rpd), n_seg, _p(out), _st()), OK)
    ck.check("heads", "out_seg", out, n_seg, rr.heads_pool(i["hs"], i["ws"], i["bs"], rp))
    out0 = _nan(cuda, 2)
    ck.status("n_seg=0 status", lib.x2g_readout_head_pool_fwd(_head_groups(t, G), G, rows, D, _p(rpd), 0, _p(out0), _st()),
              OK)
    ck.untouched("n_seg=0 out", out0)
    ck.done()


def _head_bwd(cuda, ck, t, G, rows, D, rpd, n_seg, *, mode, dh_null=(), db_null=()):
    """One x2g_readout_head_bwd (rpd None) or x2g_readout_head_pool_bwd call; DEFER: then one x2g_slab_sum_batch
    over the slabs where the header places them."""
    from x2gnn.ops import SlabJob

    lib = _lib().load()
    dh = [None if g in dh_null else _nan(cuda, rows + 1, D) for g in range(G)]
    dw = [_nan(cuda, 2, D) for _ in range(G)]
    db = [None if g in db_null else _nan(cuda, 2) for g in range(G)]
    if mode & ACCUM:
        for g in range(G):
            dw[g][0] = t["dw_old"][g]
            if db[g] is not None:
                db[g][:1] = t["db_old"][g]
    ws_b = int(lib.x2g_readout_head_bwd_workspace(rows, D, G))
    splits = int(lib.x2g_readout_head_bwd_splits(rows))
    assert ws_b == G * splits * (D + 1) * 4 and splits == min(max((rows + 31) // 32, 1), 256)
    ws = _workspace(cuda, ws_b)
    groups = _head_groups(t, G, dh, dw, db)
    flags = mode & (ACCUM | DEFER)
    if rpd is None:
        rc = lib.x2g_readout_head_bwd(_p(t["dout"]), groups, G, rows, D, flags, _p(ws), ws_b, _st())
    else:
        rc = lib.x2g_readout_head_pool_bwd(_p(t["dout"]), _p(rpd), n_seg, groups, G, rows, D, flags, _p(ws), ws_b, _st())
    ck.status(f"status mode={mode}", rc, OK)
    if mode & DEFER:
        jobs = (SlabJob * G)(*[SlabJob(ws.data_ptr() + 4 * g * splits * (D + 1),
                                       None if db[g] is None else ws.data_ptr() + 4 * (g * splits * (D + 1) + splits * D),
                                       _addr(dw[g]), _addr(db[g]), D, 0 if db[g] is None else 1, splits, 0, 0)
                               for g in range(G)])
        ck.status("slab sum status", lib.x2g_slab_sum_batch(jobs, G, 1 if mode & ACCUM else 0, _st()), OK)
    ck.untouched("workspace guard", ws[ws_b // 4:])
    return dh, dw, db


def _head_bwd_case(cuda, D, G, rows, why, rp=None):
    n_seg = None if rp is None else len(rp) - 1
    i = rr.head_inputs(D, G, rows, n_seg)
    t = _head_tensors(cuda, i)
    rpd = _dev(rp, cuda)
    entry = "x2g_readout_head_bwd" if rp is None else "x2g_readout_head_pool_bwd"
    ck = _Checker(entry, f"D={D} G={G}", f"rows={rows} {why}")
    null = dict(dh_null=tuple(range(1, G, 2)), db_null=tuple(range(2, G, 3)))
    ref = rr.heads_bwd(i["dout"], i["hs"], i["ws"], rp)
    res = {}
    for mode in (0, ACCUM, DEFER, DEFER | ACCUM):
        dh, dw, db = res[mode] = _head_bwd(cuda, ck, t, G, rows, D, rpd, n_seg, mode=mode, **null)
        tag = {0: "", ACCUM: "[accum]", DEFER: "[defer]", DEFER | ACCUM: "[defer+accum]"}[mode]
        for g in range(G):
            rw, rb = ref[g]["dw"], ref[g]["db"]
            if mode & ACCUM:
                rw, rb = _plus(rw, i["dw_old"][g]), _plus(rb, i["db_old"][g][0])
            if dh[g] is not None:
                ck.check("heads", "dh" + tag, dh[g], rows, ref[g]["dh"])
            ck.check("heads", "dw" + tag, dw[g], 1, rw)
            if db[g] is not None:
                ck.check("heads", "db" + tag, db[g], 1, (np.array([rb[0]]), np.array([rb[1]])))
    again = _head_bwd(cuda, ck, t, G, rows, D, rpd, n_seg, mode=0, **null)
    for g in range(G):
        for k, name in enumerate(("dh", "dw", "db")):
            if res[0][k][g] is not None:
                ck.same(f"group {g} {name} run to run", again[k][g], res[0][k][g])
                ck.same(f"group {g} {name} deferred vs immediate", res[DEFER][k][g], res[0][k][g])
                ck.same(f"group {g} {name} deferred + accum vs accum", res[DEFER | ACCUM][k][g], res[ACCUM][k][g])
        ck.same(f"group {g} dw accum vs old + dw", res[ACCUM][1][g][0], t["dw_old"][g] + res[0][1][g][0])
    ck.done()


@pytest.mark.parametrize("D,rows", _ids([(D, r) for D in rr.HEAD_D for r in rr.HEAD_BWD_ROWS],
                                        lambda D, r: f"D{D}-rows{r}" + {31: "-split-1", 32: "-split", 33: "-split+1",
                                                                        8191: "-256splits-1", 8192: "-256splits",
                                                                        8193: "-empty-workgroups"}.get(r, "")))
def test_head_bwd(cuda, D, rows):
    """dh_g = dout w_g, dw_g, db_g at every compiled D around the 32-rows-per-workgroup split and its 256-workgroup
    cap (8193: per = 33, the last 7 workgroups own no row and still write zero slabs into the NaN workspace); dh
    NULL for every second group, db NULL for every third; flags 0 (twice), accumulated, deferred."""
    for G in rr.head_bwd_groups(D, rows):
        _head_bwd_case(cuda, D, G, rows, "per-row")


@pytest.mark.parametrize("G", rr.HEAD_G)
@pytest.mark.parametrize("D", rr.HEAD_D)
def test_head_pool_bwd(cuda, D, G):
    """dout per segment over the ragged rowptr (empty segments first, in the middle and last, single-row
    segments): every dh row carries its own segment's dout."""
    rp = rr.ragged_rowptr(rr.head_tile(D), big=300)
    _head_bwd_case(cuda, D, G, int(rp[-1]), "ragged", rp)


@pytest.mark.parametrize("D,rows", [(4, 33), (32, 8193), (256, 8193)])
def test_head_pool_bwd_rows(cuda, D, rows):
    """The per-segment form across the workgroup split: 33 rows (2 workgroups) and 8193 (empty workgroups)."""
    _head_bwd_case(cuda, D, 3, rows, "ragged-cut", rr.ragged_rowptr(rr.head_tile(D), rows, big=300))


@pytest.mark.parametrize("pooled", [False, True], ids=["per-row", "per-segment"])
def test_head_bwd_no_rows(cuda, pooled):
    """R = 0: dw / db zeroed without X2G_ACCUM_WGRAD, untouched with it, X2G_EINVAL with X2G_DEFER_SLAB_SUM."""
    lib = _lib().load()
    D, G = 16, 3
    i = rr.head_inputs(D, G, 4, 2)
    t = _head_tensors(cuda, i)
    rpd = _dev(np.array([0, 0, 0], np.int32), cuda)
    ck = _Checker("x2g_readout_head_pool_bwd" if pooled else "x2g_readout_head_bwd", f"D={D} G={G}", "rows=0")
    ws = _workspace(cuda, 4096)
    for flags, want in ((0, OK), (ACCUM, OK), (DEFER, EINVAL)):
        dw, db = [_nan(cuda, 2, D) for _ in range(G)], [_nan(cuda, 2) for _ in range(G)]
        groups = _head_groups(t, G, None, dw, db)
        if pooled:
            rc = lib.x2g_readout_head_pool_bwd(_p(t["dout"]), _p(rpd), 2, groups, G, 0, D, flags, _p(ws), 4096, _st())
        else:
            rc = lib.x2g_readout_head_bwd(_p(t["dout"]), groups, G, 0, D, flags, _p(ws), 4096, _st())
        ck.status(f"flags={flags}", rc, want)
        for g in range(G):
            if flags == 0:
                ck.check("heads", "dw[rows=0]", dw[g], 1, (np.zeros(D), np.zeros(D)))
                ck.check("heads", "db[rows=0]", db[g], 1, (np.zeros(1), np.zeros(1)))
            else:
                ck.untouched(f"flags={flags} dw", dw[g])
                ck.untouched(f"flags={flags} db", db[g])
    ck.untouched("workspace", ws)
    ck.done()


# ------------------------------------------------------------------------------ e. the loss
@pytest.mark.parametrize("beta", rr.LOSS_BETA)
@pytest.mark.parametrize("n", rr.LOSS_N)
def test_smooth_l1(cuda, n, beta):
    """x2g_smooth_l1_mean_fwd / _fwd_grad / _bwd: n around the 256-thread workgroup and 262 145 (the backward's
    1024 x 256 grid-stride loop wraps), elements on d = 0, d = +-beta exactly, |d| = beta (1 +- 2^-23) and
    |d| = 100 beta; gout 1 and -0.37; dpred_unit bitwise the backward's for gout = 1."""
    lib = _lib().load()
    p, t = rr.loss_inputs(n, beta)
    pd, td = _dev(p, cuda), _dev(t, cuda)
    ck = _Checker("x2g_smooth_l1_mean", f"beta={beta}", f"n={n}")
    out, out2, unit_grad = _nan(cuda, 2), _nan(cuda, 2), _nan(cuda, n + 1)
    ck.status("fwd", lib.x2g_smooth_l1_mean_fwd(_p(pd), _p(td), n, beta, _p(out), _st()), OK)
    ck.status("fwd_grad", lib.x2g_smooth_l1_mean_fwd_grad(_p(pd), _p(td), n, beta, _p(out2), _p(unit_grad), _st()), OK)
    lref, dref = rr.smooth_l1_mean(p, t, beta, 1.0)
    ck.check("loss", "loss", out, 1, lref, entry="x2g_smooth_l1_mean_fwd")
    ck.check("loss", "loss", out2, 1, lref, entry="x2g_smooth_l1_mean_fwd_grad")
    ck.same("loss fwd_grad vs fwd", out2, out)
    ck.check("loss", "dpred_unit", unit_grad, n, dref, entry="x2g_smooth_l1_mean_fwd_grad")
    for gout in rr.LOSS_GOUT:
        gd, dp = _dev(np.array([gout], F), cuda), _nan(cuda, n + 1)
        ck.status("bwd", lib.x2g_smooth_l1_mean_bwd(_p(pd), _p(td), n, beta, _p(gd), _p(dp), _st()), OK)
        ck.check("loss", f"dpred[gout={gout}]", dp, n, rr.smooth_l1_mean(p, t, beta, gout)[1],
                 entry="x2g_smooth_l1_mean_bwd")
        if gout == 1.0:
            ck.same("dpred_unit vs bwd(gout = 1)", unit_grad, dp)
    ck.done()


def test_smooth_l1_invalid(cuda):
    """n = 0 or beta = 0 -> X2G_EINVAL from all three, nothing written."""
    lib = _lib().load()
    p, t = rr.loss_inputs(3, 1.0)
    pd, td, gd = _dev(p, cuda), _dev(t, cuda), _dev(np.ones(1, F), cuda)
    for n, beta in ((0, 1.0), (3, 0.0)):
        out, dp = _nan(cuda, 2), _nan(cuda, 4)
        assert lib.x2g_smooth_l1_mean_fwd(_p(pd), _p(td), n, beta, _p(out), _st()) == EINVAL
        assert lib.x2g_smooth_l1_mean_fwd_grad(_p(pd), _p(td), n, beta, _p(out), _p(dp), _st()) == EINVAL
        assert lib.x2g_smooth_l1_mean_bwd(_p(pd), _p(td), n, beta, _p(gd), _p(dp), _st()) == EINVAL
        assert _untouched(out) and _untouched(dp)


# ------------------------------------------------------------------------------ f. the wrappers under autograd
WRAP_D, WRAP_R = 128, 6
WRAP_RP = np.array([0, 0, 1, 6, 6, 18, 19, 37, 37], np.int32)  # 37 rows in ragged segments


def _params(cuda, arrays, bucket):
    """CUDA parameters of the arrays; ``bucket``: their gradients are views of one flat zeroed GradBucket."""
    from x2gnn.dist import GradBucket

    ps = [None if a is None else torch.nn.Parameter(_dev(a, cuda)) for a in arrays]
    keep = GradBucket([p for p in ps if p is not None]) if bucket else None
    return ps, keep


def _backward(bucket, outs, grads):
    from x2gnn import ops

    if bucket:
        with ops.deferred_wgrad():
            torch.autograd.backward(outs, grads)
    else:
        torch.autograd.backward(outs, grads)


def _with_guard(t):
    """A [rows, ...] result as a checker buffer: one NaN guard row appended (a wrapper owns its outputs)."""
    t = t.detach().reshape(t.shape[0], -1) if t.dim() > 1 else t.detach()
    return torch.cat([t, torch.full((1,) + tuple(t.shape[1:]), float("nan"), device=t.device)])


@pytest.mark.parametrize("bucket", [False, True], ids=["plain", "bucket-deferred"])
@pytest.mark.parametrize("n_jobs", [1, 3])
def test_wrapper_rbf_pool(cuda, n_jobs, bucket):
    """ops.rbf_pool (one job) / ops.rbf_pool_batch (three) under autograd: pooled sums, dx, drbf (summed over the
    jobs), dw, db against the reference; plain parameters, and bucket-backed ones inside ops.deferred_wgrad()."""
    from x2gnn import ops

    rows, n_seg = int(WRAP_RP[-1]), len(WRAP_RP) - 1
    owner = rr.owner_of(WRAP_RP).astype(np.int32)
    i = rr.gate_inputs(WRAP_D, WRAP_R, rows, n_seg, jobs=n_jobs)
    xs = [_dev(j["x"], cuda).requires_grad_() for j in i["jobs"]]
    rbf = _dev(i["rbf"], cuda).requires_grad_()
    ps, keep = _params(cuda, [j["w"] for j in i["jobs"]] + [j["b"] for j in i["jobs"]], bucket)
    ws, bs = ps[:n_jobs], ps[n_jobs:]
    od, rpd = _dev(owner, cuda), _dev(WRAP_RP, cuda)
    if n_jobs == 1:
        outs = [ops.rbf_pool(xs[0], rbf, ws[0], bs[0], od, rpd, n_seg)]
    else:
        outs = ops.rbf_pool_batch(xs, rbf, ws, bs, od, rpd, n_seg)
    _backward(bucket, outs, [_dev(j["g"], cuda) for j in i["jobs"]])
    ck = _Checker("ops.rbf_pool" if n_jobs == 1 else "ops.rbf_pool_batch", f"D={WRAP_D} R={WRAP_R}",
                  f"rows={rows} jobs={n_jobs} {'bucket' if bucket else 'plain'}")
    refs, dref = rr.gate_bwd_batch([dict(g=j["g"], x=j["x"], w=j["w"], b=j["b"]) for j in i["jobs"]], owner, i["rbf"])
    for k, j in enumerate(i["jobs"]):
        ck.check("gate_fwd", "pooled", _with_guard(outs[k]), n_seg, rr.pool(j["x"], i["rbf"], j["w"], j["b"], WRAP_RP))
        ck.check("gate_bwd", "dx", _with_guard(xs[k].grad), rows, refs[k]["dx"])
        ck.check("gate_bwd", "dw", _with_guard(ws[k].grad), WRAP_D, refs[k]["dw"])
        ck.check("gate_bwd", "db", _with_guard(bs[k].grad), WRAP_D, refs[k]["db"])
    ck.check("gate_bwd", "drbf", _with_guard(rbf.grad), rows, dref)
    ck.done()


SILU_LIP, SILU_CURV = 1.1, 0.5  # max |silu'| = 1.0998, max |silu''| = 0.5


def _mlp_reference(feats, params, dout, rp):
    """Three-layer readout MLPs in float64 with first-order units: each stage's unit is the sum of its own terms'
    magnitudes plus its inputs' units carried through |W|, the SiLU's slope (<= 1.1) and curvature (<= 0.5).
    -> (out (value, unit), per group dict of (value, unit) for dfeat, w1, b1, w2, b2, w3, b3)."""
    f8 = lambda a: np.asarray(a, np.float64)  # noqa: E731
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))  # noqa: E731
    d = f8(dout) if rp is None else f8(dout)[rr.owner_of(rp)]
    out = unit = 0.0
    grads = []
    for x, (w1, b1, w2, b2, w3, b3) in zip(feats, params):
        x, w1, b1, w2, b2, w3, b3 = (f8(a) for a in (x, w1, b1, w2, b2, w3, b3))
        w3 = w3.reshape(-1)
        z1, uz1 = x @ w1.T + b1, np.abs(x) @ np.abs(w1).T + np.abs(b1)
        h1 = z1 * sig(z1)
        uh1 = SILU_LIP * uz1 + np.abs(h1)
        z2 = h1 @ w2.T + b2
        uz2 = (uh1 + np.abs(h1)) @ np.abs(w2).T + np.abs(b2)
        h2 = z2 * sig(z2)
        uh2 = SILU_LIP * uz2 + np.abs(h2)
        out = out + h2 @ w3 + b3[0]
        unit = unit + (uh2 + np.abs(h2)) @ np.abs(w3) + np.abs(b3[0])
        ds = lambda z: sig(z) * (1.0 + z * (1.0 - sig(z)))  # noqa: E731
        dh2 = d[:, None] * w3[None, :]
        dz2 = dh2 * ds(z2)
        udz2 = np.abs(dh2) * (np.abs(ds(z2)) + SILU_CURV * uz2) + np.abs(dz2)
        dh1, udh1 = dz2 @ w2, (udz2 + np.abs(dz2)) @ np.abs(w2)
        dz1 = dh1 * ds(z1)
        udz1 = udh1 * np.abs(ds(z1)) + np.abs(dh1) * SILU_CURV * uz1 + np.abs(dz1)
        grads.append(dict(
            dfeat=(dz1 @ w1, (udz1 + np.abs(dz1)) @ np.abs(w1)),
            w1=(dz1.T @ x, (udz1 + np.abs(dz1)).T @ np.abs(x)), b1=(dz1.sum(0), (udz1 + np.abs(dz1)).sum(0)),
            w2=(dz2.T @ h1, (udz2 + np.abs(dz2)).T @ np.abs(h1) + np.abs(dz2).T @ uh1),
            b2=(dz2.sum(0), (udz2 + np.abs(dz2)).sum(0)),
            w3=((d @ h2)[None, :], (np.abs(d) @ (np.abs(h2) + uh2))[None, :]), b3=(d.sum(), np.abs(d).sum())))
    if rp is not None:
        out, unit = rr.seg_sum(out, rp), rr.seg_sum(unit, rp)
    return (out, unit), grads


@pytest.mark.parametrize("bucket", [False, True], ids=["plain", "bucket-deferred"])
@pytest.mark.parametrize("pooled", [False, True], ids=["per-row", "pool"])
def test_wrapper_readout_mlps(cuda, pooled, bucket):
    """ops.readout_mlps per row and with pool= under autograd, 3 readouts of D = 128 over 37 rows: the energies
    and every gradient against the float64 MLP of the same weights (both hidden layers in float64, so the check
    reaches the energies), within K['heads'] first-order units (_mlp_reference)."""
    from x2gnn import ops
    from x2gnn.layers import _mlp

    G, rows, n_seg = 3, int(WRAP_RP[-1]), len(WRAP_RP) - 1
    torch.manual_seed(5)
    mlps = [_mlp(WRAP_D, 1, 3).to(cuda) for _ in range(G)]
    rng = np.random.default_rng(11)
    feats_np = [rng.standard_normal((rows, WRAP_D)).astype(F) for _ in range(G)]
    dout = rng.standard_normal(n_seg if pooled else rows).astype(F)
    feats = [_dev(f, cuda).requires_grad_() for f in feats_np]
    keep = None
    if bucket:
        from x2gnn.dist import GradBucket

        keep = GradBucket([p for m in mlps for p in m.parameters()])
    assert ops.readout_mlps_supported(feats, mlps)
    rpd = _dev(WRAP_RP, cuda)
    out = ops.readout_mlps(feats, mlps, pool=(rpd, n_seg) if pooled else None)
    _backward(bucket, [out], [_dev(dout, cuda).view(-1, 1)])
    params = [[p.detach().cpu().numpy() for p in (m[0].weight, m[0].bias, m[2].weight, m[2].bias, m[4].weight, m[4].bias)]
              for m in mlps]
    (ref, unit), grads = _mlp_reference(feats_np, params, dout, WRAP_RP if pooled else None)
    ck = _Checker("ops.readout_mlps", f"D={WRAP_D} G={G}", f"rows={rows} {'pool' if pooled else 'per-row'} "
                                                             f"{'bucket' if bucket else 'plain'}")
    ck.check("heads", "energies", _with_guard(out.view(-1)), ref.shape[0], (ref, unit))
    for g, m in enumerate(mlps):
        ck.check("heads", "dfeat", _with_guard(feats[g].grad), rows, grads[g]["dfeat"])
        for name, p in (("w1", m[0].weight), ("b1", m[0].bias), ("w2", m[2].weight), ("b2", m[2].bias),
                        ("w3", m[4].weight), ("b3", m[4].bias)):
            ck.check("heads", "d" + name, _with_guard(p.grad), p.shape[0], grads[g][name])
    ck.done()


@pytest.mark.parametrize("seeded", [False, True], ids=["backward-kernel", "unit-seed"])
def test_wrapper_smooth_l1_loss(cuda, seeded):
    """ops.smooth_l1_loss under autograd (the backward kernel, and the forward-written gradient handed back for
    the unit seed) against the reference, 37 elements."""
    from x2gnn import ops

    p, t = rr.loss_inputs(37, 1.0)
    pd = _dev(p, cuda).requires_grad_()
    seed = torch.ones((), device=cuda) if seeded else None
    loss = ops.smooth_l1_loss(pd, _dev(t, cuda), beta=1.0, unit_seed=seed)
    if seeded:
        torch.autograd.backward(loss, seed)
    else:
        loss.backward()
    lref, dref = rr.smooth_l1_mean(p, t, 1.0, 1.0)
    ck = _Checker("ops.smooth_l1_loss", "beta=1.0", f"n=37 {'unit-seed' if seeded else 'backward'}")
    ck.check("loss", "loss", _with_guard(loss.view(1)), 1, lref)
    ck.check("loss", "dpred", _with_guard(pd.grad), 37, dref)
    ck.done()


# ------------------------------------------------------------------------------ the profile
class _StopOnDeviceError:
    """(script mode) A failed bound is a figure to record and the run goes on; a HIP error ends it."""

    @staticmethod
    def pytest_exception_interact(node, call, report):
        if "HIP error" in str(call.excinfo.value):
            node.session.shouldstop = "HIP error: nothing more is launched"


def _write(path):
    """Run every case of this module once and write the figures (module docstring)."""
    t0 = time.time()
    rc = pytest.main([os.path.abspath(__file__), "-m", "gpu", "-q", "-p", "no:cacheprovider"],
                     plugins=[_StopOnDeviceError()])
    wall = time.time() - t0
    rec = sys.modules["test_gpu_readout_fp64"].RECORD  # (the module as pytest imported it)
    f3 = lambda v: float(f"{v:.3e}")  # noqa: E731
    emu = rr.emulation_report()
    head = dict(pytest_exit_code=int(rc), wall_seconds=round(wall, 1), comparisons=len(rec),
                errors="|kernel - ref64| per element; worst err/bound = max over the elements of error / (K * 2^-24 * "
                       "unit); unit 0 requires an exact 0",
                e32=rr.E32,
                families={k: dict(K=rr.K[k], emulation_worst_over_unit=f3(v[0]), emulation_worst_in=f"{v[1]}, {v[2]}",
                                  fixed_against=rr.EMULATION_RATIO[k]) for k, v in sorted(emu.items())})
    worst = {}
    for r in rec:
        worst[r["entry"]] = max(worst.get(r["entry"], 0.0), r["ratio"])
    head["worst_error_over_bound"] = {k: f3(v) for k, v in sorted(worst.items())}
    cols = ["entry", "output", "shape", "family", "comparisons", "elements", "worst err/bound", "worst in: case",
            "abs err there", "bound there"]
    agg = {}
    for r in rec:
        a = agg.setdefault((r["entry"], r["output"], r["shape"]), dict(n=0, el=0, worst=None))
        a["n"] += 1
        a["el"] += r["elements"]
        if a["worst"] is None or r["ratio"] > a["worst"]["ratio"]:
            a["worst"] = r
    rows = [[e, o, s, a["worst"]["family"], a["n"], a["el"], f3(a["worst"]["ratio"]), a["worst"]["case"],
             f3(a["worst"]["abs_err"]), f3(a["worst"]["bound"])] for (e, o, s), a in sorted(agg.items())]
    with open(path, "w") as f:  # one row per line
        f.write("{\n" + "".join(f" {json.dumps(k)}: {json.dumps(v)},\n" for k, v in head.items()))
        f.write(f' "columns": {json.dumps(cols)},\n "rows": [\n' + ",\n".join(json.dumps(r) for r in rows) + "\n]}\n")
    return int(rc)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--write":
        sys.exit("usage: python tests/test_gpu_readout_fp64.py --write profiles/readout_fp64_err.json")
    sys.exit(_write(sys.argv[2]))
