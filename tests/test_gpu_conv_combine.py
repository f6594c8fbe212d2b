"""The conv combine pass (csrc/conv_combine.hip, include/x2g_conv.h) through the raw ABI against its fp64 statement
(tests/conv_combine_ref.py), element by element, at the smallest shapes at which each loop structure changes.

Bound (nothing taken from the code under test): every element has to be finite and within K * 2^-24 * unit of the
fp64 value (conv_combine_ref: the units and how K was fixed against a float32 emulation on the CPU); where the unit
is 0 the kernel has to return exactly 0.  Every output buffer is prefilled with NaN and carries one guard row that
has to stay untouched bit for bit; the workspace is prefilled with NaN and followed by guard floats; inputs are
seeded on the CPU.  The backward gets the fp64 beta rounded to float32 where it is not the forward's own (the
statement's beta, not the kernel's), except in ``test_forward_backward_chain``.
"""
import ctypes

import numpy as np
import pytest
import torch

import conv_combine_ref as cr

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


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _Checker:
    """Compares the outputs of one case with the reference; collects every figure before failing."""

    def __init__(self, case):
        self.case, self.bad, self.worst = case, [], {}

    def check(self, fam, output, buf, rows, ref_unit):
        """``buf``: rows + 1 leading entries, the last one the guard."""
        if not _untouched(buf[rows:]):
            self.bad.append(f"{output}: guard written")
        if rows == 0:
            return
        ref = np.asarray(ref_unit[0], np.float64).reshape(rows, -1)
        unit = np.asarray(ref_unit[1], np.float64).reshape(rows, -1)
        got = buf[:rows].detach().cpu().double().numpy().reshape(rows, -1)
        assert got.shape == ref.shape, (output, got.shape, ref.shape)
        r = cr.ratio(got, ref, unit) / cr.K[fam]
        self.worst[output] = max(r, self.worst.get(output, 0.0))
        if not r <= 1.0:
            self.bad.append(f"{output}: error / bound = {r:.3g} (family {fam})")

    def zero(self, output, buf, rows):
        if not bool((buf[:rows] == 0).all()):
            self.bad.append(f"{output}: not exactly zero")

    def same(self, output, a, b):
        if not torch.equal(_bits(a), _bits(b)):
            self.bad.append(f"{output}: not bitwise equal")

    def untouched(self, output, t):
        if not _untouched(t):
            self.bad.append(f"{output}: written")

    def status(self, output, rc, want=OK):
        if rc != want:
            self.bad.append(f"{output}: status {rc}, expected {want}")

    def done(self):
        assert not self.bad, self.case + "\n" + "\n".join(self.bad)


def _fwd(cuda, attn, x_r, w, rows, H, C, concat, want_beta=True, want_stats=True):
    D = H * C if concat else C
    y, beta, stats = _nan(cuda, rows + 1, D), _nan(cuda, rows + 1), _nan(cuda, rows + 1, 2)
    t = [_dev(a, cuda) for a in (attn, x_r, w)]
    rc = _lib().load().x2g_conv_combine_fwd(_p(t[0]), _p(t[1]), _p(t[2]), rows, H, C, int(concat), _p(y),
                                            _p(beta) if want_beta and w is not None else None,
                                            _p(stats) if want_stats else None, _lib().stream_ptr())
    return rc, y, beta, stats


def _bwd(cuda, dy, attn, x_r, w, beta, rows, H, C, concat, flags=0, dw_old=None, job=None):
    """(rc, d_attn, d_xr, dw, workspace, splits): d_xr is not asked for without x_r."""
    lib = _lib().load()
    D = H * C if concat else C
    d_attn, d_xr, dw = _nan(cuda, rows + 1, H * C), _nan(cuda, rows + 1, D), _nan(cuda, 2, 3 * D)
    if dw_old is not None:
        dw[0] = _dev(dw_old, cuda)
    ws_bytes = int(lib.x2g_conv_combine_bwd_workspace(rows, H, C, int(concat))) if w is not None else 0
    assert ws_bytes == 4 * 3 * D * cr.combine_splits(rows, H * C) * (w is not None)
    ws = _nan(cuda, ws_bytes // 4 + WS_GUARD)
    t = [_dev(a, cuda) for a in (dy, attn, x_r, w, beta)]
    rc = lib.x2g_conv_combine_bwd(_p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), _p(t[4]), rows, H, C, int(concat),
                                  _p(d_attn), _p(d_xr) if x_r is not None else None,
                                  _p(dw) if w is not None else None, flags,
                                  None if job is None else ctypes.cast(ctypes.pointer(job), ctypes.c_void_p),
                                  _p(ws) if ws_bytes else None, ws_bytes, _lib().stream_ptr())
    return rc, d_attn, d_xr, dw, ws, ws_bytes // 4


def _case(cuda, H, C, concat, gated, with_xr, rows, why, regime):
    i = cr.combine_inputs(H, C, concat, rows, regime)
    x, w = (i["x_r"] if with_xr else None), (i["w_beta"] if gated else None)
    ck = _Checker(f"H={H} C={C} concat={concat} gated={gated} x_r={with_xr} rows={rows} ({why}) {regime}")
    ref = cr.combine_fwd(i["attn"], x, w, H, C, concat)
    rc, y, beta, stats = _fwd(cuda, i["attn"], x, w, rows, H, C, concat)
    ck.status("fwd status", rc)
    ck.check("fwd", "y", y, rows, ref["y"])
    ck.check("stats", "row_stats", stats, rows, ref["stats"])
    beta64 = None
    if gated:
        beta64 = ref["beta"][0].astype(F)
        if regime == "saturated":  # finite, 0 or 1 where exp over / underflows; compared through y and the backward
            b, s = beta[:rows].cpu().numpy(), ref["s"][0]
            if not (np.isfinite(b).all() and (b >= 0).all() and (b <= 1).all() and (b[s >= 95] == 1).all()
                    and (b[s <= -95] == 0).all()):
                ck.bad.append("beta: not finite in [0, 1] with exact 0 / 1 at |s| >= 95")
            if not _untouched(beta[rows:]):
                ck.bad.append("beta: guard written")
        else:
            ck.check("fwd", "beta", beta, rows, ref["beta"])
    else:
        ck.untouched("beta", beta)
    refb = cr.combine_bwd(i["dy"], i["attn"], x, w, H, C, concat)
    rc, d_attn, d_xr, dw, ws, n_ws = _bwd(cuda, i["dy"], i["attn"], x, w, beta64, rows, H, C, concat)
    ck.status("bwd status", rc)
    ck.check("bwd", "d_attn", d_attn, rows, refb["d_attn"])
    if with_xr:
        ck.check("bwd", "d_xr", d_xr, rows, refb["d_xr"])
    else:
        ck.untouched("d_xr", d_xr)
    if gated:
        ck.check("dw", "dw_beta", dw, 1, refb["dw"])
        ck.untouched("workspace guard", ws[n_ws:])
        if regime == "equal":
            ck.zero("dw_beta", dw, 1)
    else:
        ck.untouched("dw_beta", dw)
        ck.untouched("workspace", ws)
    ck.done()


def _group(cuda, H, C, pick):
    for case in cr.cases():
        if case[:2] == (H, C) and pick(*case[2:]):
            _case(cuda, *case)


@pytest.mark.parametrize("gated", [True, False], ids=["gated", "skip"])
@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("H,C", cr.HC)
def test_every_row_count(cuda, H, C, concat, gated):
    """Forward (y, beta, row statistics) and backward (d_attn, d_xr, dw_beta) at 1, 3, 63, 64, 65 rows, a workgroup
    pass - 1 / exactly / + 1 and splits x pass + 1 rows."""
    _group(cuda, H, C, lambda c, g, xr, rows, why, regime: (c, g, xr, regime) == (concat, gated, True, "normal"))


@pytest.mark.parametrize("H,C", cr.HC)
def test_mean_without_skip(cuda, H, C):
    """concat=False, root_weight=False: x_r NULL, y = the mean over heads."""
    _group(cuda, H, C, lambda c, g, xr, rows, why, regime: not xr)


@pytest.mark.parametrize("H,C", cr.HC)
def test_regimes(cuda, H, C):
    """|s| reaching 100 with either sign (finite beta of 0 / 1, no NaN), and attn == x_r (exact zeros)."""
    _group(cuda, H, C, lambda c, g, xr, rows, why, regime: regime != "normal")


@pytest.mark.parametrize("W", cr.WIDTHS)
def test_forward_grid_wraps(cuda, W):
    """1024 workgroups x pass + 1 rows: the forward's grid-stride loop takes a second pass of one row."""
    H, C = W // 8, 8
    rows = cr.fwd_wrap_rows(W)
    for concat in (True, False):
        i = cr.combine_inputs(H, C, concat, rows)
        ck = _Checker(f"W={W} concat={concat} rows={rows}")
        ref = cr.combine_fwd(i["attn"], i["x_r"], i["w_beta"], H, C, concat)
        rc, y, beta, stats = _fwd(cuda, i["attn"], i["x_r"], i["w_beta"], rows, H, C, concat)
        ck.status("status", rc)
        ck.check("fwd", "y", y, rows, ref["y"])
        ck.check("fwd", "beta", beta, rows, ref["beta"])
        ck.check("stats", "row_stats", stats, rows, ref["stats"])
        ck.done()


@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("H,C", cr.HC)
def test_flags(cuda, H, C, concat):
    """X2G_ACCUM_WGRAD onto non-zero old contents (unit plus |old|); the deferred form summed by x2g_slab_sum_batch,
    bitwise the immediate form (plain and accumulating); rows == 0."""
    lib, L = _lib().load(), _lib()
    W, D = H * C, (H * C if concat else C)
    for rows in (cr.combine_tile(W) + 1, cr.COMBINE_SPLITS * cr.combine_tile(W) + 1):
        i = cr.combine_inputs(H, C, concat, rows)
        ck = _Checker(f"H={H} C={C} concat={concat} rows={rows}")
        beta = cr.combine_fwd(i["attn"], i["x_r"], i["w_beta"], H, C, concat)["beta"][0].astype(F)
        args = (cuda, i["dy"], i["attn"], i["x_r"], i["w_beta"], beta, rows, H, C, concat)
        assert int(lib.x2g_conv_combine_splits(rows, W)) == cr.combine_splits(rows, W)
        rc, _, _, dw_plain, _, _ = _bwd(*args)
        ck.status("plain", rc)
        rc, _, _, dw_acc, _, _ = _bwd(*args, flags=ACCUM, dw_old=i["dw_old"])
        ck.status("accum", rc)
        ck.check("dw", "dw_beta accum", dw_acc, 1, cr.combine_bwd(i["dy"], i["attn"], i["x_r"], i["w_beta"], H, C,
                                                                 concat, i["dw_old"])["dw"])
        for flags, old, want in ((DEFER, None, dw_plain), (DEFER | ACCUM, i["dw_old"], dw_acc)):
            job = L.STRUCTS["x2g_slab_job"]()
            rc, d_attn, d_xr, dw, ws, n_ws = _bwd(*args, flags=flags, dw_old=old, job=job)
            ck.status("deferred", rc)
            if old is None:
                ck.untouched("dw_beta before the deferred sum", dw)
            if (job.n_w, job.n_b, job.splits, job.dw, job.part_w) != (3 * D, 0, cr.combine_splits(rows, W),
                                                                      dw.data_ptr(), ws.data_ptr()):
                ck.bad.append("slab job fields")
            jobs = (L.STRUCTS["x2g_slab_job"] * 1)(job)
            ck.status("slab sum", lib.x2g_slab_sum_batch(ctypes.cast(jobs, ctypes.c_void_p), 1,
                                                         1 if flags & ACCUM else 0, L.stream_ptr()))
            ck.same("dw_beta deferred", dw[:1], want[:1])
            ck.untouched("dw_beta guard", dw[1:])
            ck.untouched("workspace guard", ws[n_ws:])
        ck.status("deferred without a job", _bwd(*args, flags=DEFER)[0], EINVAL)
        ck.done()
    # rows == 0: dw zeroed (accumulating: left alone), nothing else written; the deferred form is refused
    i = cr.combine_inputs(H, C, concat, 1)
    ck = _Checker(f"H={H} C={C} concat={concat} rows=0")
    args = (cuda, i["dy"], i["attn"], i["x_r"], i["w_beta"], np.full(1, 0.5, F), 0, H, C, concat)  # (one-row buffers)
    rc, d_attn, d_xr, dw, ws, _ = _bwd(*args)
    ck.status("rows=0", rc)
    ck.zero("dw_beta at rows=0", dw, 1)
    ck.untouched("dw guard", dw[1:])
    ck.untouched("d_attn", d_attn)
    ck.untouched("d_xr", d_xr)
    rc, _, _, dw, _, _ = _bwd(*args, flags=ACCUM, dw_old=i["dw_old"])
    ck.status("rows=0 accum", rc)
    ck.same("dw_beta kept", dw[:1], _dev(i["dw_old"], cuda)[None])
    ck.status("rows=0 deferred", _bwd(*args, flags=DEFER, job=L.STRUCTS["x2g_slab_job"]())[0], EINVAL)
    rc, y, beta, stats = _fwd(cuda, i["attn"], i["x_r"], i["w_beta"], 0, H, C, concat)
    ck.status("fwd rows=0", rc)
    for name, t in (("y", y), ("beta", beta), ("stats", stats)):
        ck.untouched(name, t)
    ck.done()


def test_status_codes(cuda):
    """An uncompiled width: X2G_EUNSUPPORTED; NULL attn, w_beta with NULL x_r, negative rows: X2G_EINVAL; nothing
    is written in any of them."""
    lib, st = _lib().load(), _lib().stream_ptr()
    rows = 9
    ck = _Checker("status codes")
    for H, C, concat, null_attn, null_xr, n, want in (
            (12, 8, True, False, False, rows, EUNSUPPORTED), (16, 6, False, False, False, rows, EUNSUPPORTED),
            (16, 32, True, False, False, rows, EUNSUPPORTED), (4, 4, True, False, False, rows, EUNSUPPORTED),
            (16, 8, True, True, False, rows, EINVAL), (16, 8, True, False, True, rows, EINVAL),
            (16, 8, False, False, True, rows, EINVAL), (16, 8, True, False, False, -1, EINVAL)):
        W, D = H * C, (H * C if concat else C)
        a, x, w = _nan(cuda, rows, W), _nan(cuda, rows, D), _nan(cuda, 3 * D)
        y, beta, stats = _nan(cuda, rows + 1, D), _nan(cuda, rows + 1), _nan(cuda, rows + 1, 2)
        rc = lib.x2g_conv_combine_fwd(None if null_attn else _p(a), None if null_xr else _p(x), _p(w), n, H, C,
                                      int(concat), _p(y), _p(beta), _p(stats), st)
        ck.status(f"fwd H={H} C={C} attn={not null_attn} x_r={not null_xr} rows={n}", rc, want)
        dy, d_attn, d_xr, dw = _nan(cuda, rows, D), _nan(cuda, rows + 1, W), _nan(cuda, rows + 1, D), _nan(cuda, 3 * D)
        ws = _nan(cuda, 3 * D * 128)
        rc = lib.x2g_conv_combine_bwd(_p(dy), None if null_attn else _p(a), None if null_xr else _p(x), _p(w),
                                      _p(beta), n, H, C, int(concat), _p(d_attn), _p(d_xr), _p(dw), 0, None, _p(ws),
                                      ws.numel() * 4, st)
        ck.status(f"bwd H={H} C={C} attn={not null_attn} x_r={not null_xr} rows={n}", rc, want)
        for name, t in (("y", y), ("beta", beta), ("stats", stats), ("d_attn", d_attn), ("d_xr", d_xr), ("dw", dw),
                        ("ws", ws)):
            ck.untouched(f"{name} after status {want}", t)
    big = 2 ** 31 // (128 * 4)  # rows x width x 4 bytes = 2^31: refused at the ABI, before any launch
    a, y = _nan(cuda, 8, 128), _nan(cuda, 8, 128)
    ck.status("rows x width x 4 = 2^31", lib.x2g_conv_combine_fwd(_p(a), None, None, big, 16, 8, 1, _p(y), None, None,
                                                                  st), EUNSUPPORTED)
    ck.untouched("y", y)
    ck.done()


def test_forward_backward_chain(cuda):
    """The backward fed the forward's own float32 beta and a w_beta at a 4-byte offset (a parameter inside a flat
    buffer), twice: the same bits both times, within the bound."""
    H, C, concat, rows = 16, 8, True, 1025
    i = cr.combine_inputs(H, C, concat, rows)
    ck = _Checker("forward -> backward")
    flat = torch.zeros(3 * H * C + 1, device=cuda)
    flat[1:] = _dev(i["w_beta"], cuda)
    lib, st = _lib().load(), _lib().stream_ptr()
    a, x, dy = (_dev(i[k], cuda) for k in ("attn", "x_r", "dy"))
    outs = []
    for _ in range(2):
        y, beta = _nan(cuda, rows + 1, H * C), _nan(cuda, rows + 1)
        d_attn, d_xr, dw = _nan(cuda, rows + 1, H * C), _nan(cuda, rows + 1, H * C), _nan(cuda, 2, 3 * H * C)
        ws = _nan(cuda, 3 * H * C * 128 + WS_GUARD)
        w = ctypes.c_void_p(flat.data_ptr() + 4)
        ck.status("fwd", lib.x2g_conv_combine_fwd(_p(a), _p(x), w, rows, H, C, 1, _p(y), _p(beta), None, st))
        ck.status("bwd", lib.x2g_conv_combine_bwd(_p(dy), _p(a), _p(x), w, _p(beta), rows, H, C, 1, _p(d_attn),
                                                  _p(d_xr), _p(dw), 0, None, _p(ws), 3 * H * C * 128 * 4, st))
        outs.append((y, beta, d_attn, d_xr, dw))
    for u, v in zip(*outs):
        ck.same("two runs", u, v)
    ref = cr.combine_fwd(i["attn"], i["x_r"], i["w_beta"], H, C, concat)
    refb = cr.combine_bwd(i["dy"], i["attn"], i["x_r"], i["w_beta"], H, C, concat)
    y, beta, d_attn, d_xr, dw = outs[0]
    ck.check("fwd", "y", y, rows, ref["y"])
    ck.check("bwd", "d_attn", d_attn, rows, refb["d_attn"])
    ck.check("bwd", "d_xr", d_xr, rows, refb["d_xr"])
    ck.check("dw", "dw_beta", dw, 1, refb["dw"])
    ck.done()
