"""SBFTransformerConv's output combine (csrc/conv_combine.hip, include/x2g_conv.h) stated in float64 on the CPU,
each value with its *unit*, and a numpy-float32 emulation that fixes the bound's constants.

Values (numpy float64; nothing from x2gnn; the statement is the reference's sbftransformer_conv.py:115-127):

    m    = attn                     (concat)   or   attn.view(H, C).mean(heads)                 [rows, Dout]
    s    = w1 . m + w2 . x_r + w3 . (m - x_r),   beta = 1 / (1 + exp(-s)),   w_beta = [w1, w2, w3]
    y    = beta x_r + (1 - beta) m  (gated)    or   m + x_r   (x_r None: m)
    row statistics (mean_c y, sum_c (y_c - mean)^2)
    dbeta = sum_c dy_c (x_r - m)_c,  ds = dbeta beta (1 - beta),  dm = dy (1 - beta) + ds (w1 + w3),
    d_xr = dy beta + ds (w2 - w3),  d_attn = dm (/ H, broadcast over heads),  dw_beta = sum_e ds_e [m, x_r, m - x_r]

Every input is the float32 array the kernel gets, widened to float64.

Units.  Every function returns (value, unit) pairs: the unit is the float64 sum of the magnitudes of the terms that
make the value up.  With um = mean_h |attn_h| (= |m| for concat: the unit of m) and slack = um - |m| (what a
cancelling mean over heads can lose; 0 for concat):

    unit(m - x_r) = |m - x_r| + slack
    unit(s)       = sum_c |w1| um + |w2| |x_r| + |w3| unit(m - x_r)          (concat: sum |w| |operand|)
    unit(beta)    = beta (1 - beta) unit(s) + beta + 2^-102
                    (2^-102 = 2^-126 / 2^-24: exp(-s) overflows float32 only where the exact beta is below the
                    smallest normal number 2^-126, and the kernel's 0 there is off by less than that; the term
                    is the format's underflow threshold, 1e-31 of a unit of any beta that is not underflowing)
    unit(1 - beta) = unit(beta) + (1 - beta)      (1 - beta is formed from the rounded beta: near beta = 1 its error
                                                   is beta's, not relative to the tiny difference)
    unit(y)       = |beta x_r| + (1 - beta) um + unit(m - x_r) unit(beta)     (no gate: um + |x_r|)
    unit(mean)    = mean_c unit(y_c),   unit(M2) = sum_c 2 |y_c - mean| (unit(y_c) + unit(mean)) + (y_c - mean)^2
    unit(dbeta)   = sum_c |dy_c| unit(m - x_r)_c
    unit(g')      = unit(beta) (1 - beta) + beta unit(1 - beta),  g' = beta (1 - beta)
    unit(ds)      = unit(dbeta) g' + |dbeta| unit(g')
    unit(dm)      = |dy| unit(1 - beta) + unit(ds) (|w1| + |w3|),   unit(d_attn) = unit(dm) / H
    unit(d_xr)    = |dy| unit(beta) + unit(ds) (|w2| + |w3|)
    unit(dw_beta) = sum_e unit(ds_e) [um, |x_r|, unit(m - x_r)]   (+ |old| when added onto old contents)

A kernel passes when its value is finite and |kernel - ref64| <= K * 2^-24 * unit; there is no absolute floor, and
where the unit is exactly 0 the kernel has to return exactly 0 (attn == x_r with concat: dbeta, ds and all of
dw_beta).

K per family is fixed against the emulation below (``emu_*``: numpy float32, float32 ``exp``, every sum sequential
in head / channel / row order), measured against the float64 statement and never against a kernel: the emulation's
worst error / (2^-24 unit) over the shapes of tests/test_gpu_conv_combine.py (``cases`` at the end of this module),
times 4, rounded up to a power of two.  4x because the kernels sum in another order (a butterfly over lanes,
per-slot partials, LDS fold, slab sum, fma contraction), which can cost a small multiple of a sequential sum's
error but not more.  ``emulation_report`` measures the ratios; tests/test_conv_combine_ref.py asserts that each stays
at or below EMULATION_RATIO and that 4 * EMULATION_RATIO <= K:

    family   worst emulation ratio (output, case)                                        x 4     K
    fwd      3.23  (beta, H = 8, C = 16, concat, 1025 rows: the 384-term sequential s)      12.9    16
    bwd      3.26  (dbeta, H = 4, C = 8, concat, 4097 rows: the 32-term sequential sum)     13.0    16
    dw       0.62  (dw_beta, H = 4, C = 8, concat, one row: unit(ds) is several |ds|)        2.5     4
    stats    3.05  (M2, H = 8, C = 16, concat, 1025 rows, attn == x_r)                      12.2    16

In the ``saturated`` regime (|s| reaching 100) beta itself is asserted finite, in [0, 1] and exactly 0 or 1 where
|s| >= 95 (float32's exp over- or underflows there), and compared through y and the backward, whose units carry
unit(beta); its own ratio is left out of the report there.
"""
import functools

import numpy as np

E32 = 2.0 ** -24
TINY = 2.0 ** -126 / E32  # float32's smallest normal number, in units: see unit(beta)
F = np.float32
# worst |emulation - ref64| / (2^-24 unit) per family over the GPU test's shapes, rounded up (emulation_report)
EMULATION_RATIO = dict(fwd=3.3, bwd=3.3, dw=0.7, stats=3.1)
K = dict(fwd=16.0, bwd=16.0, dw=4.0, stats=16.0)


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


# ------------------------------------------------------------------------------------------------ values, units
def _mean_heads(attn, H, C, concat):
    """(m, um): the row the combine works on and its unit."""
    a = _f64(attn)
    if concat:
        return a, np.abs(a)
    a = a.reshape(a.shape[0], H, C)
    return a.mean(1), np.abs(a).mean(1)


def _gate(m, um, x, w):
    """s, beta and their units (w: float64 [3 Dout])."""
    D = m.shape[1]
    w1, w2, w3 = w[:D], w[D:2 * D], w[2 * D:]
    diff, udiff = m - x, np.abs(m - x) + (um - np.abs(m))
    s = m @ w1 + x @ w2 + diff @ w3
    us = um @ np.abs(w1) + np.abs(x) @ np.abs(w2) + udiff @ np.abs(w3)
    with np.errstate(over="ignore"):
        beta = 1.0 / (1.0 + np.exp(-s))
        omb = 1.0 / (1.0 + np.exp(s))  # 1 - beta without the cancellation
    ub = beta * omb * us + beta + TINY
    return dict(w1=w1, w2=w2, w3=w3, diff=diff, udiff=udiff, s=s, us=us, beta=beta, omb=omb, ub=ub, uomb=ub + omb)


def combine_fwd(attn, x_r, w_beta, H, C, concat):
    """dict(y, beta (gated only), s (gated only), stats) of (value, unit)."""
    m, um = _mean_heads(attn, H, C, concat)
    x = _f64(x_r)
    out = {}
    if w_beta is not None:
        g = _gate(m, um, x, _f64(w_beta))
        b, omb = g["beta"][:, None], g["omb"][:, None]
        y = b * x + omb * m
        uy = np.abs(b * x) + omb * um + g["udiff"] * g["ub"][:, None]
        out["beta"], out["s"] = (g["beta"], g["ub"]), (g["s"], g["us"])
    elif x is not None:
        y, uy = m + x, um + np.abs(x)
    else:
        y, uy = m, um
    mu, umu = y.mean(1), uy.mean(1)
    d = y - mu[:, None]
    m2 = (d * d).sum(1)
    um2 = (2 * np.abs(d) * (uy + umu[:, None]) + d * d).sum(1)
    out["y"] = (y, uy)
    out["stats"] = (np.stack([mu, m2], 1), np.stack([umu, um2], 1))
    return out


def combine_bwd(dy, attn, x_r, w_beta, H, C, concat, dw_old=None):
    """dict(d_attn, d_xr, dw (gated only), dbeta, ds (gated only)) of (value, unit)."""
    g_ = _f64(dy)
    rows = g_.shape[0]
    Hh = 1 if concat else H

    def bcast(v):
        return v if concat else np.broadcast_to((v / Hh)[:, None, :], (rows, H, C)).reshape(rows, H * C)

    if w_beta is None:
        return dict(d_attn=(bcast(g_), bcast(np.abs(g_))), d_xr=(g_, np.abs(g_)))
    m, um = _mean_heads(attn, H, C, concat)
    x = _f64(x_r)
    q = _gate(m, um, x, _f64(w_beta))
    beta, omb, ub, uomb = q["beta"], q["omb"], q["ub"], q["uomb"]
    dbeta = -(g_ * q["diff"]).sum(1)
    udbeta = (np.abs(g_) * q["udiff"]).sum(1)
    gp, ugp = beta * omb, ub * omb + beta * uomb
    ds, uds = dbeta * gp, udbeta * gp + np.abs(dbeta) * ugp
    w1, w2, w3 = q["w1"], q["w2"], q["w3"]
    dm = g_ * omb[:, None] + ds[:, None] * (w1 + w3)[None, :]
    udm = np.abs(g_) * uomb[:, None] + uds[:, None] * (np.abs(w1) + np.abs(w3))[None, :]
    dxr = g_ * beta[:, None] + ds[:, None] * (w2 - w3)[None, :]
    udxr = np.abs(g_) * ub[:, None] + uds[:, None] * (np.abs(w2) + np.abs(w3))[None, :]
    dw = np.concatenate([ds @ m, ds @ x, ds @ q["diff"]])
    udw = np.concatenate([uds @ um, uds @ np.abs(x), uds @ q["udiff"]])
    if dw_old is not None:
        dw, udw = dw + _f64(dw_old), udw + np.abs(_f64(dw_old))
    return dict(d_attn=(bcast(dm), bcast(udm)), d_xr=(dxr, udxr), dw=(dw, udw), dbeta=(dbeta, udbeta), ds=(ds, uds))


# ------------------------------------------------------------------------------------------------ float32 emulation
def _fma(a, b, c):
    """fma in float32: the product exact (float64 holds it), one rounding of the sum (to float64, then float32)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def _seq(v, axis=0):
    """Sequential float32 sum along an axis (cumsum accumulates in order)."""
    v = np.asarray(v, F)
    if v.shape[axis] == 0:
        return np.zeros(np.delete(v.shape, axis).astype(int), F)
    return np.take(np.cumsum(v, axis=axis, dtype=F), -1, axis=axis)


def _emu_m(attn, H, C, concat):
    a = np.asarray(attn, F)
    if concat:
        return a
    return _seq(a.reshape(a.shape[0], H, C), axis=1) * F(1.0 / H)


def _emu_beta(m, x, w):
    D = m.shape[1]
    d = m - x
    terms = np.stack([w[None, :D] * m, w[None, D:2 * D] * x, w[None, 2 * D:] * d], 2).reshape(m.shape[0], 3 * D)
    s = _seq(terms, axis=1)
    with np.errstate(over="ignore"):
        return (F(1) / (F(1) + np.exp(-s, dtype=F))).astype(F)


def emu_fwd(attn, x_r, w_beta, H, C, concat):
    """dict(y, beta (gated), stats) in float32."""
    m = _emu_m(attn, H, C, concat)
    out = {}
    if w_beta is not None:
        x = np.asarray(x_r, F)
        b = _emu_beta(m, x, np.asarray(w_beta, F))
        y = b[:, None] * x + (F(1) - b)[:, None] * m
        out["beta"] = b
    elif x_r is not None:
        y = m + np.asarray(x_r, F)
    else:
        y = m
    mu = _seq(y, axis=1) * F(1.0 / y.shape[1])
    d = y - mu[:, None]
    out["y"], out["stats"] = y, np.stack([mu, _seq(d * d, axis=1)], 1)
    return out


def emu_bwd(dy, attn, x_r, w_beta, H, C, concat, dw_old=None):
    g = np.asarray(dy, F)
    rows = g.shape[0]
    Hh = 1 if concat else H

    def bcast(v):
        return v if concat else np.broadcast_to((v * F(1.0 / Hh))[:, None, :], (rows, H, C)).reshape(rows, H * C)

    if w_beta is None:
        return dict(d_attn=bcast(g), d_xr=g)
    m, x, w = _emu_m(attn, H, C, concat), np.asarray(x_r, F), np.asarray(w_beta, F)
    D = m.shape[1]
    b = _emu_beta(m, x, w)
    dbeta = _seq(g * (x - m), axis=1)
    ds = dbeta * (b * (F(1) - b))
    dm = g * (F(1) - b)[:, None] + ds[:, None] * (w[:D] + w[2 * D:])[None, :]
    dxr = g * b[:, None] + ds[:, None] * (w[D:2 * D] - w[2 * D:])[None, :]
    dw = _seq(ds[:, None] * np.concatenate([m, x, m - x], 1), axis=0)
    if dw_old is not None:
        dw = dw + np.asarray(dw_old, F)
    return dict(d_attn=bcast(dm), d_xr=dxr, dw=dw, dbeta=dbeta, ds=ds)


# ------------------------------------------------------------------------------------------------ shapes, inputs
HC = ((16, 8), (8, 16), (32, 4), (4, 8), (8, 8), (16, 16))  # (heads, channels): widths 128, 128, 128, 32, 64, 256
WIDTHS = (32, 64, 128, 256)
COMBINE_SPLITS, COMBINE_FWD_GRID = 128, 1024  # kCombineSplits, kCombineFwdGrid
REGIMES = ("normal", "saturated", "equal")


def combine_tile(W):
    """Rows per workgroup pass of both kernels: RPB = 256 / LPR row slots, LPR = W / 4 lanes per row."""
    return 256 // (W // 4)


def combine_splits(rows, W):
    """x2g_conv_combine_splits: one partial slab per workgroup, a workgroup per tile up to 128."""
    return 0 if rows <= 0 else max(1, min(COMBINE_SPLITS, -(-rows // combine_tile(W))))


def combine_rows(W):
    """(rows, boundary): a workgroup pass - 1, exactly, + 1 (at W = 32 the 32-row pass sits between 3 and 63);
    splits x tile + 1: the backward's grid-stride loop wraps and workgroup 0's second pass holds one row."""
    t = combine_tile(W)
    rows = {1: "one-row", 3: "three-rows", 63: "63", 64: "64", 65: "65"}
    rows.update({t - 1: "wg-1", t: "wg", t + 1: "wg+1", COMBINE_SPLITS * t + 1: "bwd-wraps-one-row"})
    return sorted((r, why) for r, why in rows.items() if r > 0)


def fwd_wrap_rows(W):
    """The forward's grid cap: 1024 workgroups x tile + 1 rows, workgroup 0 takes a second pass of one row."""
    return COMBINE_FWD_GRID * combine_tile(W) + 1


def combine_inputs(H, C, concat, rows, regime="normal", seed=0):
    """Seeded float32 inputs: attn [rows, H*C], x_r [rows, Dout], w_beta [3 Dout], dy [rows, Dout], dw_old.
    ``saturated``: w_beta scaled so that s reaches +100 on some row and -100 on another (one row: |s| = 100);
    ``equal``: x_r == attn (concat only)."""
    D = H * C if concat else C
    rng = np.random.default_rng(100003 * H + 1009 * C + 17 * rows + 5 * bool(concat) + seed)
    nrm = lambda *s: rng.standard_normal(s).astype(F)  # noqa: E731
    i = dict(attn=nrm(rows, H * C), x_r=nrm(rows, D), w_beta=nrm(3 * D) / F(np.sqrt(3 * D)), dy=nrm(rows, D),
             dw_old=nrm(3 * D))
    if regime == "equal":
        assert concat
        i["x_r"] = i["attn"].copy()
    elif regime == "saturated":
        s = combine_fwd(i["attn"], i["x_r"], i["w_beta"], H, C, concat)["s"][0]
        reach = min(s.max(), -s.min()) if s.max() > 0 > s.min() else np.abs(s).max()
        i["w_beta"] = (i["w_beta"] * F(100.5 / reach)).astype(F)
    return i


def cases():
    """(H, C, concat, gated, with_xr, rows, boundary, regime) of tests/test_gpu_conv_combine.py: every (H, C) x
    concat x gate at every row count; no x_r at all with concat=False; the regimes at 65 rows and at the wrap."""
    out = []
    for H, C in HC:
        W = H * C
        for concat in (True, False):
            for gated in (True, False):
                for rows, why in combine_rows(W):
                    out.append((H, C, concat, gated, True, rows, why, "normal"))
                if gated:
                    for rows in (65, COMBINE_SPLITS * combine_tile(W) + 1):
                        out.append((H, C, concat, True, True, rows, "regime", "saturated"))
                        if concat:
                            out.append((H, C, True, True, True, rows, "regime", "equal"))
        for rows, why in combine_rows(W):
            out.append((H, C, False, False, False, rows, why, "normal"))
    return out


# ------------------------------------------------------------------------------------------------ the report
def ratio(got, ref, unit):
    """Worst |got - ref| / (2^-24 unit); an element with unit 0 has to be exactly 0 (inf otherwise)."""
    got, ref, unit = np.asarray(got, np.float64), np.asarray(ref), np.asarray(unit)
    err = np.abs(got - ref)
    if not np.isfinite(got).all():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(unit > 0, err / (E32 * unit), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


FAMILY = dict(y="fwd", beta="fwd", stats="stats", d_attn="bwd", d_xr="bwd", dbeta="bwd", ds="bwd", dw="dw")


@functools.lru_cache(maxsize=None)
def emulation_report():
    """{family: (worst emulation error / (2^-24 unit), output, case)} over the GPU test's shapes."""
    worst = {}
    for H, C, concat, gated, with_xr, rows, why, regime in cases():
        i = combine_inputs(H, C, concat, rows, regime)
        x, w = (i["x_r"] if with_xr else None), (i["w_beta"] if gated else None)
        case = f"H={H} C={C} concat={concat} gated={gated} x_r={with_xr} rows={rows} {regime}"
        ref, emu = combine_fwd(i["attn"], x, w, H, C, concat), emu_fwd(i["attn"], x, w, H, C, concat)
        pairs = [(ref, emu)]
        for old in (None, i["dw_old"]):  # (plain, and added onto old contents: X2G_ACCUM_WGRAD)
            pairs.append((combine_bwd(i["dy"], i["attn"], x, w, H, C, concat, old),
                          emu_bwd(i["dy"], i["attn"], x, w, H, C, concat, old)))
        for r, e in pairs:
            for k in e:
                if k == "beta" and regime == "saturated":
                    continue  # (compared through y and the backward there: a float32 beta stops at 0 / 1)
                v = ratio(e[k], *r[k])
                if v > worst.get(FAMILY[k], (-1.0,))[0]:
                    worst[FAMILY[k]] = (v, k, case)
    return worst
