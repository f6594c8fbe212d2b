"""The K-target readout heads and the per-target error statistics (csrc/readout_multi.hip, include/x2g_multi.h)
stated in float64 on the CPU, each value with its *unit*, exactly as tests/readout_ref.py states the K = 1 heads
(its helpers are imported, its rule is this module's).

Values (numpy float64; nothing from x2gnn; the statements are include/x2g_multi.h's comments):
``heads_k``       out[r, k] = sum_g (h_g[r, :] . w_g[k, :] + b_g[k])          hs[g] [R, D], ws[g] [K, D], bs[g] [K] / None
``heads_k_pool``  its sum over the rows of each segment                      -> [S, K]
``heads_k_bwd``   per group dh [R, D] = d w_g, dw [K, D] = d^T h_g, db [K] = column sums of d, with d = dout per
                  row, or per segment with ``seg_rowptr``
``error_cols``    per target k: sum_i |d|, sum_i d^2, max_i |d|, n with d = pred[i, k] - target[i, k] rounded to
                  float32 first (as torch forms it), everything after in float64

Units and the pass rule are readout_ref's: the unit of a value is the float64 sum of the magnitudes of the terms
that make it up (out[r, k]: sum_g (|h_g[r]| . |w_g[k]| + |b_g[k]|); dh: |d| |w| summed over the targets; dw[k, c]:
sum_r |d[r, k]| |h[r, c]|; onto old contents: plus |old|); a kernel passes when its value is finite and
|kernel - ref64| <= K_BOUND[family] * 2^-24 * unit, no absolute floor, and a zero unit requires an exact zero.

K_BOUND per family is fixed against the numpy-float32 emulation below (``emu_*``: every sum sequential, in
channel, group, target and row order), measured against the float64 statement and never against a kernel: the
emulation's worst error / (2^-24 unit) over the shapes of tests/test_gpu_readout_multi.py (the case lists at the end
of this module), times 4 for the kernels' other summation order (chunk dot products, lane butterflies, per-slot
partials, the LDS fold, the slab sum, fma contraction), rounded up to a power of two.  ``emulation_report`` measures
the ratios; tests/test_readout_multi_ref.py asserts that each stays at or below EMULATION_RATIO and that
4 * EMULATION_RATIO <= K_BOUND:

    family        worst emulation ratio (output, case)                                      x 4      K_BOUND
    heads_k       5.40   (pooled heads, D = 4, K = 12, G = 1: the 300-row segment)           21.6     32
    heads_k_seg   255.28 (db from per-segment dout, D = 4, K = 12, G = 5, 1070 rows)         1021.2   1024

``heads_k`` is every output but dw / db of the backward from a per-segment dout, which are ``heads_k_seg``.  That
family's bound is far above the K = 1 family's 32 (readout_ref's own report runs the backward from per-row dout
only): with dout per segment every row of a 300-row segment adds the SAME value to db, and a sequential float32 sum
of equal addends rounds the same way at every step once the running total outgrows the addend, so the errors add
up instead of cancelling (a row-order sum of 1070 such terms is 255 units off, where 1070 terms of random sign
stay near 5).  The rule is kept as it stands rather than fitted to the kernel, whose per-slot partials make it
much more accurate than that; a wrong segment or a dropped row is an error of the order of the unit itself, 2^24
of these, and is caught all the same.

The error statistics carry tests/test_gpu_metrics.py's bound, which needs no emulation: every term is
non-negative and each of the at most n float64 additions rounds once, so |got - ref| <= n * 2^-52 * ref for the two
sums; the maximum and the count are exact.
"""
import functools

import numpy as np

import readout_ref as rr
from readout_ref import E32, F, _f64, _seq, _seq_seg, owner_of, ragged_rowptr, seg_sum  # noqa: F401

EMULATION_RATIO = dict(heads_k=5.4, heads_k_seg=255.3)
K_BOUND = dict(heads_k=32.0, heads_k_seg=1024.0)


# ------------------------------------------------------------------------------------------------ values, units
def heads_k(hs, ws, bs):
    """(out [R, K], unit): out[r, k] = sum_g (h_g[r] . w_g[k] + b_g[k])."""
    out = unit = 0.0
    for h, w, b in zip(hs, ws, bs):
        out = out + _f64(h) @ _f64(w).T + (0.0 if b is None else _f64(b)[None, :])
        unit = unit + np.abs(_f64(h)) @ np.abs(_f64(w)).T + (0.0 if b is None else np.abs(_f64(b))[None, :])
    return out, unit


def heads_k_pool(hs, ws, bs, seg_rowptr):
    v, u = heads_k(hs, ws, bs)
    return seg_sum(v, seg_rowptr), seg_sum(u, seg_rowptr)


def heads_k_bwd(dout, hs, ws, seg_rowptr=None):
    """[dict(dh, dw, db) of (value, unit) per group]; ``seg_rowptr``: dout [S, K] is given per segment of rows."""
    d = _f64(dout)
    if seg_rowptr is not None:
        d = d[owner_of(seg_rowptr)]
    res = []
    for h, w in zip(hs, ws):
        h, w = _f64(h), _f64(w)
        res.append(dict(dh=(d @ w, np.abs(d) @ np.abs(w)), dw=(d.T @ h, np.abs(d).T @ np.abs(h)),
                        db=(d.sum(0), np.abs(d).sum(0))))
    return res


def error_cols(pred, target):
    """[K, 4] float64: sum |d|, sum d^2, max |d|, n per column, d = pred - target rounded to float32 first."""
    d = np.asarray(pred, F) - np.asarray(target, F)
    assert d.dtype == F and d.ndim == 2
    a = np.abs(d).astype(np.float64)
    return np.stack([a.sum(0), (a * a).sum(0), a.max(0), np.full(d.shape[1], float(d.shape[0]))], axis=1)


# ------------------------------------------------------------------------------------------------ float32 emulation
def emu_heads_k(hs, ws, bs):
    R, K = np.asarray(hs[0]).shape[0], np.asarray(ws[0]).shape[0]
    out = np.zeros((R, K), F)
    for h, w, b in zip(hs, ws, bs):
        h, w = np.asarray(h, F), np.asarray(w, F)
        for k in range(K):
            d = _seq(h * w[k][None, :], axis=1)
            out[:, k] = out[:, k] + (d + (F(b[k]) if b is not None else F(0)))
    return out


def emu_heads_k_pool(hs, ws, bs, seg_rowptr):
    return _seq_seg(emu_heads_k(hs, ws, bs), seg_rowptr)


def emu_heads_k_bwd(dout, hs, ws, seg_rowptr=None):
    d = np.asarray(dout, F)
    if seg_rowptr is not None:
        d = d[owner_of(seg_rowptr)]
    res = []
    for h, w in zip(hs, ws):
        h, w = np.asarray(h, F), np.asarray(w, F)
        dh = np.zeros(h.shape, F)
        for k in range(w.shape[0]):  # targets in order
            dh = dh + d[:, k:k + 1] * w[k][None, :]
        dw = np.stack([_seq(d[:, k:k + 1] * h, axis=0) for k in range(w.shape[0])])
        res.append(dict(dh=dh, dw=dw, db=_seq(d, axis=0)))
    return res


# ------------------------------------------------------------------------------------------------ shapes, inputs
KS = (1, 2, 5, 12, 16)
DS = (4, 16, 128, 256)  # 1, 4, 32, 64 lanes per row
GS = (1, 5, 8)
ERR_N, ERR_K = (1, 255, 256, 257, 4099), (1, 12)


def fwd_tile(D):
    """Rows per workgroup pass of heads_k_fwd_kernel: 4 waves x RPW (64 / LPR) x U (2)."""
    return 2 * rr.head_tile(D)


def fwd_cases():
    """(D, K, G, rows, boundary): every (D, K) at 1 row and one less / one more than a workgroup's rows, the group
    count cycling through GS; per D one row more than 2048 workgroups cover in one pass."""
    out = []
    for a, D in enumerate(DS):
        t = fwd_tile(D)
        for b, K in enumerate(KS):
            for c, (rows, why) in enumerate(((1, "rows=1"), (t - 1, "wg-1"), (t, "wg"), (t + 1, "wg+1"))):
                out.append((D, K, GS[(a + b + c) % 3], rows, why))
        out.append((D, 2, 1, 2048 * t + 1, "past-grid-cap"))
    return out


def pool_cases():
    """(D, K, G): every (D, K) over readout_ref.ragged_rowptr(head_tile(D), big=300), the group count cycling."""
    return [(D, K, GS[(a + b) % 3]) for a, D in enumerate(DS) for b, K in enumerate(KS)]


def bwd_cases():
    """(D, K, G, rows): every D at every row count of readout_ref.HEAD_BWD_ROWS, K and G cycling; at 8191 rows and
    more the wide heads run fewer targets and one group (the float64 statement's size, not the kernel's)."""
    out = []
    for a, D in enumerate(DS):
        for b, rows in enumerate(rr.HEAD_BWD_ROWS):
            K, G = KS[(a + b) % 5], GS[(a + b) % 3]
            if rows >= 8191 and D >= 128:
                K, G = min(K, 5), 1
            out.append((D, K, G, rows))
    return out


def bwd_seg_cases():
    """(D, K, G, rows or None): dout per segment; None: the ragged rowptr as it is, a number: cut to that many
    rows (33: two workgroups; 8193: empty workgroups)."""
    out = [(D, K, GS[(a + b + 1) % 3], None) for a, D in enumerate(DS) for b, K in enumerate(KS)]
    return out + [(4, 12, 5, 33), (128, 5, 1, 8193), (256, 2, 1, 8193)]


def seg_rowptr_for(D, rows=None):
    return ragged_rowptr(rr.head_tile(D), rows, big=300)


def head_k_inputs(D, K, G, rows, n_seg=None, seed=0):
    """hs, ws [K, D], bs ([K]; every third group's None), dout ([rows, K] or [n_seg, K]), dw_old, db_old."""
    rng = np.random.default_rng(7919 * D + 104729 * K + 101 * G + 13 * rows + seed)
    nrm = lambda *s: rng.standard_normal(s).astype(F)  # noqa: E731
    return dict(hs=[nrm(rows, D) for _ in range(G)], ws=[nrm(K, D) / F(np.sqrt(D)) for _ in range(G)],
                bs=[None if g % 3 == 1 else nrm(K) for g in range(G)],
                dout=nrm(rows if n_seg is None else n_seg, K), dw_old=[nrm(K, D) for _ in range(G)],
                db_old=[nrm(K) for _ in range(G)])


def error_inputs(n, K, seed=0):
    """pred / target [n, K] float32 with magnitudes over about 1e-3 .. 1e3 and exact ties at every index = 3 mod 7
    (tests/test_gpu_metrics.py's draw, per column)."""
    rng = np.random.default_rng(1000 * n + K + seed)
    pred = (10.0 ** rng.uniform(-3, 3, (n, K)) * rng.choice([-1.0, 1.0], (n, K))).astype(F)
    target = (pred + 10.0 ** rng.uniform(-3, 3, (n, K)) * rng.choice([-1.0, 1.0], (n, K))).astype(F)
    flat_p, flat_t = pred.reshape(-1), target.reshape(-1)
    flat_t[3::7] = flat_p[3::7]
    return pred, target


# ------------------------------------------------------------------------------------------------ the report
@functools.lru_cache(maxsize=None)
def emulation_report():
    """{family: (worst emulation error / (2^-24 unit), output, case)} over the GPU test's shapes."""
    rep = rr.Report()
    for D, K, G, rows, why in fwd_cases():
        i = head_k_inputs(D, K, G, rows)
        rep.add("heads_k", "out", f"fwd D={D} K={K} G={G} rows={rows}", emu_heads_k(i["hs"], i["ws"], i["bs"]),
                heads_k(i["hs"], i["ws"], i["bs"]))
    for D, K, G in pool_cases():
        rp = seg_rowptr_for(D)
        i = head_k_inputs(D, K, G, int(rp[-1]))
        rep.add("heads_k", "out_seg", f"pool D={D} K={K} G={G}", emu_heads_k_pool(i["hs"], i["ws"], i["bs"], rp),
                heads_k_pool(i["hs"], i["ws"], i["bs"], rp))
    cases = [(D, K, G, rows, None) for D, K, G, rows in bwd_cases()]
    for D, K, G, rows in bwd_seg_cases():
        rp = seg_rowptr_for(D, rows)
        cases.append((D, K, G, int(rp[-1]), rp))
    for D, K, G, rows, rp in cases:
        i = head_k_inputs(D, K, G, rows, None if rp is None else len(rp) - 1)
        ref, emu = heads_k_bwd(i["dout"], i["hs"], i["ws"], rp), emu_heads_k_bwd(i["dout"], i["hs"], i["ws"], rp)
        for g in range(G):
            for k in ref[g]:
                fam = "heads_k_seg" if rp is not None and k != "dh" else "heads_k"
                rep.add(fam, k, f"bwd D={D} K={K} G={G} rows={rows} {'seg' if rp is not None else 'row'}",
                        emu[g][k], ref[g][k])
    return rep.worst
