"""The rbf gate / pool (csrc/rbf_gate.hip), the readout heads and the smooth-L1 loss (csrc/readout.hip) stated in
float64 on the CPU, each value with its *unit*, and a numpy-float32 emulation that fixes the bound's constants.

Values (numpy float64; nothing from x2gnn; the statements are include/x2g.h's comments and oracle/ref_cpu.py):
``gate`` out = x * (rbf @ w.T + b), ``pool`` its sum over the rows of each segment, ``gate_bwd`` dx / drbf / dw / db
as the comment above x2g_rbf_gate_bwd states them (g_row = g[owner[e]] with an owner; ``gate_bwd_batch`` sums drbf
over the jobs), ``heads`` out[r] = sum_g (h_g[r] . w_g + b_g), ``heads_pool`` its sum per segment, ``heads_bwd``
dh_g / dw_g / db_g (dout per row, or per segment with ``seg_rowptr``), ``smooth_l1_mean`` the loss and dpred.
Every input is the float32 array the kernel gets, widened to float64.

Units.  Every function returns (value, unit) pairs: the unit is the float64 sum of the absolute values of the
terms that make the value up (a pooled channel: sum_e |x| (sum_j |w| |rbf| + |b|); dw[c, j]: sum_e |g_row x| |rbf|;
dout * w: that product's magnitude; the loss: the mean of the per-element terms; a value added onto old contents:
plus |old|).  A kernel passes when its value is finite and |kernel - ref64| <= K * 2^-24 * unit; there is no
absolute floor, and where the unit is exactly 0 the kernel has to return exactly 0.

K per family is fixed against the emulation below (``emu_*``: numpy float32, the filter formed by fma in j order,
every sum sequential in row / channel / group order), measured against the float64 reference and never against a
kernel: the emulation's worst error / (2^-24 unit) over the shapes of tests/test_gpu_readout_fp64.py (the case
lists at the end of this module), times 4, rounded up to a power of two.  4x because the kernels sum in another
order (per-slot partials, LDS fold, slab sum, fma contraction), which can cost a small multiple of a sequential
sum's error but not more.  ``emulation_report`` measures the ratios; tests/test_readout_ref.py asserts that each
stays at or below EMULATION_RATIO and that 4 * EMULATION_RATIO <= K:

    family     worst emulation ratio (output, case)                               x 4     K
    gate_fwd   4.14  (gate out, D = 128, R = 8, 101 rows: the 9-term fma chain)    16.6    32
    gate_bwd   6.71  (drbf, D = 128, R = 6: the 128-channel sequential sum)        26.8    32
    heads      4.06  (pooled heads, D = 4, G = 1: the 300-row segment)             16.2    32
    loss       11.12 (loss, n = 256: 256 one-term partials added in order)         44.5    64

The loss is the one departure from "one sequential sum": its emulation adds 256 element-strided partial sums
(the forward is documented as one 256-thread workgroup) and then those 256 in order.  A single sequential
float32 sum of 262 145 non-negative terms is 1111 units off (every addend loses its low bits against the
running total, always in the same direction), which would set K = 8192: wider than the 1e-5 relative
perturbation the bound has to catch.
"""
import functools

import numpy as np

E32 = 2.0 ** -24
F = np.float32
# worst |emulation - ref64| / (2^-24 unit) per family over the GPU test's shapes, rounded up (emulation_report)
EMULATION_RATIO = dict(gate_fwd=4.2, gate_bwd=6.8, heads=4.1, loss=11.2)
K = dict(gate_fwd=32.0, gate_bwd=32.0, heads=32.0, loss=64.0)


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


# ------------------------------------------------------------------------------------------------ index helpers
def owner_of(rowptr):
    """The segment of every row of a CSR rowptr."""
    rowptr = np.asarray(rowptr, np.int64)
    return np.repeat(np.arange(rowptr.shape[0] - 1), np.diff(rowptr))


def seg_sum(v, rowptr):
    v = np.asarray(v)
    out = np.zeros((len(rowptr) - 1,) + v.shape[1:], v.dtype)
    np.add.at(out, owner_of(rowptr), v)
    return out


# ------------------------------------------------------------------------------------------------ values, units
def _filter(rbf, w, b):
    rbf, w, b = _f64(rbf), _f64(w), _f64(b)
    f, fa = rbf @ w.T, np.abs(rbf) @ np.abs(w).T
    if b is not None:
        f, fa = f + b[None, :], fa + np.abs(b)[None, :]
    return f, fa


def gate(x, rbf, w, b=None):
    """out[e, c] = x[e, c] * (sum_j w[c, j] rbf[e, j] + b[c])   (w [D, R])."""
    f, fa = _filter(rbf, w, b)
    x = _f64(x)
    return x * f, np.abs(x) * fa


def pool(x, rbf, w, b, rowptr):
    v, u = gate(x, rbf, w, b)
    return seg_sum(v, rowptr), seg_sum(u, rowptr)


def gate_bwd(g, owner, x, rbf, w, b=None, dx_add=None, drbf_old=None):
    """dict(dx, drbf, dw, db) of (value, unit): dx = g_row f (+ dx_add), drbf[e, j] = sum_c (g_row x)_c w[c, j]
    (+ drbf_old), dw[c, j] = sum_e (g_row x)_c rbf[e, j], db[c] = sum_e (g_row x)_c."""
    g, x, rbf, w = _f64(g), _f64(x), _f64(rbf), _f64(w)
    gr = g if owner is None else g[np.asarray(owner, np.int64)]
    f, fa = _filter(rbf, w, b)
    dx, dxu = gr * f, np.abs(gr) * fa
    if dx_add is not None:
        dx, dxu = dx + _f64(dx_add), dxu + np.abs(_f64(dx_add))
    gx = gr * x
    drbf, drbfu = gx @ w, np.abs(gx) @ np.abs(w)
    if drbf_old is not None:
        drbf, drbfu = drbf + _f64(drbf_old), drbfu + np.abs(_f64(drbf_old))
    return dict(dx=(dx, dxu), drbf=(drbf, drbfu), dw=(gx.T @ rbf, np.abs(gx).T @ np.abs(rbf)),
                db=(gx.sum(0), np.abs(gx).sum(0)))


def gate_bwd_batch(jobs, owner, rbf, drbf_old=None):
    """jobs: dicts with g, x, w, b, dx_add -> (one gate_bwd dict per job, (drbf, unit) summed over the jobs)."""
    outs = [gate_bwd(j["g"], owner, j["x"], rbf, j["w"], j.get("b"), j.get("dx_add")) for j in jobs]
    drbf, unit = sum(o["drbf"][0] for o in outs), sum(o["drbf"][1] for o in outs)
    if drbf_old is not None:
        drbf, unit = drbf + _f64(drbf_old), unit + np.abs(_f64(drbf_old))
    return outs, (drbf, unit)


def heads(hs, ws, bs):
    """out[r] = sum_g (h_g[r] . w_g + b_g)   (bs[g]: a float or None)."""
    out = unit = 0.0
    for h, w, b in zip(hs, ws, bs):
        out = out + _f64(h) @ _f64(w) + (0.0 if b is None else float(b))
        unit = unit + np.abs(_f64(h)) @ np.abs(_f64(w)) + (0.0 if b is None else abs(float(b)))
    return out, unit


def heads_pool(hs, ws, bs, seg_rowptr):
    v, u = heads(hs, ws, bs)
    return seg_sum(v, seg_rowptr), seg_sum(u, seg_rowptr)


def heads_bwd(dout, hs, ws, seg_rowptr=None):
    """[dict(dh, dw, db) of (value, unit) per group]; ``seg_rowptr``: dout is given per segment of rows."""
    d = _f64(dout)
    if seg_rowptr is not None:
        d = d[owner_of(seg_rowptr)]
    res = []
    for h, w in zip(hs, ws):
        h, w = _f64(h), _f64(w)
        dh = d[:, None] * w[None, :]
        res.append(dict(dh=(dh, np.abs(dh)), dw=(d @ h, np.abs(d) @ np.abs(h)), db=(d.sum(), np.abs(d).sum())))
    return res


def smooth_l1_mean(pred, target, beta, gout=1.0):
    """((loss, unit), (dpred, unit)): mean of (|d| < beta ? 0.5 d^2 / beta : |d| - 0.5 beta), d = pred - target;
    dpred = gout / n * clamp(d / beta, -1, 1)."""
    d = _f64(pred) - _f64(target)
    beta = float(beta)
    a = np.abs(d)
    terms = np.where(a < beta, 0.5 * d * d / beta, a - 0.5 * beta)
    dp = float(F(gout)) / d.shape[0] * np.clip(d / beta, -1.0, 1.0)  # (gout as the kernel gets it: float32)
    return (terms.mean(), np.abs(terms).mean()), (dp, np.abs(dp))


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


def _seq_seg(v, rowptr):
    """Per segment, the rows added in row order in float32."""
    rowptr = np.asarray(rowptr, np.int64)
    out = np.zeros((rowptr.shape[0] - 1,) + v.shape[1:], F)
    lens = np.diff(rowptr)
    for k in range(int(lens.max()) if lens.size else 0):
        segs = np.nonzero(lens > k)[0]
        out[segs] = out[segs] + v[rowptr[segs] + k]
    return out


def emu_filter(rbf, w, b):
    rbf, w = np.asarray(rbf, F), np.asarray(w, F)
    a = np.zeros((rbf.shape[0], w.shape[0]), F) + (np.asarray(b, F)[None, :] if b is not None else F(0))
    for j in range(w.shape[1]):
        a = _fma(w[None, :, j], rbf[:, j:j + 1], a)
    return a


def emu_gate(x, rbf, w, b=None):
    return np.asarray(x, F) * emu_filter(rbf, w, b)


def emu_pool(x, rbf, w, b, rowptr):
    return _seq_seg(emu_gate(x, rbf, w, b), rowptr)


def emu_gate_bwd(g, owner, x, rbf, w, b=None, dx_add=None, drbf_old=None):
    g, x, rbf, w = (np.asarray(a, F) for a in (g, x, rbf, w))
    gr = g if owner is None else g[np.asarray(owner, np.int64)]
    dx = gr * emu_filter(rbf, w, b)
    if dx_add is not None:
        dx = dx + np.asarray(dx_add, F)
    gx = gr * x
    drbf = _seq(gx[:, :, None] * w[None, :, :], axis=1)
    if drbf_old is not None:
        drbf = drbf + np.asarray(drbf_old, F)
    return dict(dx=dx, drbf=drbf, dw=_seq(gx[:, :, None] * rbf[:, None, :], axis=0), db=_seq(gx, axis=0))


def emu_heads(hs, ws, bs):
    out = np.zeros(np.asarray(hs[0]).shape[0], F)
    for h, w, b in zip(hs, ws, bs):
        d = _seq(np.asarray(h, F) * np.asarray(w, F)[None, :], axis=1)
        out = out + (d + (F(b) if b is not None else F(0)))
    return out


def emu_heads_pool(hs, ws, bs, seg_rowptr):
    return _seq_seg(emu_heads(hs, ws, bs), seg_rowptr)


def emu_heads_bwd(dout, hs, ws, seg_rowptr=None):
    d = np.asarray(dout, F)
    if seg_rowptr is not None:
        d = d[owner_of(seg_rowptr)]
    return [dict(dh=d[:, None] * np.asarray(w, F)[None, :], dw=_seq(d[:, None] * np.asarray(h, F), axis=0),
                 db=_seq(d, axis=0)) for h, w in zip(hs, ws)]


LOSS_LANES = 256  # the loss forward is one 256-thread workgroup (include/x2g.h: one launch; csrc/readout.hip)


def emu_smooth_l1_mean(pred, target, beta, gout=1.0):
    """The loss as 256 element-strided sequential sums, then those 256 in order (module docstring: one sequential
    sum over all n would set K = 8192)."""
    d = np.asarray(pred, F) - np.asarray(target, F)
    beta, n = F(beta), F(d.shape[0])
    a = np.abs(d)
    terms = np.where(a < beta, F(0.5) * d * d / beta, a - F(0.5) * beta).astype(F)
    g = F(gout) / n
    dp = g * np.where(d < -beta, F(-1), np.where(d > beta, F(1), d / beta)).astype(F)
    lanes = np.zeros((-(-d.shape[0] // LOSS_LANES)) * LOSS_LANES, F)
    lanes[:d.shape[0]] = terms
    return _seq(_seq(lanes.reshape(-1, LOSS_LANES), axis=0)) / n, dp


# ------------------------------------------------------------------------------------------------ shapes, inputs
GATE_D, GATE_R = (64, 128, 256), tuple(range(1, 9))
GATE_BWD_SPLITS, GATE_BWD_UNROLL = 128, 3  # kGateBwdSplits, rbf_gate_bwd_kernel's UNROLL
HEAD_D, HEAD_G = (4, 8, 16, 32, 64, 128, 256), (1, 3, 8)
HEAD_BWD_ROWS = (1, 31, 32, 33, 8191, 8192, 8193)  # 32 rows per split, 256 splits; 8193: per = 33, 7 empty workgroups
LOSS_N, LOSS_BETA, LOSS_GOUT = (1, 3, 255, 256, 257, 1000, 262145), (0.5, 1.0, 2.0), (1.0, -0.37)


def gate_fwd_tile(D):
    """Rows per workgroup pass of rbf_gate_fwd_kernel: RPB (256 / LPR row slots) x UNROLL (4)."""
    return (256 // (D // 4)) * 4


def pool_tile(D):
    """Rows per wave pass of rbf_pool_fwd_kernel: UNROLL (8) x RPI (64 / LPR)."""
    return 8 * (64 // (D // 4))


def gate_bwd_rpb(D):
    return 256 // (D // 4)


def gate_fwd_rows(D):
    t = gate_fwd_tile(D)
    return [(0, "rows=0"), (1, "rows=1"), (t - 1, "tile-1"), (t, "tile"), (t + 1, "tile+1"), (3 * t + 5, "3tiles+5")]


def gate_bwd_rows(D):
    """(rows, boundary): 8 rows per workgroup up to 128 workgroups; 1025: per = 9 and workgroups 114.. own no row;
    3 RPB 128 + 5: more than one UNROLL pass per slot."""
    big = GATE_BWD_UNROLL * gate_bwd_rpb(D) * GATE_BWD_SPLITS + 5
    return [(1, "one-row"), (7, "wg-1"), (8, "wg"), (9, "wg+1"), (1023, "128wg-1"), (1024, "128wg"),
            (1025, "empty-workgroups"), (big, "second-unroll-pass")]


def head_tile(D):
    """Rows per workgroup pass of the head forward kernels: 4 waves x RPW (64 / LPR)."""
    return 4 * (64 // (D // 4))


def head_fwd_rows(D):
    t = head_tile(D)
    return [(0, "rows=0"), (1, "rows=1"), (t - 1, "wg-1"), (t, "wg"), (t + 1, "wg+1"), (2048 * t + 1, "past-grid-cap")]


def ragged_lengths(tile):
    """Segment lengths with empty segments first, in the middle and last, 1, tile - 1, tile, tile + 1 and 400."""
    return [0, 1, tile - 1, 0, tile, tile + 1, 1, 400, 0]


def ragged_rowptr(tile, total=None, big=400):
    """int32 rowptr over ``ragged_lengths`` (400 -> ``big``); with ``total`` the pattern is repeated and cut so
    that the segments cover exactly that many rows (the last segment stays empty)."""
    pat = [big if n == 400 else n for n in ragged_lengths(tile)]
    if total is None:
        lens = pat
    else:
        lens, left, i = [], int(total), 0
        while left > 0:
            n = min(pat[i % len(pat)], left)
            lens.append(n)
            left -= n
            i += 1
        lens.append(0)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def gate_inputs(D, R, rows, n_seg=None, seed=0, jobs=1):
    """Seeded float32 inputs: per job x, w, b, g ([rows, D] or [n_seg, D]), dx_add; shared rbf and drbf_old."""
    rng = np.random.default_rng(100003 * D + 1009 * R + 17 * rows + seed)
    nrm = lambda *s: rng.standard_normal(s).astype(F)  # noqa: E731
    out = dict(rbf=nrm(rows, R), drbf_old=nrm(rows, R), jobs=[])
    for _ in range(jobs):
        out["jobs"].append(dict(x=nrm(rows, D), w=(nrm(D, R) / F(np.sqrt(R))), b=nrm(D),
                                g=nrm(rows if n_seg is None else n_seg, D), dx_add=nrm(rows, D),
                                dw_old=nrm(D, R), db_old=nrm(D)))
    return out


def head_inputs(D, G, rows, n_seg=None, seed=0):
    """hs, ws, bs (every third group's bias None), dout ([rows] or [n_seg]), dw_old, db_old."""
    rng = np.random.default_rng(7919 * D + 101 * G + 13 * rows + seed)
    nrm = lambda *s: rng.standard_normal(s).astype(F)  # noqa: E731
    return dict(hs=[nrm(rows, D) for _ in range(G)], ws=[nrm(D) / F(np.sqrt(D)) for _ in range(G)],
                bs=[None if g % 3 == 1 else float(nrm(1)[0]) for g in range(G)],
                dout=nrm(rows if n_seg is None else n_seg), dw_old=[nrm(D) for _ in range(G)],
                db_old=[nrm(1) for _ in range(G)])


def loss_inputs(n, beta, seed=0):
    """pred, target: seeded; the first elements sit on d = 0, d = +-beta exactly (target 0), |d| = beta (1 +- 2^-23)
    and |d| = 100 beta (as many of them as n holds)."""
    rng = np.random.default_rng(31 * n + int(8 * beta) + seed)
    pred = (rng.standard_normal(n) * 1.5 * beta).astype(F)
    target = rng.standard_normal(n).astype(F)
    b = F(beta)
    special = [(target[0], target[0]), (b, 0), (-b, 0), (b * F(1 + 2.0 ** -23), 0), (-b * F(1 - 2.0 ** -23), 0),
               (F(100) * b, 0), (F(-100) * b, 0), (b * F(1 - 2.0 ** -23), 0), (-b * F(1 + 2.0 ** -23), 0)]
    order = [1, 0, 2, 3, 4, 5, 6, 7, 8]  # n = 1: d = +beta exactly
    for i, k in enumerate(order[:n]):
        pred[i], target[i] = special[k]
    return pred, target


def gate_bwd_cases():
    """(D, R, rows, boundary) of the gate backward: every (D, R) at 1025 rows, every row count at R = 6."""
    cases = [(D, R, 1025, "empty-workgroups") for D in GATE_D for R in GATE_R]
    cases += [(D, 6, rows, why) for D in GATE_D for rows, why in gate_bwd_rows(D) if rows != 1025]
    return cases


def head_bwd_groups(D, rows):
    """The group counts run at (D, rows): all of HEAD_G at the small row counts, fewer rows x groups at 8191+."""
    if rows < 8191:
        return HEAD_G
    return (3,) if D <= 64 or rows == 8193 else (1,)


# ------------------------------------------------------------------------------------------------ the report
def _ratio(got, ref, unit):
    """Worst |got - ref| / (2^-24 unit); an element with unit 0 has to be exactly 0 (inf otherwise)."""
    got, ref, unit = np.asarray(got, np.float64), np.asarray(ref), np.asarray(unit)
    err = np.abs(got - ref)
    if not np.isfinite(got).all():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(unit > 0, err / (E32 * unit), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


class Report:
    def __init__(self):
        self.worst = {}

    def add(self, family, output, case, got, ref_unit):
        r = _ratio(got, *ref_unit)
        if r > self.worst.get(family, (-1.0,))[0]:
            self.worst[family] = (r, output, case)
        return r


@functools.lru_cache(maxsize=None)
def emulation_report():
    """{family: (worst emulation error / (2^-24 unit), output, case)} over the GPU test's shapes."""
    rep = Report()
    for D in GATE_D:
        t = gate_fwd_tile(D)
        for R, rows in [(R, 3 * t + 5) for R in GATE_R] + [(6, r) for r, _ in gate_fwd_rows(D) if r]:
            for bias in (True, False):
                i = gate_inputs(D, R, rows)
                j = i["jobs"][0]
                b = j["b"] if bias else None
                rep.add("gate_fwd", "out", f"gate D={D} R={R} rows={rows}", emu_gate(j["x"], i["rbf"], j["w"], b),
                        gate(j["x"], i["rbf"], j["w"], b))
        rp = ragged_rowptr(pool_tile(D))
        for R in GATE_R:
            i = gate_inputs(D, R, int(rp[-1]))
            j = i["jobs"][0]
            rep.add("gate_fwd", "pooled", f"pool D={D} R={R}", emu_pool(j["x"], i["rbf"], j["w"], j["b"], rp),
                    pool(j["x"], i["rbf"], j["w"], j["b"], rp))
    for D, R, rows, why in gate_bwd_cases():
        rp = ragged_rowptr(pool_tile(D), rows)
        for owner, n_seg in ((None, None), (owner_of(rp), len(rp) - 1)):
            i = gate_inputs(D, R, rows, n_seg)
            j = i["jobs"][0]
            args = (j["g"], owner, j["x"], i["rbf"], j["w"], j["b"], j["dx_add"], i["drbf_old"])
            ref, emu = gate_bwd(*args), emu_gate_bwd(*args)
            for k in ref:
                rep.add("gate_bwd", k, f"D={D} R={R} rows={rows} {'pool' if n_seg else 'gate'}", emu[k], ref[k])
    for D in HEAD_D:
        for rows, why in head_fwd_rows(D):
            for G in (HEAD_G if rows <= head_tile(D) + 1 else (1,)):
                if rows:
                    i = head_inputs(D, G, rows)
                    rep.add("heads", "out", f"fwd D={D} G={G} rows={rows}", emu_heads(i["hs"], i["ws"], i["bs"]),
                            heads(i["hs"], i["ws"], i["bs"]))
        rp = ragged_rowptr(head_tile(D), big=300)
        for G in HEAD_G:
            i = head_inputs(D, G, int(rp[-1]))
            rep.add("heads", "out_seg", f"pool D={D} G={G}", emu_heads_pool(i["hs"], i["ws"], i["bs"], rp),
                    heads_pool(i["hs"], i["ws"], i["bs"], rp))
        for rows in HEAD_BWD_ROWS:
            for G in head_bwd_groups(D, rows):
                i = head_inputs(D, G, rows)
                ref, emu = heads_bwd(i["dout"], i["hs"], i["ws"]), emu_heads_bwd(i["dout"], i["hs"], i["ws"])
                for g in range(G):
                    for k in ref[g]:
                        rep.add("heads", k, f"bwd D={D} G={G} rows={rows}", emu[g][k], ref[g][k])
    for n in LOSS_N:
        for beta in LOSS_BETA:
            for gout in LOSS_GOUT:
                p, t = loss_inputs(n, beta)
                (l, dp), (le, dpe) = smooth_l1_mean(p, t, beta, gout), emu_smooth_l1_mean(p, t, beta, gout)
                rep.add("loss", "loss", f"n={n} beta={beta}", le, l)
                rep.add("loss", "dpred", f"n={n} beta={beta} gout={gout}", dpe, dp)
    return rep.worst
