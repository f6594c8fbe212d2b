"""The staged attention-dropout entry points (include/x2g_staged.h) against the masked fp64 statement of the
operation (tests/dropout_ref.py), with the error measure and bounds of tests/test_gpu_attention_fp64.py
unchanged: error = max|kernel - ref64| / max|ref64|, e32 from the same masked reference evaluated naively in
fp32 on the CPU, bound = min(max(8 e32, floor), 1e-4 scale) with that file's floors (its _Checker does it).

Graphs: attention_ref.edge_case_graph(40) (atoms without edges, degree 1 — no triplet —, degree 2, a triangle,
a chain, a hub of 40 rows: RMAX 4 with a partial last source tile) and ``stars``: hubs of degree 2, 5, 9, 16,
17, 18, 32, 33 (tail-only and full-plus-tail batches, both sides of the 16-row pack, the 17-row untiled / tiled
boundary, the RMAX 2 / 4 boundary at 32 / 33), each launched one atom per workgroup and packed.

The mask the reference takes is dropout_ref.keep_scale (numpy) of the key the kernels are given; p is the
float32 value the entry points receive.
"""
import functools
import zlib

import numpy as np
import pytest
import torch

import attention_ref as ar
import dropout_ref as dr
import test_gpu_attention_fp64 as t64
from test_gpu_attention_fp64 import EDGE_NONE, EDGE_PER_DST, TABLE_ROWS, _Checker, _dev, _nan

from oracle import triplets

pytestmark = pytest.mark.gpu

STAR_DEGREES = (2, 5, 9, 16, 17, 18, 32, 33)
KEYS = [(0, 0, 0), (1, 1, 2), (0x123456789ABCDEF, (1 << 33) + 7, 3)]


@functools.lru_cache(maxsize=None)
def _graph(name):
    if name == "edge":
        return t64._graph("edge")
    assert name == "stars"
    g = t64._Graph()
    g.name, g.batch, g.symmetric = "stars", None, True
    pairs, a = [], 0
    g.hubs = {}
    for d in STAR_DEGREES:
        g.hubs[d] = a
        pairs += [(a, a + 1 + i) for i in range(d)]
        a += d + 1
    g.ei, g.n = ar.symmetric_edges(pairs), a
    g.trip = triplets.vertex_to_edge(g.ei, g.n)[0]
    g.E, g.T = int(g.ei.shape[1]), int(g.trip.shape[1])
    g.z = torch.randint(0, TABLE_ROWS, (g.n,), generator=torch.Generator().manual_seed(g.n)).numpy()
    g.deg = np.bincount(g.ei[0], minlength=g.n)
    g.row_dst = g.z[g.ei[1]]
    g.center = g.ei[1][g.trip[1]]
    assert np.array_equal(g.center, g.ei[0][g.trip[0]])
    return g


@functools.lru_cache(maxsize=4)
def _inputs(gname, regime, H, C):
    g = _graph(gname)
    return ar.make_inputs(regime, g.E, g.T, H * C, zlib.crc32(repr(("drop", gname, regime, H, C)).encode()), TABLE_ROWS)


def _ref_one(g, x, H, C, mode, r, dtype):
    src, dst = torch.from_numpy(g.trip[0]), torch.from_numpy(g.trip[1])
    row_dst, center = torch.from_numpy(g.row_dst), torch.from_numpy(g.center)
    e_t = x["table"][row_dst[dst]] if mode == EDGE_PER_DST else None
    y, radial = x["y"].to(dtype), x["radial"].to(dtype)
    lin = (ar.sbf_from_factors(radial, y, src), x["W"], x["b"])
    res = dr.attention_dropout_ref(x["q"], x["k"], x["v"], x["skip"], None, src, dst, H, C, r, e_t=e_t,
                                   dout=x["dout"], dtype=dtype, lin=lin)
    res["row_mean"], res["row_m2"] = res["row_stats"][:, 0], res["row_stats"][:, 1]
    if e_t is not None:
        res["d_edge_atom"] = ar.rows_sum(res["de_t"], center, g.n)
    res["G"] = ar.fold_g(res["dS"], y, src, g.E)
    res["G_7"] = res["G"][:, 7]
    res["P"] = ar.p_rows(x["W"].to(dtype), radial)
    return res


@functools.lru_cache(maxsize=4)
def _ref(gname, regime, H, C, mode, key, p):
    """(masked fp64 reference, its naive fp32 evaluation): computed once per case, shared, left unchanged.
    ``key`` None: r = 1 everywhere (the unmasked operation)."""
    g, x = _graph(gname), _inputs(gname, regime, H, C)
    r = np.ones((g.T, H), np.float32) if key is None else dr.keep_scale(*key, g.T, H, p)
    return _ref_one(g, x, H, C, mode, r, torch.float64), _ref_one(g, x, H, C, mode, r, torch.float32)


def _key(cuda, key):
    seed, step, _ = key
    to_i64 = lambda v: v - (1 << 64) if v >= 1 << 63 else v  # noqa: E731
    return torch.tensor([to_i64(seed), to_i64(step)], dtype=torch.int64, device=cuda)


def _variants(g, lg):
    """Launch lists (entry, order, packs, info, unit0, units, rows, skip_rows or None) per variant name."""
    sf, tiled = "x2g_sbf_attention_fwd_center_sf", "x2g_sbf_attention_fwd_center_sf_tiled"
    po, pp, info, units, hubs, rows = lg.sched
    N, order = g.n, lg.center_order
    deg_sorted = np.sort(g.deg)[::-1]
    n_big = int((deg_sorted > 17).sum())
    n_r4 = int((deg_sorted > 32).sum())  # the atoms that need RMAX 4 lead the order
    one = []
    if n_r4:
        one.append((tiled, order, None, None, 0, n_r4, int(deg_sorted[0]), 0))
    if n_big > n_r4:  # (launched with their own largest degree: the RMAX 2 instance where it is <= 32)
        one.append((tiled, order, None, None, n_r4, n_big - n_r4, int(deg_sorted[n_r4]), 0))
    one.append((sf, order, None, None, n_big, N - n_big, max(int(deg_sorted[n_big]), 1), None))
    packed = [(tiled, po, pp, info, 0, hubs, lg.max_degree, 0)] * (hubs > 0) + \
        [(sf, po, pp, info, hubs, units - hubs, rows, None)]
    return {"one_atom": one, "packed": packed}


def _forward(g, lg, x, H, C, mode, launches, cuda, drop):
    """Run the launches (``drop`` = (p, key tensor, salt) through the staged entries, None through the plain
    ones) with every output buffer; returns dict(out, logits, seg_max, seg_den, rs, S, P)."""
    from x2gnn._lib import call, ptr, stream_ptr

    E, T, D = g.E, g.T, H * C
    q, k, v, skip, y, radial, W, b = _dev(x, cuda, "q", "k", "v", "skip", "y", "radial", "W", "b")
    edge = x["table"].to(cuda) if mode == EDGE_PER_DST else None
    src_row = lg.src_type if edge is not None else None
    common = (ptr(q), ptr(k), ptr(v), ptr(skip), ptr(edge), ptr(src_row), mode, ptr(radial), ptr(y), ptr(W), ptr(b),
              ptr(lg.atom_rowptr), ptr(lg.edge_rev), ptr(lg.rev_trip))
    o = dict(out=_nan(cuda, E, D), logits=_nan(cuda, T, H), seg_max=_nan(cuda, E, H), seg_den=_nan(cuda, E, H),
             rs=_nan(cuda, E, 2), S=_nan(cuda, T, D), P=_nan(cuda, E, 7, D))
    outs = (E, T, H, C, *[ptr(o[n]) for n in ("out", "logits", "seg_max", "seg_den", "rs", "S", "P")], stream_ptr())
    tail = () if drop is None else (drop[0], ptr(drop[1]), drop[2])
    for entry, order, packs, inf, u0, nu, mrows, skip_rows in launches:
        extra = (mrows,) if skip_rows is None else (mrows, skip_rows)
        call(entry + ("_drop" if drop is not None else ""), *common, ptr(order), ptr(packs), ptr(inf), u0, nu, *extra,
             *outs, *tail)
    return o


def _backward(g, lg, x, H, C, mode, fwd, cuda, drop):
    from x2gnn._lib import call, ptr, stream_ptr

    E, T, D, N = g.E, g.T, H * C, g.n
    q, k, v, dout, y, b = _dev(x, cuda, "q", "k", "v", "dout", "y", "b")
    edge = x["table"].to(cuda) if mode == EDGE_PER_DST else None
    src_row = lg.src_type if edge is not None else None
    o = dict(dq=_nan(cuda, E, D), dk=_nan(cuda, E, D), dv=_nan(cuda, E, D), G=_nan(cuda, E, 8, D),
             d_edge_atom=_nan(cuda, N, D) if edge is not None else None)
    tail = () if drop is None else (drop[0], ptr(drop[1]), drop[2])
    call("x2g_sbf_attention_bwd_center" + ("_drop" if drop is not None else ""), ptr(q), ptr(k), ptr(v), ptr(edge),
         ptr(src_row), mode, None, ptr(fwd["P"]), ptr(b), ptr(y), ptr(lg.atom_rowptr), ptr(lg.edge_rev),
         ptr(lg.rev_trip), ptr(lg.center_order), None, ptr(fwd["seg_max"]), ptr(fwd["seg_den"]), ptr(dout), N,
         lg.max_degree, E, T, H, C, ptr(o["dq"]), ptr(o["dk"]), ptr(o["dv"]), ptr(o["G"]), ptr(o["d_edge_atom"]),
         ptr(torch.empty(2, T, H, device=cuda)), stream_ptr(), *tail)
    return o


def _check_all(ck, ent, mode, refs, fwd, bwd):
    for n in ("out", "logits", "seg_max", "seg_den", "S", "P"):
        ck.check(ent, mode, refs, n, fwd[n])
    ck.check(ent, mode, refs, "row_mean", fwd["rs"][:, 0])
    ck.check(ent, mode, refs, "row_m2", fwd["rs"][:, 1])
    if bwd is not None:
        for n in ("dq", "dk", "dv", "G"):
            ck.check(ent + "+bwd", mode, refs, n, bwd[n])
        ck.check(ent + "+bwd", mode, refs, "G[7]", bwd["G"][:, 7], "G_7")
        if bwd["d_edge_atom"] is not None:
            ck.check(ent + "+bwd", mode, refs, "d_edge_atom", bwd["d_edge_atom"])


# ------------------------------------------------------------------------------ (a) the mask itself
@pytest.mark.parametrize("p", [0.1, 0.5, 0.25])
def test_mask_kernel_is_the_numpy_definition(cuda, p):
    """x2g_attn_dropout_mask == dropout_ref.keep_scale at every (t, h), for three (seed, step, salt) — high
    words of seed and step included —, H = 16 and 8, T not a multiple of the block."""
    from x2gnn._lib import call, ptr, stream_ptr

    p32 = float(np.float32(p))
    for key in KEYS:
        for T, H in ((4099, 16), (1031, 8)):
            r = _nan(cuda, T, H)
            call("x2g_attn_dropout_mask", T, H, p32, ptr(_key(cuda, key)), key[2], ptr(r), stream_ptr())
            want = dr.keep_scale(*key, T, H, p32)
            assert np.array_equal(r.cpu().numpy(), want), (key, T, H)
            assert 0 < (want == 0).mean() < 1


# ------------------------------------------------------------------------------ (b) (c) forward and backward
CASES = [(16, 8, "unit", 0.1), (16, 8, "peaked", 0.5), (8, 16, "unit", 0.5), (8, 16, "peaked", 0.1)]


@pytest.mark.parametrize("H,C,regime,p", CASES)
@pytest.mark.parametrize("gname", ["edge", "stars"])
def test_dropout_entries_against_the_masked_reference(cuda, gname, H, C, regime, p):
    """(b) out, seg_max, seg_den, row statistics, the stored logits, S and P rows of the two drop forwards (one
    atom per workgroup with the tiled form's RMAX 2 and 4 launches; packed) and dq, dk, dv, G, the per-atom edge
    gradient of the drop backward, against the masked fp64 reference; (c) seg_max, seg_den, logits, S and P
    rows bitwise those of the plain entries on the same inputs and launches."""
    g = _graph(gname)
    lg, x = t64._line_graph(g, cuda), _inputs(gname, regime, H, C)
    p32 = float(np.float32(p))
    key = KEYS[1] if H == 16 else KEYS[2]
    drop = (p32, _key(cuda, key), key[2])
    ck = _Checker(gname, regime, H, C)
    not_bitwise = []
    for mode in (EDGE_NONE, EDGE_PER_DST):
        refs = _ref(gname, regime, H, C, mode, key, p32)
        outs = {}
        for vname, launches in _variants(g, lg).items():
            fwd = _forward(g, lg, x, H, C, mode, launches, cuda, drop)
            bwd = _backward(g, lg, x, H, C, mode, fwd, cuda, drop)
            _check_all(ck, f"drop[{vname},p={p}]", mode, refs, fwd, bwd)
            plain = _forward(g, lg, x, H, C, mode, launches, cuda, None)
            for n in ("seg_max", "seg_den", "logits", "S", "P"):  # (NaN nowhere: every row is written)
                if not torch.equal(fwd[n], plain[n]):
                    rows = (fwd[n] != plain[n]).reshape(fwd[n].shape[0], -1).any(1).nonzero().flatten().tolist()
                    not_bitwise.append((vname, mode, n, len(rows), rows[:4]))
            assert not torch.equal(fwd["out"], plain["out"])
            outs[vname] = (fwd, bwd)
        # packing changes no bit of an untiled unit (every sum keeps its order within an atom's block), with the
        # mask too: the destinations whose center atom has at most 17 rows
        small = torch.from_numpy(g.deg[g.ei[1]] <= 17).to(cuda)
        for n in ("out", "seg_den"):
            assert torch.equal(outs["one_atom"][0][n][small], outs["packed"][0][n][small]), n
    ck.done()
    assert not not_bitwise, f"differ from the plain entry (variant, mode, output, rows, first rows): {not_bitwise}"


# ------------------------------------------------------------------------------ (d) p = 0
@pytest.mark.parametrize("gname", ["edge", "stars"])
def test_p_0_through_the_drop_entries_is_the_unmasked_operation(cuda, gname):
    H, C, regime = 16, 8, "unit"
    g = _graph(gname)
    lg, x = t64._line_graph(g, cuda), _inputs(gname, regime, H, C)
    drop = (0.0, _key(cuda, KEYS[1]), 1)
    ck = _Checker(gname, regime, H, C)
    for mode in (EDGE_NONE, EDGE_PER_DST):
        refs = _ref(gname, regime, H, C, mode, None, 0.0)
        for vname, launches in _variants(g, lg).items():
            fwd = _forward(g, lg, x, H, C, mode, launches, cuda, drop)
            bwd = _backward(g, lg, x, H, C, mode, fwd, cuda, drop)
            _check_all(ck, f"drop[{vname},p=0]", mode, refs, fwd, bwd)
    ck.done()


# ------------------------------------------------------------------------------ (e) a destination with nothing kept
def test_a_destination_whose_triplets_are_all_dropped_gives_the_skip_row(cuda):
    """The degree-2 star: each of its two hub-bound destinations has one triplet.  A seed under which all 16
    heads of one of them are dropped at p = 0.5 (found with the numpy definition on the host): out == skip there,
    exactly, and its gradient rows dq are zero."""
    H, C, p = 16, 8, 0.5
    g = _graph("stars")
    lg, x = t64._line_graph(g, cuda), _inputs("stars", "unit", H, C)
    hub = g.hubs[2]
    rows = np.nonzero(g.center == hub)[0]  # the two triplets through the hub
    assert len(rows) == 2
    thr = np.uint64(dr.threshold(p))
    seeds = np.arange(1 << 18, dtype=np.uint64)
    # keys of (seed, step 3, salt 1) for every candidate seed at once (seed_hi = step_hi = 0)
    k0 = dr.mix(seeds ^ dr.mix(np.uint64(3) ^ np.uint64((1 * 0x9E3779B9) & 0xFFFFFFFF)))
    k1 = dr.mix((np.uint64(0) + dr.mix(np.uint64(0) ^ k0)) & dr.M32)
    found = None
    for t in rows:
        c = (np.uint64(int(t) * H) + np.arange(H, dtype=np.uint64))[None, :]
        kept = dr.mix((dr.mix(c ^ k0[:, None]) + k1[:, None]) & dr.M32) >= thr
        hit = np.nonzero(~kept.any(1))[0]
        if len(hit):
            found = (int(seeds[hit[0]]), int(t))
            break
    assert found is not None, "no seed below 2^18 drops all 16 heads of either triplet"
    seed, t = found
    key = (seed, 3, 1)
    assert not dr.keep_scale(*key, g.T, H, p)[t].any()
    d = int(g.trip[1][t])
    drop = (p, _key(cuda, key), 1)
    fwd = _forward(g, lg, x, H, C, EDGE_PER_DST, _variants(g, lg)["packed"], cuda, drop)
    assert torch.equal(fwd["out"][d].cpu(), x["skip"][d])
    bwd = _backward(g, lg, x, H, C, EDGE_PER_DST, fwd, cuda, drop)
    assert float(bwd["dq"][d].abs().max()) == 0.0


# ------------------------------------------------------------------------------ (f) refusals
def test_refusals(cuda):
    from x2gnn import _lib

    lib = _lib.load()
    n = None
    key = _key(cuda, KEYS[1])
    kp = _lib.ptr(key)
    dummy = _lib.ptr(torch.zeros(128, device=cuda))
    H, C = 16, 8
    fwd = lambda p, k: lib.x2g_sbf_attention_fwd_center_sf_drop(  # noqa: E731
        n, n, n, n, n, n, 0, n, n, n, n, n, n, n, n, n, n, 0, 1, 17, 4, 4, H, C, n, n, n, n, n, n, n, n, p, k, 0)
    til = lambda p, k, md=33: lib.x2g_sbf_attention_fwd_center_sf_tiled_drop(  # noqa: E731
        n, n, n, n, n, n, 0, n, n, n, n, n, n, n, n, n, n, 0, 1, md, 0, 4, 4, H, C, n, n, n, n, n, n, n, n, p, k, 0)
    bwd = lambda p, k, sp=None, pp=None: lib.x2g_sbf_attention_bwd_center_drop(  # noqa: E731
        n, n, n, n, n, 0, sp, pp, n, n, n, n, n, n, n, n, n, n, 1, 4, 4, 4, H, C, n, n, n, n, n, n, n, p, k, 0)
    mask = lambda p, k: lib.x2g_attn_dropout_mask(4, H, p, k, 0, dummy, n)  # noqa: E731
    EINVAL, EUNSUPPORTED = 1001, 1002
    for f in (fwd, til, bwd, mask):
        assert f(1.0, kp) == EINVAL      # drop_p outside [0, 1)
        assert f(-0.5, kp) == EINVAL
        assert f(float("nan"), kp) == EINVAL
        assert f(0.5, None) == EINVAL    # NULL key
    assert bwd(0.5, kp, sp=dummy) == EUNSUPPORTED  # the S-row form (sbfproj given, sbf_p NULL)
    assert til(0.5, kp, md=65) == EUNSUPPORTED     # no RMAX 8 dropout instance


def test_operator_refuses_routes_without_dropout_kernels(cuda, monkeypatch):
    """ops.sbf_attention with dropout set: NotImplementedError naming the condition, for per-triplet edge
    attributes, absent sbf factors, a line graph that is not symmetric and the center kernels switched off; and p
    = 0 runs the plain entries."""
    from test_gpu_model import record_calls
    from x2gnn import ops
    from x2gnn.plan import GraphPlan

    H, C = 16, 8
    g = t64._graph("mol")
    x = t64._inputs("mol", "unit", H, C)
    lg = GraphPlan.from_atom_batch(g.batch.to(cuda)).lg
    sbf, radial, y = _dev(x, cuda, "sbf", "radial", "y")
    lg.sbf_factors = (sbf, radial, y)
    q, k, v, skip, table, W, b, e_trip = _dev(x, cuda, "q", "k", "v", "skip", "table", "W", "b", "e_trip")
    drop = (0.25, _key(cuda, KEYS[1]), 0)
    kw = dict(edge_mode=ops.EDGE_PER_DST, edge_row=lg.dst_type)
    with pytest.raises(NotImplementedError, match="per-triplet"):
        ops.sbf_attention(q, k, v, skip, e_trip, sbf, W, b, lg, H, C, edge_mode=ops.EDGE_PER_TRIPLET, dropout=drop)
    with pytest.raises(NotImplementedError, match="factors"):
        ops.sbf_attention(q, k, v, skip, table, sbf.clone(), W, b, lg, H, C, dropout=drop, **kw)
    with monkeypatch.context() as m:
        m.setattr(ops, "_CENTER_P", False)
        with pytest.raises(NotImplementedError, match="switched off"):
            ops.sbf_attention(q, k, v, skip, table, sbf, W, b, lg, H, C, dropout=drop, **kw)
    d = t64._graph("directed")
    lgd = ops.vertex_to_edge(torch.from_numpy(d.ei).to(cuda), d.n, d.T)
    xd = t64._inputs("directed", "unit", H, C)
    qd, kd, vd, sd, sbfd = _dev(xd, cuda, "q", "k", "v", "skip", "sbf")
    with pytest.raises(NotImplementedError, match="symmetric"):
        ops.sbf_attention(qd, kd, vd, sd, None, sbfd, W, b, lgd, H, C, dropout=drop)
    with pytest.raises(ValueError):
        ops.sbf_attention(q, k, v, skip, table, sbf, W, b, lg, H, C, dropout=(1.0, drop[1], 0), **kw)
    seen = record_calls(monkeypatch)
    out0 = ops.sbf_attention(q, k, v, skip, table, sbf, W, b, lg, H, C, dropout=(0.0, drop[1], 0), **kw)
    assert not any(n.endswith("_drop") for n, _ in seen)
    out1 = ops.sbf_attention(q, k, v, skip, table, sbf, W, b, lg, H, C, **kw)
    assert torch.equal(out0, out1)
    seen.clear()
    out2 = ops.sbf_attention(q, k, v, skip, table, sbf, W, b, lg, H, C, dropout=drop, **kw)
    names = [n for n, _ in seen]
    assert "x2g_sbf_attention_fwd_center_sf_drop" in names and "x2g_sbf_attention_fwd_center_sf" not in names
    assert not torch.equal(out2, out1)
