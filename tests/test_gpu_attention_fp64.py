"""Every SBF-transformer attention entry point against the fp64 statement of the operation
(tests/attention_ref.py), at small shapes.

Error measure and bound (nothing taken from the code under test): for each output the error is
max|kernel - ref64| / max|ref64|.  The same case is also evaluated by the reference function in float32 on the
CPU (the naive plain-torch evaluation), whose error e32 is measured the same way.  The bound is
max(8 * e32, floor), floor being the suite's kernel-to-kernel tolerance for that kind of output: 2e-6 absolute
for forward outputs, logits and segment maxima (_close_fwd), 1e-5 of scale for seg_den, row_stats and S / P
rows, 2e-5 of scale + 1e-6 for backward outputs (_close_bwd).  The factor 8: a kernel differs from the naive
evaluation in summation order (online rescale, 4-channel partial sums, source tiles), the device expf and
fused multiply-adds, each worth a small constant.  No bound exceeds 1e-4 of its output's scale: the bound is
capped there.  The cap binds only in ``offset`` for dq and the per-destination / per-atom edge gradient on the
edge graph's degree-40 hub, where the naive fp32 evaluation alone reaches e32 = 1.7e-5 (dq) and 2.8e-5
(d_edge) of scale: both are sums over a segment of terms dlogit_t * (common row) whose dlogit_t add up to
zero, a cancellation of ~40x that the per-triplet fp32 products of the naive form do not survive; the kernels
have to stay within 1e-4 of scale there regardless.

Inputs are drawn on the host from a seeded generator in fp32; that fp32 value is what both the kernel and the
reference receive.  Regimes: ``unit`` randn; ``peaked`` |logit| up to ~190 (fp32 exp overflows without the max
shift); ``offset`` whole segments near a common logit of either sign up to ~200 (an unshifted sum underflows).

``python tests/test_gpu_attention_fp64.py --write profiles/attention_fp64_err.json`` runs every case once and
writes, per (entry point, output), the worst error / bound of each regime and the comparison it is worst in with
its error, e32 and bound, and what each entry point was covered at; ``--all-rows`` writes one row per (entry
point, graph, regime, H, C, mode, output) instead.
"""
import functools
import json
import os
import sys
import zlib

import numpy as np
import pytest
import torch

if __name__ == "__main__":  # (run as a script: the paths conftest.py sets up for pytest)
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "x2-gnn_amd"), os.path.join(_root, "tests")]

import attention_ref as ar
from conftest import golden

from oracle import triplets

pytestmark = pytest.mark.gpu

RECORD = []  # one dict per comparison made (the --write entry dumps it)
EDGE_NONE, EDGE_PER_TRIPLET, EDGE_PER_DST = 0, 1, 2
MODE_NAME = {EDGE_NONE: "none", EDGE_PER_TRIPLET: "per_triplet", EDGE_PER_DST: "per_dst"}
TABLE_ROWS = 10
HUB = 40  # the edge graph's hub degree: above the 16-row pack capacity and the 17-row fused / tiled boundary
FWD, STAT, BWD = "fwd", "stat", "bwd"
KIND = dict(out=FWD, logits=FWD, seg_max=FWD, seg_den=STAT, row_mean=STAT, row_m2=STAT, S=STAT, P=STAT)  # else BWD


# ------------------------------------------------------------------------------ graphs, inputs, references
class _Graph:
    pass


@functools.lru_cache(maxsize=None)
def _graph(name):
    """Host description of a test graph: edge_index, the oracle's triplets, atom elements."""
    g = _Graph()
    g.name, g.batch = name, None
    if name == "edge":
        g.ei, g.n = ar.edge_case_graph(HUB)
        g.symmetric = True
    elif name == "mol":
        from x2gnn.data import collate
        from x2gnn.synth import synthetic_molecules

        g.batch = collate(synthetic_molecules(6, "S160", seed=31))
        g.ei, g.n, g.symmetric = g.batch.edge_index.numpy().astype(np.int64), int(g.batch.num_nodes), True
    elif name == "directed":
        z = golden("triplets.npz")
        g.ei, g.n, g.symmetric = z["directed_edge_index"].astype(np.int64), int(z["directed_num_nodes"]), False
    else:
        raise ValueError(name)
    g.trip = triplets.vertex_to_edge(g.ei, g.n)[0]
    g.E, g.T = int(g.ei.shape[1]), int(g.trip.shape[1])
    if g.batch is not None:
        g.z = g.batch.x.numpy().reshape(-1).astype(np.int64)
        assert g.z.max() < TABLE_ROWS
    else:
        g.z = torch.randint(0, TABLE_ROWS, (g.n,), generator=torch.Generator().manual_seed(g.n)).numpy()
    g.deg = np.bincount(g.ei[0], minlength=g.n)
    g.row_dst = g.z[g.ei[1]]  # the table row of a destination line node (a -> b): b's element
    g.center = g.ei[1][g.trip[1]]  # the atom a triplet runs through
    assert np.array_equal(g.center, g.ei[0][g.trip[0]])
    return g


_LG = {}


def _line_graph(g, cuda):
    """The device line graph of ``g`` with the center kernels' schedules: collate's shipped ones for ``mol``,
    data.center_packs for ``edge``."""
    if g.name in _LG:
        return _LG[g.name]
    from x2gnn import ops
    from x2gnn.data import center_hubs, center_packs

    e = torch.from_numpy(g.ei).to(cuda)
    ei32 = ops._i32(e)
    if g.symmetric:
        lg = ops.LineGraph(ei32[0].contiguous(), ei32[1].contiguous(), g.n, g.T, symmetric=True, with_transpose=True)
    else:
        lg = ops.vertex_to_edge(e, g.n, g.T)
    # index arrays only: the kernels' triplet order is the oracle's
    assert np.array_equal(lg.trip_src.cpu().numpy(), g.trip[0]) and np.array_equal(lg.trip_dst.cpu().numpy(), g.trip[1])
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(cuda)  # noqa: E731
    lg.atom_type, lg.src_type, lg.dst_type = i32(g.z), i32(g.z[g.ei[0]]), i32(g.row_dst)
    lg.max_degree = int(g.deg.max())
    if g.symmetric:
        if g.batch is not None:
            st = g.batch._store
            order, packs, info = st["_x2g_pack_order"].numpy(), st["_x2g_center_packs"].numpy(), st["_x2g_pack_info"]
            hubs, rows = int(st["_x2g_center_hubs"]), int(st["_x2g_center_rows"])
            lg.center_order = st["_x2g_center_order"].to(cuda)
            info = info.to(cuda)
        else:
            order, packs, _ = center_packs(g.deg)
            hubs, rows = center_hubs(g.deg, order, packs)
            lg.center_order = i32(np.argsort(-g.deg, kind="stable"))
            first = np.concatenate([[0], np.cumsum(g.deg)[:-1]])
            info = i32(np.stack([order, first[order], g.deg[order], np.where(g.deg[order] > 0, g.z[order], 0)], 1)
                       .reshape(-1))
        lg.sched = (i32(order), i32(packs), info, int(len(packs)) - 1, hubs, rows)
    _LG[g.name] = lg
    return lg


@functools.lru_cache(maxsize=8)
def _inputs(gname, regime, H, C):
    g = _graph(gname)
    seed = zlib.crc32(repr((gname, regime, H, C)).encode())
    x = ar.make_inputs(regime, g.E, g.T, H * C, seed, TABLE_ROWS)
    # the raw basis rows the destination-major kernels (and x2g_sbf_project) read: the fp32 product
    x["sbf"] = (x["radial"][torch.from_numpy(g.trip[0])].view(g.T, 7, 6) * x["y"][:, :7, None]).reshape(g.T, 42).contiguous()
    return x


def _ref_one(g, x, H, C, mode, sform, dtype):
    src, dst = torch.from_numpy(g.trip[0]), torch.from_numpy(g.trip[1])
    row_dst, center = torch.from_numpy(g.row_dst), torch.from_numpy(g.center)
    e_t = {EDGE_NONE: None, EDGE_PER_TRIPLET: x["e_trip"], EDGE_PER_DST: x["table"][row_dst[dst]]}[mode]
    y, radial = x["y"].to(dtype), x["radial"].to(dtype)
    if sform == "S":  # S given
        S, lin = x["S"], None
    elif sform == "raw":  # the fp32 basis rows given, projected per triplet
        S, lin = None, (x["sbf"], x["W"], x["b"])
    else:  # "fac": the kernel forms radial[src] * Y itself
        S, lin = None, (ar.sbf_from_factors(radial, y, src), x["W"], x["b"])
    r = ar.attention_ref(x["q"], x["k"], x["v"], x["skip"], S, src, dst, H, C, e_t=e_t, dout=x["dout"], dtype=dtype,
                         lin=lin)
    r["row_mean"], r["row_m2"] = r["row_stats"][:, 0], r["row_stats"][:, 1]
    if e_t is not None:
        r["d_edge_dst"] = ar.rows_sum(r["de_t"], dst, g.E)
        r["d_edge_atom"] = ar.rows_sum(r["de_t"], center, g.n)
        r["d_table"] = ar.rows_sum(r["d_edge_dst"], row_dst, TABLE_ROWS)
    r["G"] = ar.fold_g(r["dS"], y, src, g.E)
    r["dW_g"], r["db_g"] = ar.wgrad_from_g(r["G"], radial)
    if sform == "fac":
        r["P"] = ar.p_rows(x["W"].to(dtype), radial)
    return r


@functools.lru_cache(maxsize=4)
def _ref(gname, regime, H, C, mode, sform):
    """(fp64 reference, its naive fp32 evaluation) of one case: computed once, shared, left unchanged."""
    g, x = _graph(gname), _inputs(gname, regime, H, C)
    return _ref_one(g, x, H, C, mode, sform, torch.float64), _ref_one(g, x, H, C, mode, sform, torch.float32)


class _Checker:
    """Compares kernel outputs of one case with the reference pair; collects every figure before failing."""

    def __init__(self, gname, regime, H, C):
        self.key = dict(graph=gname, regime=regime, H=H, C=C)
        self.bad = []

    def check(self, entry, mode, refs, name, got, ref_name=None):
        ref_name = ref_name or name
        r64, r32 = refs[0][ref_name], refs[1][ref_name].double()
        got = got.detach().cpu().double().reshape(r64.shape)
        rec = dict(entry=entry, mode=MODE_NAME[mode], output=name, **self.key)
        if torch.isnan(got).any():
            self.bad.append((rec, "NaN in the kernel output"))
            return
        fin = torch.isfinite(r64)  # (seg_max of a destination without triplets: -inf on both sides)
        if not bool(fin.all()):
            if not torch.equal(got[~fin], r64[~fin]):
                self.bad.append((rec, "non-finite entries differ"))
            got, r64, r32 = got[fin], r64[fin], r32[fin]
        scale = float(r64.abs().max())
        err, e32 = float((got - r64).abs().max()), float((r32 - r64).abs().max())
        kind = KIND.get(ref_name, BWD)
        floor = {FWD: 2e-6, STAT: 1e-5 * scale, BWD: 2e-5 * scale + 1e-6}[kind]
        # no bound above 1e-4 of scale: where 8 e32 would be (see the module docstring), the kernel has to
        # meet 1e-4 of scale itself
        bound = min(max(8.0 * e32, floor), 1e-4 * scale)
        assert bound <= 1e-4 * scale
        rec.update(err=err / scale, e32=e32 / scale, bound=bound / scale)
        RECORD.append(rec)
        if not err <= bound:
            self.bad.append((rec, "error above bound"))

    def done(self):
        assert not self.bad, "\n".join(f"{why}: {rec}" for rec, why in self.bad)


def _dev(x, cuda, *names):
    return [x[n].to(cuda) for n in names]


def _nan(cuda, *shape):
    return torch.full(shape, float("nan"), device=cuda, dtype=torch.float32)


# ------------------------------------------------------------------------------ a. destination-major family
def _dst_major(ck, lg, g, x, H, C, mode, sform, cuda):
    """x2g_sbf_attention_fwd, _fwd_stats, _bwd_dst, _bwd_src on one case, every output against the reference."""
    from x2gnn._lib import call, ptr, stream_ptr

    refs = _ref(g.name, ck.key["regime"], H, C, mode, sform)
    E, T, D = g.E, g.T, H * C
    q, k, v, skip, dout = _dev(x, cuda, "q", "k", "v", "skip", "dout")
    edge = {EDGE_NONE: None, EDGE_PER_TRIPLET: x["e_trip"], EDGE_PER_DST: x["table"]}[mode]
    edge = edge.to(cuda) if edge is not None else None
    edge_row = lg.dst_type if mode == EDGE_PER_DST else None
    if sform == "S":
        sbf, w, b, sdim = x["S"].to(cuda), None, None, D
    else:
        sbf, w, b, sdim = x["sbf"].to(cuda), x["W"].to(cuda), x["b"].to(cuda), 42
    tag = "[w_sbf]" if sform == "raw" else ""
    for stats in (False, True):
        out, alpha, smax, sden = _nan(cuda, E, D), _nan(cuda, T, H), _nan(cuda, E, H), _nan(cuda, E, H)
        rs = _nan(cuda, E, 2) if stats else None
        name = "x2g_sbf_attention_fwd_stats" if stats else "x2g_sbf_attention_fwd"
        call(name, ptr(q), ptr(k), ptr(v), ptr(skip), ptr(edge), ptr(edge_row), mode, ptr(sbf), ptr(w), ptr(b),
             ptr(lg.trip_rowptr), ptr(lg.trip_src), E, T, H, C, sdim, ptr(out), ptr(alpha), ptr(smax), ptr(sden),
             *((ptr(rs),) if stats else ()), stream_ptr())
        for n, t in (("out", out), ("logits", alpha), ("seg_max", smax), ("seg_den", sden)):
            ck.check(name + tag, mode, refs, n, t)
        if stats:
            ck.check(name + tag, mode, refs, "row_mean", rs[:, 0])
            ck.check(name + tag, mode, refs, "row_m2", rs[:, 1])
    dq, dlogit, dproj = _nan(cuda, E, D), _nan(cuda, T, H), _nan(cuda, T, D)
    d_edge = {EDGE_NONE: None, EDGE_PER_TRIPLET: _nan(cuda, T, D), EDGE_PER_DST: _nan(cuda, E, D)}[mode]
    call("x2g_sbf_attention_bwd_dst", ptr(q), ptr(k), ptr(v), ptr(edge), ptr(edge_row), mode, ptr(sbf), ptr(w), ptr(b),
         ptr(lg.trip_rowptr), ptr(lg.trip_src), ptr(alpha), ptr(smax), ptr(sden), ptr(dout), E, T, H, C, sdim,
         ptr(dq), ptr(d_edge), ptr(dlogit), ptr(dproj), stream_ptr())
    ent = "x2g_sbf_attention_bwd_dst" + tag
    ck.check(ent, mode, refs, "dq", dq)
    ck.check(ent, mode, refs, "dlogit", dlogit)
    ck.check(ent, mode, refs, "d_sbfproj", dproj, "dS")
    if mode != EDGE_NONE:
        ck.check(ent, mode, refs, "d_edge", d_edge, "de_t" if mode == EDGE_PER_TRIPLET else "d_edge_dst")
    src_rowptr, src_perm = lg.src_csr()
    dk, dv = _nan(cuda, E, D), _nan(cuda, E, D)
    call("x2g_sbf_attention_bwd_src", ptr(q), ptr(sbf), ptr(w), ptr(b), ptr(src_rowptr), ptr(src_perm),
         ptr(lg.trip_dst), ptr(alpha), ptr(smax), ptr(sden), ptr(dlogit), ptr(dout), E, T, H, C, sdim, ptr(dk),
         ptr(dv), stream_ptr())
    # (the source pass adds the edge term's share of dk / dv nowhere: k[src] + e and v[src] + e have unit
    # Jacobians in k and v, so dk, dv are the reference's whatever the mode)
    ck.check("x2g_sbf_attention_bwd_src" + tag, mode, refs, "dk", dk)
    ck.check("x2g_sbf_attention_bwd_src" + tag, mode, refs, "dv", dv)


# every (D, C) dispatch() in csrc/attention.hip instantiates
SUPPORTED = [(D, C) for D in (32, 64) for C in (2, 4, 8, 16)] + [(128, C) for C in (4, 8, 16)] + \
    [(256, C) for C in (4, 8, 16, 32)]
ALL_MODES = (EDGE_NONE, EDGE_PER_TRIPLET, EDGE_PER_DST)


@pytest.mark.parametrize("D,C", SUPPORTED)
def test_destination_major_dispatch_matrix(cuda, D, C):
    """Every supported (D, C) of the destination-major kernels on the edge-case graph (degree-1 atoms, atoms
    without edges, a hub of degree 40, a triangle, a chain), unit inputs: the three edge modes, S given
    (w_sbf NULL) and the raw [T, 42] basis with W, b (the PRE = false templates), forward with and without row
    statistics, both backward passes — against the fp64 reference."""
    H = D // C
    g = _graph("edge")
    lg, x = _line_graph(g, cuda), _inputs("edge", "unit", H, C)
    ck = _Checker("edge", "unit", H, C)
    for mode in ALL_MODES:
        for sform in ("S", "raw"):
            _dst_major(ck, lg, g, x, H, C, mode, sform, cuda)
    ck.done()


@pytest.mark.parametrize("regime", ["peaked", "offset"])
@pytest.mark.parametrize("H,C", [(16, 8), (8, 16), (32, 4)])
def test_destination_major_large_logits(cuda, H, C, regime):
    """D = 128 at the three head shapes with logits beyond the fp32 exp range (``peaked``) and whole segments
    far from zero of either sign (``offset``): the max shift of the forward and of the backward's recomputed
    probabilities.  (``unit`` at these shapes is in the dispatch matrix.)"""
    g = _graph("edge")
    lg, x = _line_graph(g, cuda), _inputs("edge", regime, H, C)
    ck = _Checker("edge", regime, H, C)
    for mode in ALL_MODES:
        _dst_major(ck, lg, g, x, H, C, mode, "S", cuda)
    _dst_major(ck, lg, g, x, H, C, EDGE_PER_DST, "raw", cuda)
    ck.done()


@pytest.mark.parametrize("regime", ar.REGIMES)
def test_destination_major_directed_graph(cuda, regime):
    """The non-symmetric ``directed`` line graph of triplets.npz (generic transpose, ragged segments)."""
    g = _graph("directed")
    lg, x = _line_graph(g, cuda), _inputs("directed", regime, 16, 8)
    ck = _Checker("directed", regime, 16, 8)
    for mode in ALL_MODES:
        for sform in ("S", "raw"):
            _dst_major(ck, lg, g, x, 16, 8, mode, sform, cuda)
    ck.done()


@pytest.mark.parametrize("H,C", [(4, 32), (64, 2), (12, 8), (128, 2)])
def test_unsupported_shapes_are_refused(cuda, H, C):
    """(D=128, C=32), (D=128, C=2), D=96 and (D=256, C=2) lie outside the compiled set: X2G_EUNSUPPORTED from
    all-NULL calls (nothing is launched), from each of the four destination-major entry points."""
    from x2gnn import _lib

    lib, D = _lib.load(), H * C
    n = None
    assert lib.x2g_sbf_attention_fwd(n, n, n, n, n, n, 0, n, n, n, n, n, 0, 0, H, C, D, n, n, n, n, n) == 1002
    assert lib.x2g_sbf_attention_fwd_stats(n, n, n, n, n, n, 0, n, n, n, n, n, 0, 0, H, C, D, n, n, n, n, n, n) == 1002
    assert lib.x2g_sbf_attention_bwd_dst(n, n, n, n, n, 0, n, n, n, n, n, n, n, n, n, 0, 0, H, C, D, n, n, n, n,
                                         n) == 1002
    assert lib.x2g_sbf_attention_bwd_src(n, n, n, n, n, n, n, n, n, n, n, n, 0, 0, H, C, D, n, n, n) == 1002


# ------------------------------------------------------------------------------ b. factorised backward
def _forward_state(lg, g, x, H, C, mode, cuda):
    """(alpha, smax, sden) of x2g_sbf_attention_fwd with S given (checked in the tests above)."""
    from x2gnn._lib import call, ptr, stream_ptr

    E, T, D = g.E, g.T, H * C
    q, k, v, skip, S = _dev(x, cuda, "q", "k", "v", "skip", "S")
    edge = x["table"].to(cuda) if mode == EDGE_PER_DST else None
    out, alpha, smax, sden = _nan(cuda, E, D), _nan(cuda, T, H), _nan(cuda, E, H), _nan(cuda, E, H)
    call("x2g_sbf_attention_fwd", ptr(q), ptr(k), ptr(v), ptr(skip), ptr(edge),
         ptr(lg.dst_type) if edge is not None else None, mode, ptr(S), None, None, ptr(lg.trip_rowptr),
         ptr(lg.trip_src), E, T, H, C, D, ptr(out), ptr(alpha), ptr(smax), ptr(sden), stream_ptr())
    return alpha, smax, sden


def _fold_backward(ck, lg, g, x, H, C, mode, cuda):
    from x2gnn import _lib
    from x2gnn._lib import call, ptr, stream_ptr

    refs = _ref(g.name, ck.key["regime"], H, C, mode, "S")
    E, T, D = g.E, g.T, H * C
    q, k, v, S, dout, y, radial = _dev(x, cuda, "q", "k", "v", "S", "dout", "y", "radial")
    edge = x["table"].to(cuda) if mode == EDGE_PER_DST else None
    edge_row = lg.dst_type if edge is not None else None
    alpha, smax, sden = _forward_state(lg, g, x, H, C, mode, cuda)
    src_rowptr, src_perm = lg.src_csr()
    lib = _lib.load()
    # (g round trip, src_dst, src_row): present / NULL
    for with_g, with_sdst, with_srow in ((True, True, True), (False, False, False), (False, True, False),
                                         (True, False, True)):
        opt = f"[g={int(with_g)},src_dst={int(with_sdst)},src_row={int(with_srow)}]"
        dq, gt, prob, rho = _nan(cuda, E, D), (_nan(cuda, T, H) if with_g else None), _nan(cuda, T, H), _nan(cuda, E, H)
        de = _nan(cuda, E, D) if edge is not None else None
        call("x2g_sbf_attention_bwd_dst_g", ptr(q), ptr(k), ptr(v), ptr(edge), ptr(edge_row), mode, ptr(S),
             ptr(lg.trip_rowptr), ptr(lg.trip_src), ptr(alpha), ptr(smax), ptr(sden), ptr(dout), E, T, H, C, ptr(dq),
             ptr(de), ptr(gt), ptr(prob), ptr(rho), stream_ptr())
        ent = "x2g_sbf_attention_bwd_dst_g" + opt
        ck.check(ent, mode, refs, "dq", dq)
        ck.check(ent, mode, refs, "prob", prob)
        ck.check(ent, mode, refs, "seg_rho", rho)
        if with_g:
            ck.check(ent, mode, refs, "g", gt)
        if edge is not None:
            ck.check(ent, mode, refs, "d_edge", de, "d_edge_dst")
        dk, dv, G = _nan(cuda, E, D), _nan(cuda, E, D), _nan(cuda, E, 8, D)
        call("x2g_sbf_attention_bwd_src_fold", ptr(q), ptr(v), ptr(edge), ptr(edge_row),
             ptr(lg.src_type) if (edge is not None and with_srow) else None, TABLE_ROWS if edge is not None else 0,
             mode, ptr(S), ptr(y), ptr(src_rowptr), ptr(src_perm), ptr(lg.src_dst) if with_sdst else None,
             ptr(lg.trip_dst), ptr(prob), ptr(gt), ptr(rho), ptr(dout), E, T, H, C, ptr(dk), ptr(dv), ptr(G),
             stream_ptr())
        ent = "x2g_sbf_attention_bwd_src_fold" + opt
        ck.check(ent, mode, refs, "dk", dk)
        ck.check(ent, mode, refs, "dv", dv)
        ck.check(ent, mode, refs, "G", G)
        for l in range(8):  # every slot on its own scale (slot 7, the bias sum, is the largest)
            ck.check(ent, mode, _slot(refs, l), f"G[{l}]", G[:, l], "G_l")
        dw, db = _nan(cuda, D, 42), _nan(cuda, D)
        ws_b = int(lib.x2g_sbf_radial_wgrad_workspace(E, D))
        ws = torch.empty(max(ws_b, 1), dtype=torch.uint8, device=cuda)
        call("x2g_sbf_radial_wgrad", ptr(G), ptr(radial), E, D, ptr(dw), ptr(db), 0, ptr(ws), ws_b, stream_ptr())
        ck.check("x2g_sbf_radial_wgrad" + opt, mode, refs, "dW_sbf", dw, "dW_g")
        ck.check("x2g_sbf_radial_wgrad" + opt, mode, refs, "db_sbf", db, "db_g")


def _slot(refs, l):
    return tuple({"G_l": r["G"][:, l]} for r in refs)


@pytest.mark.parametrize("H,C,regime", [(4, 8, "unit"), (4, 16, "unit"), (16, 8, "unit"), (16, 8, "peaked"),
                                        (16, 8, "offset"), (8, 16, "unit"), (32, 4, "unit")])
def test_factorised_backward(cuda, H, C, regime):
    """x2g_sbf_attention_bwd_dst_g + x2g_sbf_attention_bwd_src_fold + x2g_sbf_radial_wgrad at D = 32, 64, 128
    (all three regimes at D = 128), without and with a 10-row per-destination table, g round trip / src_dst /
    src_row present and NULL: dq, d_edge, g, prob, seg_rho, dk, dv, G (whole and slot by slot), dW_sbf, db_sbf
    against the gradients of the fp64 reference."""
    g = _graph("edge")
    lg, x = _line_graph(g, cuda), _inputs("edge", regime, H, C)
    ck = _Checker("edge", regime, H, C)
    for mode in (EDGE_NONE, EDGE_PER_DST):
        _fold_backward(ck, lg, g, x, H, C, mode, cuda)
    ck.done()


# ------------------------------------------------------------------------------ c. center family
def _center_family(ck, lg, g, x, H, C, mode, cuda):
    from x2gnn import _lib
    from x2gnn._lib import call, ptr, stream_ptr

    regime = ck.key["regime"]
    E, T, D, N = g.E, g.T, H * C, g.n
    q, k, v, skip, dout, y, radial, W, b = _dev(x, cuda, "q", "k", "v", "skip", "dout", "y", "radial", "W", "b")
    edge = x["table"].to(cuda) if mode == EDGE_PER_DST else None
    src_row = lg.src_type if edge is not None else None
    assert int(_lib.load().x2g_sbf_attention_bwd_center_lds(lg.max_degree, H)) <= 160 * 1024

    def fwd_bufs():
        return [_nan(cuda, E, D), _nan(cuda, T, H), _nan(cuda, E, H), _nan(cuda, E, H), _nan(cuda, E, 2)]

    def check_fwd(ent, refs, bufs):
        out, alpha, smax, sden, rs = bufs
        for n, t in (("out", out), ("logits", alpha), ("seg_max", smax), ("seg_den", sden), ("row_mean", rs[:, 0]),
                     ("row_m2", rs[:, 1])):
            ck.check(ent, mode, refs, n, t)

    def backward(ent, refs, S, P, alpha, smax, sden):
        dq, dk, dv, G = _nan(cuda, E, D), _nan(cuda, E, D), _nan(cuda, E, D), _nan(cuda, E, 8, D)
        de = _nan(cuda, N, D) if edge is not None else None
        call("x2g_sbf_attention_bwd_center", ptr(q), ptr(k), ptr(v), ptr(edge), ptr(src_row), mode, ptr(S), ptr(P),
             ptr(b) if P is not None else None, ptr(y), ptr(lg.atom_rowptr), ptr(lg.edge_rev), ptr(lg.rev_trip),
             ptr(lg.center_order), ptr(alpha), ptr(smax), ptr(sden), ptr(dout), N, lg.max_degree, E, T, H, C, ptr(dq),
             ptr(dk), ptr(dv), ptr(G), ptr(de), ptr(torch.empty(2, T, H, device=cuda)), stream_ptr())
        for n, t in (("dq", dq), ("dk", dk), ("dv", dv), ("G", G)):
            ck.check(ent, mode, refs, n, t)
        ck.check(ent, mode, _slot(refs, 7), "G[7]", G[:, 7], "G_l")
        if edge is not None:  # per atom, not only after the keyed sum
            ck.check(ent, mode, refs, "d_edge_atom", de)

    # S rows given: x2g_sbf_attention_fwd_center, then the backward from S rows on its state
    refs = _ref(g.name, regime, H, C, mode, "S")
    S = x["S"].to(cuda)
    bufs = fwd_bufs()
    call("x2g_sbf_attention_fwd_center", ptr(q), ptr(k), ptr(v), ptr(skip), ptr(edge), ptr(src_row), mode, ptr(S), 0,
         ptr(lg.atom_rowptr), ptr(lg.edge_rev), ptr(lg.rev_trip), ptr(lg.center_order), 0, N, lg.max_degree, E, T, H, C,
         *[ptr(t) for t in bufs], stream_ptr())
    check_fwd("x2g_sbf_attention_fwd_center", refs, bufs)
    backward("x2g_sbf_attention_bwd_center[S rows]", refs, S, None, bufs[1], bufs[2], bufs[3])

    # lin_sbf fused: S_t rebuilt from the factors
    refs = _ref(g.name, regime, H, C, mode, "fac")
    po, pp, info, units, hubs, rows = lg.sched
    common = (ptr(q), ptr(k), ptr(v), ptr(skip), ptr(edge), ptr(src_row), mode, ptr(radial), ptr(y), ptr(W), ptr(b),
              ptr(lg.atom_rowptr), ptr(lg.edge_rev), ptr(lg.rev_trip))
    sf, tiled = "x2g_sbf_attention_fwd_center_sf", "x2g_sbf_attention_fwd_center_sf_tiled"
    deg_sorted = np.sort(g.deg)[::-1]
    n_big = int((deg_sorted > 17).sum())  # atoms beyond the untiled form's 17-row image (center_order leads with them)
    variants = {
        # one atom per workgroup by decreasing degree (the atoms of more than 17 rows through the tiled form)
        "one_atom": [(tiled, lg.center_order, None, None, 0, n_big, lg.max_degree, 0)] * (n_big > 0) +
                    [(sf, lg.center_order, None, None, n_big, N - n_big, max(int(deg_sorted[n_big]), 1), None)],
        # the model's launches: packs with atom_info, the leading hub units tiled (data.center_hubs)
        "packed": [(tiled, po, pp, info, 0, hubs, lg.max_degree, 0)] * (hubs > 0) +
                  [(sf, po, pp, info, hubs, units - hubs, rows, None)],
        # every atom through the source-tiled form
        "all_tiled": [(tiled, lg.center_order, None, None, 0, N, lg.max_degree, 0)],
    }
    state = None
    for vname, launches in variants.items():
        bufs = fwd_bufs()
        S2, P2 = _nan(cuda, T, D), _nan(cuda, E, 7, D)
        outs = (E, T, H, C, *[ptr(t) for t in bufs], ptr(S2), ptr(P2), stream_ptr())
        for entry, order, packs, inf, u0, nu, mrows, skip_rows in launches:
            extra = (mrows,) if skip_rows is None else (mrows, skip_rows)
            call(entry, *common, ptr(order), ptr(packs), ptr(inf), u0, nu, *extra, *outs)
        ent = (tiled if vname == "all_tiled" else sf) + f"[{vname}]"
        check_fwd(ent, refs, bufs)
        ck.check(ent, mode, refs, "S", S2)
        ck.check(ent, mode, refs, "P", P2)
        if vname == "packed":
            state = (P2, bufs[2], bufs[3])
    backward("x2g_sbf_attention_bwd_center[P rows]", refs, None, state[0], None, state[1], state[2])


@pytest.mark.parametrize("regime", ar.REGIMES)
@pytest.mark.parametrize("gname", ["edge", "mol"])
@pytest.mark.parametrize("H,C", [(16, 8), (8, 16), (32, 4)])
def test_center_family(cuda, H, C, gname, regime):
    """x2g_sbf_attention_fwd_center, _fwd_center_sf (one atom per workgroup; packed with atom_info),
    _fwd_center_sf_tiled (every atom; the model's split launch) and _bwd_center from S rows and from P rows, at
    D = 128, without and with the element-table edge term: every forward output, the stored S and P rows, dq,
    dk, dv, G and the per-atom edge gradient against the fp64 reference.  ``edge``: degree-1 atoms, atoms
    without edges, a hub of degree 40 (the center backward's LDS image of it fits 160 KiB at every head count:
    asserted); ``mol``: six S160 molecules with collate's shipped schedule."""
    g = _graph(gname)
    lg, x = _line_graph(g, cuda), _inputs(gname, regime, H, C)
    ck = _Checker(gname, regime, H, C)
    for mode in (EDGE_NONE, EDGE_PER_DST):
        _center_family(ck, lg, g, x, H, C, mode, cuda)
    ck.done()


# ------------------------------------------------------------------------------ d. operator level
@pytest.mark.parametrize("route", ["shipped", "center_s_rows", "dst_major_fold"])
def test_operator_routes(cuda, monkeypatch, route):
    """ops.sbf_attention under autograd on ``mol`` in the ``peaked`` regime through its three routes (which
    kernels ran is asserted from the calls made): the shipped one (fused forward + center backward from P rows),
    the center backward from S rows (ops._CENTER_P off) and the destination-major fold passes (ops._CENTER off).
    Each gives the reference's out, dq, dk, dv, table gradient, dW_sbf and db_sbf.  (The fold route's
    x2g_sbf_project reads the fp32 product radial[src] * Y, the fused forward forms it itself; the reference
    takes the unrounded product: a difference of 6e-8 of S, far inside the floors.)"""
    from test_gpu_model import record_calls
    from x2gnn import ops
    from x2gnn.plan import GraphPlan

    H, C = 16, 8
    g = _graph("mol")
    x = _inputs("mol", "peaked", H, C)
    refs = _ref("mol", "peaked", H, C, EDGE_PER_DST, "fac")
    if route == "center_s_rows":
        monkeypatch.setattr(ops, "_CENTER_P", False)
    elif route == "dst_major_fold":
        monkeypatch.setattr(ops, "_CENTER", False)
    lg = GraphPlan.from_atom_batch(g.batch.to(cuda)).lg
    assert np.array_equal(lg.trip_src.cpu().numpy(), g.trip[0]) and np.array_equal(lg.trip_dst.cpu().numpy(), g.trip[1])
    sbf, radial, y = _dev(x, cuda, "sbf", "radial", "y")
    lg.sbf_factors = (sbf, radial, y)
    leaves = [x[n].to(cuda).requires_grad_(True) for n in ("q", "k", "v", "skip", "table", "W", "b")]
    q, k, v, skip, table, W, b = leaves
    seen = record_calls(monkeypatch)
    out = ops.sbf_attention(q, k, v, skip, table, sbf, W, b, lg, H, C, edge_mode=ops.EDGE_PER_DST, edge_row=lg.dst_type)
    grads = torch.autograd.grad(out, leaves, x["dout"].to(cuda))
    names = [n for n, _ in seen]
    bwd_center = [a for n, a in seen if n == "x2g_sbf_attention_bwd_center"]
    if route == "dst_major_fold":
        assert not any("center" in n for n in names)
        for n in ("x2g_sbf_project", "x2g_sbf_attention_bwd_dst_g", "x2g_sbf_attention_bwd_src_fold",
                  "x2g_sbf_radial_wgrad"):
            assert names.count(n) == 1, n
        assert names.count("x2g_sbf_attention_fwd_stats") + names.count("x2g_sbf_attention_fwd") == 1
    else:
        assert names.count("x2g_sbf_attention_fwd_center_sf") == 1 and "x2g_sbf_project" not in names
        assert len(bwd_center) == 1 and "x2g_sbf_attention_bwd_dst_g" not in names
        s_rows, p_rows = bwd_center[0][6], bwd_center[0][7]  # (sbfproj, sbf_p): exactly one of the two
        assert (s_rows is None) == (route == "shipped") and (p_rows is None) == (route == "center_s_rows")
    ck = _Checker("mol", "peaked", H, C)
    ent = f"ops.sbf_attention[{route}]"
    ck.check(ent, EDGE_PER_DST, refs, "out", out)
    for n, t, rn in zip(("dq", "dk", "dv", "dskip", "d_table", "dW_sbf", "db_sbf"), grads,
                        ("dq", "dk", "dv", "dskip", "d_table", "dW", "db")):
        ck.check(ent, EDGE_PER_DST, refs, n, t, rn)
    ck.done()


def _write(path, all_rows=False):
    """Run every case of this module once and write the figures: per (entry point, output) the number of
    comparisons, the worst error / bound in each regime and the comparison it is worst in (graph, regime, H, C,
    mode, launch variant, error, e32, bound), and per entry point what was covered.  ``all_rows``: one row per
    (entry point, graph, regime, H, C, mode, output) instead (some 4500: not for committing)."""
    rc = pytest.main([os.path.abspath(__file__), "-m", "gpu", "-q", "-p", "no:cacheprovider"])
    rec = sys.modules["test_gpu_attention_fp64"].RECORD  # (the module as pytest imported it)
    f3 = lambda v: float(f"{v:.3e}")  # noqa: E731
    cover, agg = {}, {}
    for r in rec:
        entry, _, variant = r["entry"].partition("[")
        c = cover.setdefault(entry, dict(comparisons=0, graphs=set(), regimes=set(), shapes=set(), modes=set(),
                                         variants=set()))
        c["comparisons"] += 1
        for k, v in (("graphs", r["graph"]), ("regimes", r["regime"]), ("shapes", (r["H"] * r["C"], r["C"])),
                     ("modes", r["mode"]), ("variants", variant.rstrip("]"))):
            c[k].add(v)
        a = agg.setdefault((entry, r["output"].split("[")[0]), dict(n=0, by_regime={}, worst=None))
        ratio = r["err"] / r["bound"]
        a["n"] += 1
        a["by_regime"][r["regime"]] = max(a["by_regime"].get(r["regime"], 0.0), ratio)
        if a["worst"] is None or ratio > a["worst"][0]:
            a["worst"] = (ratio, r, variant.rstrip("]"))
    head = dict(pytest_exit_code=int(rc), comparisons=len(rec), errors="max|kernel - ref64| / max|ref64|",
                bounds_at_the_cap=sum(1 for r in rec if r["bound"] >= 1e-4 * (1 - 1e-12)),
                worst_error_over_bound={e: f3(max(a["by_regime"][g] for (e2, _), a in agg.items() if e2 == e
                                                  for g in a["by_regime"])) for e in sorted(cover)})
    cov_cols = ["entry", "comparisons", "graphs", "regimes", "D/C", "modes", "variants"]
    cov = [[e, c["comparisons"], " ".join(sorted(c["graphs"])), " ".join(sorted(c["regimes"])),
            " ".join(f"{d}/{ch}" for d, ch in sorted(c["shapes"])), " ".join(sorted(c["modes"])),
            " | ".join(sorted(v for v in c["variants"] if v))] for e, c in sorted(cover.items())]
    if all_rows:
        cols = ["entry", "graph", "regime", "H", "C", "mode", "output", "err", "e32", "bound"]
        rows = [[f3(r[c]) if isinstance(r[c], float) else r[c] for c in cols] for r in rec]
    else:
        cols = ["entry", "output", "comparisons", "worst err/bound: unit", "peaked", "offset", "worst in: graph",
                "regime", "H", "C", "mode", "variant", "err", "e32", "bound"]
        rows = []
        for (entry, output), a in sorted(agg.items()):
            _, r, variant = a["worst"]
            rows.append([entry, output, a["n"]] + [f3(a["by_regime"][g]) if g in a["by_regime"] else None
                                                   for g in ar.REGIMES] +
                        [r["graph"], r["regime"], r["H"], r["C"], r["mode"], variant, f3(r["err"]), f3(r["e32"]),
                         f3(r["bound"])])
    with open(path, "w") as f:  # one row per line
        lines = lambda rr: ",\n".join(json.dumps(row) for row in rr)  # noqa: E731
        f.write("{\n" + "".join(f" {json.dumps(k)}: {json.dumps(v)},\n" for k, v in head.items()))
        f.write(f' "covered_columns": {json.dumps(cov_cols)},\n "covered": [\n{lines(cov)}\n],\n')
        f.write(f' "columns": {json.dumps(cols)},\n "rows": [\n{lines(rows)}\n]}}\n')
    return int(rc)


if __name__ == "__main__":
    if len(sys.argv) not in (3, 4) or sys.argv[1] != "--write" or sys.argv[3:] not in ([], ["--all-rows"]):
        sys.exit("usage: python tests/test_gpu_attention_fp64.py --write profiles/attention_fp64_err.json [--all-rows]")
    sys.exit(_write(sys.argv[2], all_rows=len(sys.argv) == 4))
