"""ops._attention_route as a table: which forward and backward an sbf_attention call takes, what the forward stores
for that backward and why dropout is refused, on bare line-graph descriptions (no GPU: the one library entry the
route asks, x2g_sbf_attention_bwd_center_lds, is a host query).

The expected values are written out from the rules, not computed with the helpers under test:
- the center kernels take a call on a symmetric line graph (edge_rev) of known degree <= 128 at D = 128, channels a
  multiple of 4, without a per-triplet edge term, and with EDGE_PER_DST only when edge_row is lg.dst_type;
- the factors are the call's when sbf is lg.sbf_factors' product of 42 columns, D is 32 / 64 / 128, the edge term is
  not per triplet, and a per-destination table has its edge_row and at most 16 rows;
- the fused forward needs both; its untiled launches hold at most 17 rows, the rest goes through the tiled form;
- the center backward needs atom_type, an LDS image of 2248 B per row of the largest atom at 16 heads within
  160 KiB (degree <= 72), and T * heads * 8 B (P rows) or T * 512 B (S rows) below 2^31.
"""
import types

import numpy as np
import pytest
import torch

NONE, PER_TRIPLET, PER_DST = 0, 1, 2
SF, TILED = "x2g_sbf_attention_fwd_center_sf", "x2g_sbf_attention_fwd_center_sf_tiled"
DST_TYPE, SRC_TYPE, ATOM_TYPE, ORDER, PACK_ORDER, INFO = (object() for _ in range(6))
SBF, RADIAL, YLM = object(), object(), object()


def line_graph(**kw):
    """A symmetric batch as GraphPlan leaves it: 100 atoms of degree <= 12 in 7 packs of at most 16 rows."""
    f = dict(E=600, N=100, T=5000, edge_rev=object(), rev_trip=object(), max_degree=12, atom_type=ATOM_TYPE,
             src_type=SRC_TYPE, dst_type=DST_TYPE, center_order=ORDER, pack_order=PACK_ORDER,
             center_packs=np.zeros(8, dtype=np.int32), center_rows=16, pack_info=INFO, center_hubs=0,
             center_mixed=False, sbf_factors=(SBF, RADIAL, YLM), sbf_pending=None, mol_counts=None,
             _infer_tile_cache={})
    f.update(kw)
    return types.SimpleNamespace(**f)


def route(lg, mode=PER_DST, edge_rows=10, edge_row=DST_TYPE, H=16, C=8, own=True, sbf_dim=42, keeps=True,
          keep_alpha=False, dropout=False, grad=True):
    from x2gnn import ops

    if mode != PER_DST:
        edge_rows, edge_row = (None, None) if mode == NONE else (lg.T, None)
    return ops._attention_route(lg, mode, edge_rows, edge_row, H, C, own, sbf_dim, keeps, keep_alpha, dropout, grad)


def stored(r):
    return "".join(c for c, on in zip("aspr", (r.alpha, r.sproj, r.sbf_p, r.rstats)) if on)


# the shipped route and each switch off; (forward, backward, stored: a = logits, s = S rows, p = P rows, r = row stats)
@pytest.mark.parametrize("switch,forward,backward,keeps", [
    (None, "fused", "center_p", "pr"),
    ("_CENTER_P", "fused", "center_s", "asr"),
    ("_CENTER_BWD", "fused", "dst_fold", "asr"),
    ("_CENTER_SF", "center", "center_s", "asr"),
    ("_CENTER", "dst", "dst_fold", "asr"),
    ("_PACK_FWD", "fused", "center_p", "pr"),
    ("_LN_FUSE", "fused", "center_p", "p"),
])
def test_switches(monkeypatch, switch, forward, backward, keeps):
    from x2gnn import ops

    if switch is not None:
        monkeypatch.setattr(ops, switch, False)
    lg = line_graph()
    r = route(lg)
    assert (r.forward, r.backward, stored(r)) == (forward, backward, keeps)
    assert r.factors == (RADIAL, YLM) and r.reads_sbf == (forward != "fused") and r.tiles is None
    assert r.src_row is (None if switch == "_CENTER" else SRC_TYPE)
    if forward != "fused":
        assert r.launches is None and r.order is None and r.packs is None and r.info is None
    elif switch == "_PACK_FWD":  # one atom per workgroup by decreasing degree
        assert (r.order, r.packs, r.info, r.launches) == (ORDER, None, None, [(SF, 0, 100, 12, 0)])
    else:
        assert r.order is PACK_ORDER and r.packs is lg.center_packs and r.info is INFO
        assert r.launches == [(SF, 0, 7, 16, 0)]


def test_logits_only_when_somebody_reads_them():
    lg = line_graph()
    assert stored(route(lg, keep_alpha=True)) == "apr"  # return_attention
    r = route(lg, keeps=False, grad=False)  # no_grad: nothing kept
    assert (r.forward, r.backward, stored(r)) == ("fused", None, "r")
    r = route(lg, keeps=False)  # grad mode on, nothing requires grad
    assert (r.forward, r.backward, stored(r), r.tiles) == ("fused", None, "r", None)


def test_without_factors():
    """sbf is not the factors' product (a clone): S is projected and read, by the center forward on a symmetric
    graph; the backward is the plain two-pass one, which reads the logits and S."""
    r = route(line_graph(), own=False)
    assert (r.forward, r.backward, stored(r), r.factors, r.reads_sbf) == ("center", "dst_plain", "asr", None, True)
    assert route(line_graph(), sbf_dim=7 * 16).factors is None
    assert route(line_graph(sbf_factors=None), own=False).backward == "dst_plain"


def test_inference_tiles(monkeypatch):
    from x2gnn import ops

    monkeypatch.setattr(ops, "INFER_TILE", 4096)
    # four molecules of 25 atoms, 150 line nodes and 1250 triplets: three fit a tile of 4096 triplets
    counts = (np.full(4, 150), np.full(4, 1250), np.full(4, 25))
    whole = [(0, 450, 0, 3750, (0, 75)), (450, 600, 3750, 5000, (75, 100))]
    r = route(line_graph(mol_counts=counts), own=False, keeps=False, grad=False)
    assert (r.forward, r.backward, stored(r), r.tiles) == ("center", None, "sr", whole)
    # the fused forward has no S to tile; nor does a call with grad mode on
    assert route(line_graph(mol_counts=counts), keeps=False, grad=False).tiles is None
    assert route(line_graph(mol_counts=counts), own=False, keeps=False, grad=True).tiles is None
    # no atom counts (an edge may join two molecules): the destination-major kernel per tile, which needs the logits
    r = route(line_graph(mol_counts=counts[:2]), own=False, keeps=False, grad=False)
    assert (r.forward, stored(r)) == ("dst", "asr") and [t[:4] for t in r.tiles] == [t[:4] for t in whole]
    assert all(t[4] is None for t in r.tiles)
    # no host counts at all (the drop-in API): whole destination segments from the row pointer
    monkeypatch.setattr(ops, "INFER_TILE", 4)
    lg = line_graph(E=4, T=9, N=None, edge_rev=None, rev_trip=None, max_degree=None, atom_type=None,
                    trip_rowptr=torch.tensor([0, 3, 3, 8, 9], dtype=torch.int32))
    r = route(lg, mode=NONE, keeps=False, grad=False)
    assert (r.forward, r.backward) == ("dst", None)
    assert r.tiles == [(0, 2, 0, 3, None), (2, 3, 3, 8, None), (3, 4, 8, 9, None)]


@pytest.mark.parametrize("mode", [NONE, PER_DST])
def test_hub_takes_the_source_tiled_launch(mode):
    """A hub of degree 40 leading collate's packs (center_hubs = 1), then 6 packs of at most 17 rows."""
    lg = line_graph(max_degree=40, center_hubs=1, center_rows=17)
    r = route(lg, mode=mode)
    assert (r.forward, r.backward, stored(r)) == ("fused", "center_p", "pr")
    assert r.launches == [(TILED, 0, 1, 40, 0), (SF, 1, 6, 17, 0)]
    assert r.src_row is (SRC_TYPE if mode == PER_DST else None)
    # the device-made schedule: both forms over all units, each leaving out the other's
    r = route(line_graph(max_degree=40, center_mixed=True, center_rows=17), mode=mode)
    assert r.launches == [(TILED, 0, 7, 40, 17), (SF, 0, 7, 17, 0)]
    assert route(line_graph(center_mixed=True, center_rows=17), mode=mode).launches == [(SF, 0, 7, 17, 0)]


def test_not_symmetric():
    lg = line_graph(edge_rev=None, rev_trip=None, max_degree=None, atom_type=None)
    r = route(lg, mode=NONE)
    assert (r.forward, r.backward, stored(r), r.src_row) == ("dst", "dst_fold", "asr", None)
    r = route(lg, mode=PER_TRIPLET)  # a per-triplet edge term: no factors either
    assert (r.forward, r.backward, stored(r), r.factors) == ("dst", "dst_plain", "asr", None)


def test_d64_has_factors_but_no_center_route():
    r = route(line_graph(), H=8, C=8)
    assert (r.forward, r.backward, stored(r), r.factors) == ("dst", "dst_fold", "as", (RADIAL, YLM))
    assert route(line_graph(), H=64, C=2).forward == "dst"  # D = 128, channels no multiple of 4


@pytest.mark.parametrize("degree", [None, 129])
def test_degree_unknown_or_above_the_center_bound(degree):
    r = route(line_graph(max_degree=degree))
    assert (r.forward, r.backward, stored(r), r.src_row) == ("dst", "dst_fold", "asr", None)
    assert ("symmetric" if degree is None else "CENTER_MAX_DEGREE") in route(line_graph(max_degree=degree),
                                                                             dropout=True).dropout_refusal


def test_degree_65_unpacked_is_all_tiled_and_refuses_dropout():
    lg = line_graph(max_degree=65, center_packs=None)
    r = route(lg)
    assert (r.forward, r.backward, r.launches) == ("fused", "center_p", [(TILED, 0, 100, 65, 0)])
    assert "degree above 64" in route(lg, dropout=True).dropout_refusal
    # degree 73: the center backward's LDS image (73 x 2248 B) is above 160 KiB
    assert route(line_graph(max_degree=73, center_packs=None)).backward == "dst_fold"


def test_atom_type_absent():
    """The forward stays fused and stores S rows; the backward falls to the fold passes."""
    r = route(line_graph(atom_type=None))
    assert (r.forward, r.backward, stored(r)) == ("fused", "dst_fold", "asr")
    assert "P-row center backward" in route(line_graph(atom_type=None), dropout=True).dropout_refusal
    assert route(line_graph(atom_type=None), dropout=True, keeps=False, grad=False).dropout_refusal is None


def test_32bit_offsets(monkeypatch):
    from x2gnn import ops

    big = (1 << 31) // 512  # the first T whose S rows overflow; the (g, a) scratch is T * 128 B at 16 heads
    assert route(line_graph(T=big - 1)).backward == "center_p"
    assert route(line_graph(T=big)).backward == "center_p"
    assert route(line_graph(T=(1 << 31) // 128 - 1)).backward == "center_p"
    r = route(line_graph(T=(1 << 31) // 128))  # both refused
    assert (r.forward, r.backward, stored(r)) == ("fused", "dst_fold", "asr")
    monkeypatch.setattr(ops, "_CENTER_P", False)
    assert route(line_graph(T=big - 1)).backward == "center_s"
    assert route(line_graph(T=big)).backward == "dst_fold"


def test_table_of_17_rows_has_no_factors():
    r = route(line_graph(), edge_rows=17)
    assert (r.forward, r.backward, stored(r), r.factors, r.src_row) == ("center", "dst_plain", "asr", None, SRC_TYPE)
    assert route(line_graph(), edge_rows=16).forward == "fused"
    assert "factors" in route(line_graph(), edge_rows=17, dropout=True).dropout_refusal


def test_edge_row_not_the_line_graphs_own():
    r = route(line_graph(), edge_row=object())
    assert (r.forward, r.backward, stored(r), r.src_row) == ("dst", "dst_fold", "asr", None)
    assert r.factors == (RADIAL, YLM)
    assert "edge_row is not" in route(line_graph(), edge_row=object(), dropout=True).dropout_refusal
    r = route(line_graph(), edge_row=None)  # one edge row per destination line node: no table to stage
    assert (r.forward, r.backward, r.factors) == ("dst", "dst_plain", None)


def test_dropout_refusals_in_order(monkeypatch):
    from x2gnn import ops

    lg = line_graph()
    assert route(lg, dropout=True).dropout_refusal is None
    assert route(lg, dropout=False, mode=PER_TRIPLET).dropout_refusal is None  # (asked only with dropout)
    assert "per-triplet" in route(lg, dropout=True, mode=PER_TRIPLET).dropout_refusal
    assert "heads * channels = 64" in route(lg, dropout=True, H=8).dropout_refusal
    assert "factors" in route(lg, dropout=True, own=False).dropout_refusal
    assert "LDS image" in route(line_graph(center_rows=40), dropout=True).dropout_refusal  # a pack of 40 rows
    for switch in ("_CENTER", "_CENTER_SF", "_CENTER_P"):
        with monkeypatch.context() as m:
            m.setattr(ops, switch, False)
            assert "switched off" in route(lg, dropout=True, mode=PER_TRIPLET).dropout_refusal, switch
    # every condition at once: the first in order is named
    bad = line_graph(edge_rev=None, max_degree=None, atom_type=None)
    assert "per-triplet" in route(bad, dropout=True, mode=PER_TRIPLET, H=8, own=False).dropout_refusal
    assert "symmetric" in route(bad, dropout=True, H=8, own=False).dropout_refusal


def test_each_predicate_runs_once(monkeypatch):
    from x2gnn import ops

    counts = {}
    for fn in ("_center_split", "_center_rows", "_center_bwd_ok"):
        def counted(*a, _inner=getattr(ops, fn), _fn=fn, **kw):
            counts[_fn] = counts.get(_fn, 0) + 1
            return _inner(*a, **kw)
        monkeypatch.setattr(ops, fn, counted)
    route(line_graph(), dropout=True)
    assert counts == {"_center_split": 1, "_center_rows": 1, "_center_bwd_ok": 1}
    counts.clear()
    route(line_graph(T=(1 << 31) // 128))  # the P-row form refused: the S-row form is asked too
    assert counts == {"_center_split": 1, "_center_rows": 1, "_center_bwd_ok": 2}
