"""ops.sbf_attention's kernel calls, route by route: the sequence of C-ABI calls one forward (and backward) makes is
equal, in order, to the sequence recorded before the host layer's routing moved into ops._attention_route
(tests/golden/attention_calls.json), and the route is decided once per call.

A call is recorded as its entry point and its arguments reduced by the entry's argtypes: NULL or not for a
pointer parameter, the value for any other.  ``python tests/test_gpu_attention_route.py --write PATH`` records
every case again (only to be run on a tree whose calls are known to be right).
"""
import contextlib
import copy
import ctypes
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":  # (run as a script: the paths conftest.py sets up for pytest)
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "x2-gnn_amd"), os.path.join(_root, "tests")]

from conftest import GOLDEN as GOLDEN_DIR
from test_gpu_attention_fp64 import EDGE_NONE, EDGE_PER_DST, EDGE_PER_TRIPLET, _graph, _inputs, _line_graph
from test_gpu_model import record_calls

pytestmark = pytest.mark.gpu

RECORDED = os.path.join(GOLDEN_DIR, "attention_calls.json")


def reduce_calls(seen):
    """test_gpu_model.record_calls' [(name, args)] as [[name, [NULL or not per pointer parameter, any other value]]]."""
    from x2gnn import _lib

    out = []
    for name, args in seen:
        types = _lib.SIGNATURES.get(name) or _lib.STAGED_SIGNATURES[name]
        assert len(types) == len(args), name
        row = []
        for t, a in zip(types, args):
            a = a.value if isinstance(a, ctypes._SimpleCData) else a
            if t is ctypes.c_void_p or not isinstance(a, (int, float)):
                row.append("ptr" if a else "NULL")
            else:
                row.append(a)
        out.append([name, row])
    return out


_LGS = {}


def _lg(gname, cuda):
    """``mol`` through GraphPlan.from_atom_batch; ``edge`` with data.center_packs' schedule on the line graph (the
    hub of degree 40 leads it: the source-tiled launch); ``directed`` as vertex_to_edge leaves it."""
    if gname in _LGS:
        return _LGS[gname]
    from x2gnn.plan import GraphPlan

    g = _graph(gname)
    if gname == "mol":
        lg = GraphPlan.from_atom_batch(g.batch.to(cuda)).lg
    else:
        lg = copy.copy(_line_graph(g, cuda))  # (the fp64 tests' own line graph stays as they made it)
        if gname == "edge":
            lg.pack_order, lg.center_packs, lg.pack_info, _, lg.center_hubs, lg.center_rows = lg.sched
    lg.src_csr()  # (built on first use: not a call of whichever case happens to come first)
    _LGS[gname] = lg
    return lg


# name: (graph, H, C, edge mode, sbf is the factors' product, ops switches, grad, sbf_attention keywords)
_D = dict(graph="mol", H=16, C=8, mode=EDGE_PER_DST, factors=True, sw={}, grad=True, kw={})
CASES = {
    "mol": _D,
    "mol_center_p_off": dict(_D, sw=dict(_CENTER_P=False)),
    "mol_center_bwd_off": dict(_D, sw=dict(_CENTER_BWD=False)),
    "mol_center_sf_off": dict(_D, sw=dict(_CENTER_SF=False)),
    "mol_center_off": dict(_D, sw=dict(_CENTER=False)),
    "mol_pack_fwd_off": dict(_D, sw=dict(_PACK_FWD=False)),
    "mol_return_attention": dict(_D, kw=dict(return_attention=True)),
    "mol_no_grad": dict(_D, grad=False),
    "mol_dropout": dict(_D, kw=dict(dropout=0.25)),
    "mol_no_factors": dict(_D, factors=False),
    "mol_no_factors_no_grad_tiled": dict(_D, factors=False, grad=False, sw=dict(INFER_TILE=4096)),
    "edge_none": dict(_D, graph="edge", mode=EDGE_NONE),
    "edge_per_dst": dict(_D, graph="edge"),
    "directed_none": dict(_D, graph="directed", mode=EDGE_NONE),
    "directed_per_triplet": dict(_D, graph="directed", mode=EDGE_PER_TRIPLET),
    "directed_no_grad_tiled": dict(_D, graph="directed", mode=EDGE_NONE, grad=False, sw=dict(INFER_TILE="T // 3")),
    "mol_d64": dict(_D, H=8, C=8),
}


def run_case(name, cuda, between=None):
    """The reduced calls of one case's forward (and backward); ``between``: an ops switch turned off after the
    forward."""
    from x2gnn import ops

    c = CASES[name]
    H, C, mode = c["H"], c["C"], c["mode"]
    lg, x = _lg(c["graph"], cuda), _inputs(c["graph"], "unit", H, C)
    sbf, radial, y = (x[n].to(cuda) for n in ("sbf", "radial", "y"))
    lg.sbf_factors = (sbf, radial, y)
    if not c["factors"]:
        sbf = sbf.clone()
    edge = {EDGE_NONE: None, EDGE_PER_TRIPLET: "e_trip", EDGE_PER_DST: "table"}[mode]
    leaves = [x[n].to(cuda).requires_grad_(True) for n in ("q", "k", "v", "skip", edge, "W", "b") if n is not None]
    q, k, v, skip = leaves[:4]
    W, b = leaves[-2:]
    edge = leaves[4] if edge is not None else None
    kw = dict(c["kw"])
    if "dropout" in kw:
        kw["dropout"] = (kw["dropout"], torch.tensor([1234, 5], dtype=torch.int64, device=cuda), 0)
    with pytest.MonkeyPatch.context() as mp, (contextlib.nullcontext() if c["grad"] else torch.no_grad()):
        for switch, value in c["sw"].items():
            mp.setattr(ops, switch, lg.T // 3 if value == "T // 3" else value)
        seen = record_calls(mp)
        out = ops.sbf_attention(q, k, v, skip, edge, sbf, W, b, lg, H, C, edge_mode=mode,
                                edge_row=lg.dst_type if mode == EDGE_PER_DST else None, **kw)
        out = out[0] if isinstance(out, tuple) else out
        if between is not None:
            mp.setattr(ops, between, False)
        if c["grad"]:
            torch.autograd.grad(out, leaves, x["dout"].to(cuda))
        torch.cuda.synchronize()
    return reduce_calls(seen)


@pytest.fixture(scope="module")
def recorded():
    with open(RECORDED) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_calls_equal_the_recorded_ones(cuda, recorded, name):
    got = json.loads(json.dumps(run_case(name, cuda)))
    want = recorded[name]
    assert [n for n, _ in got] == [n for n, _ in want]
    assert got == want
    names = [n for n, _ in got]
    if name.endswith("_tiled"):  # at least two tiles, and whole molecules take the center forward
        assert names.count("x2g_sbf_project") >= 2
        assert ("x2g_sbf_attention_fwd_center" in names) == (name.startswith("mol"))


@pytest.mark.parametrize("name", ["mol", "mol_dropout"])
def test_route_is_decided_once_and_the_backward_follows_it(cuda, monkeypatch, name):
    """One training forward and backward evaluates _center_split and _center_rows once and _center_bwd_ok at most
    twice; flipping _CENTER or _CENTER_P between the forward and the backward does not change the backward's
    calls (it runs what the forward stored for)."""
    from x2gnn import ops

    counts = {}
    for fn in ("_center_split", "_center_rows", "_center_bwd_ok"):
        def counted(*a, _inner=getattr(ops, fn), _fn=fn, **kw):
            counts[_fn] = counts.get(_fn, 0) + 1
            return _inner(*a, **kw)
        monkeypatch.setattr(ops, fn, counted)
    plain = run_case(name, cuda)
    assert counts["_center_split"] == 1 and counts["_center_rows"] == 1 and counts["_center_bwd_ok"] <= 2, counts
    for flipped in ("_CENTER", "_CENTER_P"):
        assert run_case(name, cuda, between=flipped) == plain, flipped


if __name__ == "__main__":
    assert sys.argv[1] == "--write", __doc__
    dev = torch.device("cuda:0")
    rec = {name: run_case(name, dev) for name in CASES}
    for name, calls in rec.items():
        print(name, [n for n, _ in calls])
    with open(sys.argv[2], "w") as f:
        f.write("{\n" + ",\n".join(f' "{n}": [\n  ' + ",\n  ".join(json.dumps(c) for c in calls) + "\n ]"
                                   for n, calls in rec.items()) + "\n}\n")
