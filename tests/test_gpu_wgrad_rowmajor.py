"""Row-major operands of the tiled weight-gradient launch (x2g_tiled_job.layout) and the producers
that no longer write T-layout duplicates: the projection backward (g_t NULL), the projection forward
(x_t NULL) and the chain forward (X2G_CHAIN_IN0_ROWMAJOR).

The shapes are chosen for where the kernel can go wrong, not for the workload: a partial last tile
(R % 16 != 0), fewer rows than a tile, strided and bias-less jobs, and more tiles than the flat launch
has workgroups.  It starts min(tiles, 512) workgroups, so up to R = 1000 (5 x 63 tiles) every workgroup
owns exactly one tile.  R = 4001 (1255 tiles, 2-3 per workgroup), R = 10007 (3130 tiles, 6-7 per
workgroup) and the row counts (20005, 9001, 1000, 37) (1880 tiles, 3-4 per workgroup) make workgroups
run several steps of the double-buffered loop with both tiles of a step, tile offsets past 0 and
multi-tile segments that end in a partial tile, and make some of them cross from a job of one layout
into a job of another.  x2g_chain_wgrad, the same launch over a chain's contiguous T planes, is checked at
the ABI against it."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

T, DY, X = 0, 1, 2  # x2g_tiled_job.layout bits (X2G_TILED_DY_ROWMAJOR, X2G_TILED_X_ROWMAJOR)


def _t_layout(x):
    """Row-major [R, 128] -> the tiled-transposed layout (x2g.h): 16-row tiles, feature-major inside a
    tile, padding rows zero."""
    R, F = x.shape
    nt = (R + 15) // 16
    xp = torch.zeros(nt * 16, F, device=x.device, dtype=x.dtype)
    xp[:R] = x
    return xp.view(nt, 16, F).permute(0, 2, 1).contiguous().view(-1)


def _guarded(x):
    """A copy of x whose storage goes on with a tile of NaN rows: a read past row R of a row-major
    operand would poison the sums."""
    R, F = x.shape
    buf = torch.full(((R + 16) * F,), float("nan"), device=x.device, dtype=x.dtype)
    buf[:R * F] = x.reshape(-1)
    return buf


def _run_flat(cuda, rows, dys, xs, layouts, strided, nobias, per_job_rows):
    """One flat launch (slab sums included) of len(rows) jobs; returns ([dW], [db])."""
    from x2gnn import _lib, ops
    from x2gnn._lib import ptr, stream_ptr

    lib = _lib.load()
    n = len(rows)
    keep, jobs, dws, dbs = [], [], [], []
    for j in range(n):
        dy = _guarded(dys[j]) if layouts[j] & DY else _t_layout(dys[j])
        x = _guarded(xs[j]) if layouts[j] & X else _t_layout(xs[j])
        keep += [dy, x]
        db = None if j in nobias else torch.zeros(128, device=cuda)
        if j in strided:  # a [128, 100] block at column 50 of a [128, 300] weight
            big = torch.full((128, 300), 7.0, device=cuda)
            dws.append(big)
            jobs.append(ops.TiledJob(dy.data_ptr(), x.data_ptr(), big.data_ptr() + 4 * 50, ptr(db), 300, 100, layouts[j]))
        else:
            dw = torch.zeros(128, 128, device=cuda)
            dws.append(dw)
            jobs.append(ops.TiledJob(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), ptr(db), 0, 0, layouts[j]))
        dbs.append(db)
    arr = (ops.TiledJob * n)(*jobs)
    if per_job_rows:
        r = (ctypes.c_int64 * n)(*rows)
        wsb = int(lib.x2g_tiled_wgrad_flat_rows_workspace(r, n, 128))
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=cuda)
        assert lib.x2g_tiled_wgrad_flat_rows(arr, r, n, 128, 0, None, ptr(ws), wsb, stream_ptr()) == 0
    else:
        wsb = int(lib.x2g_tiled_wgrad_flat_workspace(rows[0], 128, n))
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=cuda)
        assert lib.x2g_tiled_wgrad_flat(arr, n, rows[0], 128, 0, None, ptr(ws), wsb, stream_ptr()) == 0
    torch.cuda.synchronize()
    return dws, dbs


def _check_flat(cuda, rows, layouts, strided, nobias, per_job_rows):
    n = len(rows)
    g = torch.Generator(device=cuda).manual_seed(sum(rows) + n)
    dys = [torch.randn(R, 128, device=cuda, generator=g) for R in rows]
    xs = [torch.randn(R, 128, device=cuda, generator=g) for R in rows]
    dw_r, db_r = _run_flat(cuda, rows, dys, xs, layouts, strided, nobias, per_job_rows)
    dw_t, db_t = _run_flat(cuda, rows, dys, xs, [T] * n, strided, nobias, per_job_rows)
    for j in range(n):
        # the same bits as the launch on the T-layout copies
        assert torch.equal(dw_r[j], dw_t[j]), j
        assert (db_r[j] is None and db_t[j] is None) or torch.equal(db_r[j], db_t[j]), j
        ref = dys[j].double().t() @ xs[j].double()
        if j in strided:
            big = dw_r[j]
            assert torch.equal(big[:, :50], torch.full_like(big[:, :50], 7.0))
            assert torch.equal(big[:, 150:], torch.full_like(big[:, 150:], 7.0))
            got, ref = big[:, 50:150].double(), ref[:, :100]
        else:
            got = dw_r[j].double()
        assert float((got - ref).abs().max()) <= 2e-5 * float(ref.abs().max()) + 1e-6, j
        if db_r[j] is not None:
            rb = dys[j].double().sum(0)
            assert float((db_r[j].double() - rb).abs().max()) <= 2e-5 * float(rb.abs().max()) + 1e-6, j


@pytest.mark.parametrize("R", [1, 16, 37, 100, 1000, 4001, 10007])
def test_tiled_wgrad_flat_rowmajor_equals_t_layout(cuda, R):
    """x2g_tiled_wgrad_flat with row-major operands: five jobs, every layout pair, one strided and one
    without bias; bit for bit the all-T launch, and within the T path's tolerance of fp64 torch.  At
    4001 and 10007 rows a workgroup owns several tiles and some span two jobs (module docstring)."""
    _check_flat(cuda, [R] * 5, [T, DY, X, DY | X, DY | X], strided={3}, nobias={2}, per_job_rows=False)


@pytest.mark.parametrize("rows", [(1000, 1000, 144, 37), (20005, 9001, 1000, 37)])
def test_tiled_wgrad_flat_rows_rowmajor_equals_t_layout(cuda, rows):
    """x2g_tiled_wgrad_flat_rows with a row count per job and mixed layouts; the row-major operands are
    followed by NaN rows, so a partial last tile (144 = 9 whole tiles, the others partial) that read past
    its rows would show.  The second case has 3-4 tiles per workgroup and ends every job but the last
    in the middle of a workgroup's range."""
    _check_flat(cuda, list(rows), [DY | X, X, DY, DY | X], strided={1}, nobias={0, 2}, per_job_rows=True)


def test_tiled_wgrad_refuses_unknown_layout_bits(cuda):
    """An unknown layout bit is refused by the flat entry; nothing runs."""
    from x2gnn import _lib, ops
    from x2gnn._lib import ptr, stream_ptr

    lib = _lib.load()
    a = torch.zeros(16 * 128, device=cuda)
    dw = torch.full((128, 128), 3.0, device=cuda)
    arr = (ops.TiledJob * 1)(ops.TiledJob(a.data_ptr(), a.data_ptr(), dw.data_ptr(), None, 0, 0, 4))
    wsb = int(lib.x2g_tiled_wgrad_flat_workspace(16, 128, 1))
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    assert lib.x2g_tiled_wgrad_flat(arr, 1, 16, 128, 0, None, ptr(ws), wsb, stream_ptr()) != 0
    torch.cuda.synchronize()
    assert torch.equal(dw, torch.full_like(dw, 3.0))


@pytest.mark.parametrize("n,nobias", [(1, None), (3, None), (3, 1)])
@pytest.mark.parametrize("R", [1, 17, 37])
def test_chain_wgrad_is_the_flat_launch_on_t_planes(cuda, R, n, nobias):
    """x2g_chain_wgrad at the ABI: n stages over contiguous T planes (stage s at + s * x2g_chain_t_floats),
    stage ``nobias`` with db[s] NULL; fewer rows than a tile, one tile plus a row, a ragged third tile.
    dW / db within the weight-gradient bound of fp64 and the bits of x2g_tiled_wgrad_flat on the same
    operands; X2G_ACCUM_WGRAD adds them to the destination's contents (one fp32 add of the summed slabs);
    a workspace one byte short and X2G_DEFER_SLAB_SUM leave the destinations alone."""
    from x2gnn import _lib, ops
    from x2gnn._lib import ptr, stream_ptr

    lib = _lib.load()
    g = torch.Generator(device=cuda).manual_seed(100 * R + 10 * n + (nobias or 0))
    dz = torch.randn(n, R, 128, device=cuda, generator=g)
    x = torch.randn(n, R, 128, device=cuda, generator=g)
    tf = int(lib.x2g_chain_t_floats(R, 128))
    dz_t = torch.stack([_t_layout(dz[s]) for s in range(n)])
    in_t = torch.stack([_t_layout(x[s]) for s in range(n)])
    assert dz_t.shape == (n, tf)
    wsb = int(lib.x2g_chain_wgrad_workspace(R, 128, n))
    assert wsb == int(lib.x2g_tiled_wgrad_flat_workspace(R, 128, n)) > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)

    def fresh(fill):
        dw = torch.full((n, 128, 128), fill, device=cuda)
        db = torch.full((n, 128), fill, device=cuda)
        return dw, db

    def chain(dw, db, flags, ws_bytes):
        dwa = (ctypes.c_void_p * n)(*[dw[s].data_ptr() for s in range(n)])
        dba = (ctypes.c_void_p * n)(*[None if s == nobias else db[s].data_ptr() for s in range(n)])
        rc = lib.x2g_chain_wgrad(ptr(in_t), ptr(dz_t), n, R, 128, dwa, dba, flags, ptr(ws), ws_bytes, stream_ptr())
        torch.cuda.synchronize()
        return rc

    dw, db = fresh(0.0)
    assert chain(dw, db, 0, wsb) == 0
    for s in range(n):
        ref = dz[s].double().t() @ x[s].double()
        assert float((dw[s].double() - ref).abs().max()) <= 2e-5 * float(ref.abs().max()) + 1e-6, s
        if s == nobias:
            assert torch.equal(db[s], torch.zeros_like(db[s]))
        else:
            rb = dz[s].double().sum(0)
            assert float((db[s].double() - rb).abs().max()) <= 2e-5 * float(rb.abs().max()) + 1e-6, s

    fw, fb = fresh(0.0)
    jobs = (ops.TiledJob * n)(*[ops.TiledJob(dz_t[s].data_ptr(), in_t[s].data_ptr(), fw[s].data_ptr(),
                                             None if s == nobias else fb[s].data_ptr(), 0, 0, T) for s in range(n)])
    assert lib.x2g_tiled_wgrad_flat(jobs, n, R, 128, 0, None, ptr(ws), wsb, stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dw, fw) and torch.equal(db, fb)

    aw, ab = fresh(3.0)
    assert chain(aw, ab, ops.ACCUM_WGRAD, wsb) == 0
    assert torch.equal(aw, 3.0 + dw) and torch.equal(ab, 3.0 + db)

    for flags, ws_bytes, want in ((0, wsb - 1, 1003), (ops.DEFER_SLAB_SUM, wsb, 0)):
        uw, ub = fresh(3.0)
        assert chain(uw, ub, flags, ws_bytes) == want
        assert torch.equal(uw, torch.full_like(uw, 3.0)) and torch.equal(ub, torch.full_like(ub, 3.0))


def _record(monkeypatch):
    """Every C-ABI entry ops calls from here on: [(name, args)]."""
    from x2gnn import _lib, ops

    seen, inner = [], _lib.call

    def rec(name, *args):
        seen.append((name, args))
        return inner(name, *args)

    monkeypatch.setattr(ops, "call", rec)
    return seen


def _as_sinks(params):
    """Mark leaf tensors as bucket-backed (ops.grad_sink): a zeroed .grad the kernels sum into."""
    for p in params:
        p.grad = torch.zeros_like(p)
        p._x2g_grad_sink = True


@pytest.mark.parametrize("xrow", [True, False])
@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("E", [37, 1000])
def test_conv_proj_fused_rowmajor_wgrad(cuda, monkeypatch, E, deferred, xrow):
    """ops._ConvProjFusedFn: no T-layout copy of x (x_t NULL) or of the four gradients (g_t NULL), the
    weight gradients read them row-major, in a launch of their own and queued on a deferral; every
    gradient against fp64 torch.  xrow False: ops.WGRAD_X_ROWMAJOR off, x_t written and read as before."""
    from x2gnn import ops

    monkeypatch.setattr(ops, "WGRAD_X_ROWMAJOR", xrow)

    RR = 6
    g = torch.Generator(device=cuda).manual_seed(E + RR)
    x = torch.randn(E, 128, device=cuda, generator=g)
    rbf = torch.rand(E, RR, device=cuda, generator=g)
    wr = torch.randn(128, RR, device=cuda, generator=g) / 2
    W = [torch.randn(128, 128, device=cuda, generator=g) / 11.3 for _ in range(4)]
    B = [0.1 * torch.randn(128, device=cuda, generator=g) for _ in range(4)]
    gs = [torch.randn(E, 128, device=cuda, generator=g) for _ in range(4)]

    def leaves(dtype):
        return [t.detach().to(dtype).requires_grad_(True) for t in [x, rbf, wr] + [v for p in zip(W, B) for v in p]]

    ref = leaves(torch.float64)
    xx, rb, w_r = ref[:3]
    xs = xx * (rb @ w_r.t())
    outs = [xx @ ref[3].t() + ref[4], xs @ ref[5].t() + ref[6], xs @ ref[7].t() + ref[8], xx @ ref[9].t() + ref[10]]
    torch.autograd.backward(outs, [t.double() for t in gs])

    ins = leaves(torch.float32)
    seen = _record(monkeypatch)
    if deferred:
        _as_sinks(ins[2:])
        with ops.deferred_wgrad():
            torch.autograd.backward(ops._ConvProjFusedFn.apply(*ins), gs)
    else:
        torch.autograd.backward(ops._ConvProjFusedFn.apply(*ins), gs)
    torch.cuda.synchronize()
    fwd = [a for n, a in seen if n == "x2g_conv_proj_fwd"]
    bwd = [a for n, a in seen if n == "x2g_conv_proj_bwd_gate"]
    assert len(fwd) == 1 and (fwd[0][-3] is None) == xrow  # (..., x_t, xs_t, stream)
    assert len(bwd) == 1 and all(not bwd[0][0][i].g_t for i in range(4))
    flat = [a for n, a in seen if n.startswith("x2g_tiled_wgrad_flat") and not n.endswith("workspace")]
    assert len(flat) == 1 and [flat[0][0][i].layout for i in range(4)] == [DY | (X if xrow else T), DY, DY, DY | (X if xrow else T)]
    for i, (a, r) in enumerate(zip(ins, ref)):
        scale = float(r.grad.abs().max()) + 1e-30
        assert float((a.grad.double() - r.grad).abs().max()) <= 2e-5 * scale + 1e-6, i


def _graph_ln_ref(x, rowptr, eps):
    """PyG LayerNorm(mode='graph', affine=False) per row segment (two-pass, biased variance)."""
    out = torch.empty_like(x)
    rp = rowptr.tolist()
    for g in range(len(rp) - 1):
        a, b = rp[g], rp[g + 1]
        if b > a:
            xc = x[a:b] - x[a:b].mean()
            out[a:b] = xc / torch.sqrt((xc * xc).mean() + eps)
    return out


def _chain_ref(x, res, ws, bs, flags):
    """fp64 torch restatement of x2g_chain_fwd (include/x2g.h: row chains)."""
    from x2gnn import ops

    held, cur = None, x
    for w, b, f in zip(ws, bs, flags):
        if f & ops.CHAIN_RES_EXT:
            held = res
        if f & ops.CHAIN_HOLD:
            held = cur
        z = cur @ w.t() + b
        y = torch.nn.functional.silu(z) if f & ops.CHAIN_SILU else z
        if f & (ops.CHAIN_RES_HELD | ops.CHAIN_RES_EXT):
            y = y + held
        cur = y
    return cur


@pytest.mark.parametrize("with_ln", [False, True])
@pytest.mark.parametrize("R", [37, 1000])
def test_row_chain_rowmajor_stage0_deferred(cuda, monkeypatch, R, with_ln):
    """ops.row_chain inside ops.deferred_wgrad() with bucket-backed parameters: the forward runs with
    X2G_CHAIN_IN0_ROWMAJOR (no T plane 0) and stage 0's weight gradient reads the saved row-major input
    (the LayerNorm output with ln=, else x) in the flat launch; output and every gradient vs fp64 torch."""
    from x2gnn import ops

    S, H, RH, RE = ops.CHAIN_SILU, ops.CHAIN_HOLD, ops.CHAIN_RES_HELD, ops.CHAIN_RES_EXT
    flags = [S | H, S | RH, S | RE, S | H, S | RH, S | H, S | RH]
    counts = [20, 0, 17] if R == 37 else [165] * 6 + [10]
    rowptr = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32)
    assert int(rowptr[-1]) == R
    eps = 1e-8
    gd = torch.Generator(device=cuda).manual_seed(R + int(with_ln))
    lins = [torch.nn.Linear(128, 128).to(cuda) for _ in flags]
    with torch.no_grad():
        for m in lins:
            m.weight.copy_(torch.randn(128, 128, device=cuda, generator=gd) / 11.3)
            m.bias.copy_(torch.randn(128, device=cuda, generator=gd) * 0.1)
    x = (torch.randn(R, 128, device=cuda, generator=gd) * 2.0 + 0.7).requires_grad_(True)
    res = torch.randn(R, 128, device=cuda, generator=gd).requires_grad_(True)
    dy = torch.randn(R, 128, device=cuda, generator=gd)
    ln = None
    if with_ln:
        xd = x.detach()
        mu_r = xd.mean(1)
        stats = torch.stack([mu_r, ((xd - mu_r[:, None]) ** 2).sum(1)], 1).contiguous()
        ln = (stats, rowptr.to(cuda), len(counts), eps)
    _as_sinks([p for m in lins for p in (m.weight, m.bias)])
    seen = _record(monkeypatch)
    with ops.deferred_wgrad():
        y = ops.row_chain(x, res, lins, flags, ln=ln)
        y.backward(dy)
    torch.cuda.synchronize()
    fwd = [a for n, a in seen if n in ("x2g_chain_fwd", "x2g_chain_fwd_ln")]
    assert len(fwd) == 1
    st = next(a for a in fwd[0] if isinstance(a, ctypes.Array))
    assert st[0].flags & ops.CHAIN_IN0_ROWMAJOR and not any(st[i].flags & ops.CHAIN_IN0_ROWMAJOR for i in range(1, 7))
    flat = [a for n, a in seen if n == "x2g_tiled_wgrad_flat_rows"]
    assert len(flat) == 1 and [flat[0][0][i].layout for i in range(7)] == [X, T, T, T, T, T, T]

    x64 = x.detach().double().requires_grad_(True)
    r64 = res.detach().double().requires_grad_(True)
    wd = [m.weight.detach().double().requires_grad_(True) for m in lins]
    bd = [m.bias.detach().double().requires_grad_(True) for m in lins]
    yr = _chain_ref(_graph_ln_ref(x64, rowptr, eps) if with_ln else x64, r64, wd, bd, flags)
    yr.backward(dy.double())
    torch.testing.assert_close(y.double(), yr, rtol=1e-5, atol=1e-5)
    # (the existing chain tests' bounds: 1e-5 flat, with the LayerNorm backward 1e-5 of the largest gradient)
    torch.testing.assert_close(x.grad.double(), x64.grad, rtol=1e-5,
                               atol=1e-5 * float(x64.grad.abs().max()) if with_ln else 1e-5)
    torch.testing.assert_close(res.grad.double(), r64.grad, rtol=1e-5, atol=1e-5)
    for m, w, b in zip(lins, wd, bd):
        assert float((m.weight.grad.double() - w.grad).abs().max()) <= 2e-5 * float(w.grad.abs().max()) + 1e-6
        assert float((m.bias.grad.double() - b.grad).abs().max()) <= 2e-5 * float(b.grad.abs().max()) + 1e-6


def test_chain_fwd_refuses_in0_rowmajor_past_stage0(cuda):
    """X2G_CHAIN_IN0_ROWMAJOR on a stage other than 0 is refused at the ABI and nothing runs; on stage 0
    the chain runs and leaves plane 0 of in_t alone."""
    from x2gnn import _lib, ops
    from x2gnn._lib import ptr, stream_ptr

    lib = _lib.load()
    R = 37
    x = torch.randn(R, 128, device=cuda)
    w = torch.randn(128, 128, device=cuda) / 11.3
    zs = [torch.empty(R, 128, device=cuda) for _ in range(2)]
    y = torch.full((R, 128), 5.0, device=cuda)
    tf = int(lib.x2g_chain_t_floats(R, 128))
    in_t = torch.full((2, tf), 9.0, device=cuda)
    S, RM = ops.CHAIN_SILU, ops.CHAIN_IN0_ROWMAJOR

    def run(flags):
        st = (ops.ChainStage * 2)(ops.ChainStage(w.data_ptr(), None, zs[0].data_ptr(), None, None, flags[0]),
                                  ops.ChainStage(w.data_ptr(), None, zs[1].data_ptr(), y.data_ptr(), None, flags[1]))
        rc = lib.x2g_chain_fwd(ptr(x), None, st, 2, R, 128, ptr(in_t), stream_ptr())
        torch.cuda.synchronize()
        return rc

    assert run([S, S | RM]) != 0
    assert torch.equal(y, torch.full_like(y, 5.0)) and torch.equal(in_t, torch.full_like(in_t, 9.0))
    assert run([S | RM, S]) == 0
    assert torch.equal(in_t[0], torch.full_like(in_t[0], 9.0))  # plane 0 not written
    h = torch.nn.functional.silu(x.double() @ w.double().t())
    torch.testing.assert_close(_t_layout(h.float()).double(), in_t[1].double(), rtol=1e-5, atol=1e-5)  # plane 1 is
    torch.testing.assert_close(y.double(), torch.nn.functional.silu(h @ w.double().t()), rtol=1e-5, atol=1e-5)
