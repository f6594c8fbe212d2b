"""Every entry point of the radial x angular basis (csrc/basis.hip: x2g_bessel_env, x2g_edge_basis,
x2g_edge_basis_freq_grad, x2g_spherical_basis) against the fp64 statement of the operation (tests/basis_ref.py),
element by element, at small shapes.

Bound (nothing taken from the code under test): every in-range element has to be finite and within
K = 8 unit bounds of the fp64 value, the unit bound being e32 times the term magnitudes and the argument's
rounding of the kernel's own formula (basis_ref's ``*_unit``); K was fixed against a numpy-float32 emulation
of that formula on the CPU (tests/test_basis_ref.py), which stays below 3 unit bounds.  The bound widens by itself
where the expanded Rayleigh form cancels (short distances, high l); no comparison is skipped.  Every output is
prefilled with NaN and carries one guard row that has to stay untouched.  Calls go through the raw ABI
(x2gnn._lib.call), so that NULL outputs, num_spherical < 7 and a runtime num_radial are reachable.

Distances: the golden molecules', 2001 values on [1.0, 4.9999] (``main``), the short-bond sweep of 257 values on
[0.5, 1.0) (``short``) and d = 5 (1 - 2^-20) (``edge``).  Triplet geometries: the golden molecules, ``angles``
(exactly collinear at 0 and pi, pi / 2, within 1e-3 rad of collinear) and ``star`` (a centre with 40 neighbours).

``python tests/test_gpu_basis_fp64.py --write profiles/basis_fp64_err.json`` runs every case once and writes,
per (entry point, output, shape, l), the number of comparisons and the worst error / bound with the case it is
worst in, the short-bond sweep's absolute errors, the constant K with the emulation's ratios, and the cap
shares; ``--all-rows`` writes one row per comparison instead.
"""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":  # (run as a script: the paths conftest.py sets up for pytest)
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "x2-gnn_amd"), os.path.join(_root, "tests")]

import basis_ref as br

pytestmark = pytest.mark.gpu

RECORD = []  # one dict per (comparison, l) made (the --write entry dumps it)
ACCUM_WGRAD = 1  # X2G_ACCUM_WGRAD
CUTOFF = br.CUTOFF
F = np.float32


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _nan(cuda, *shape):
    return torch.full(shape, float("nan"), device=cuda, dtype=torch.float32)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


_NAN_BITS = int(_bits(torch.full((1,), float("nan"), dtype=torch.float32))[0])


def _untouched(t):
    return bool((_bits(t) == _NAN_BITS).all())


class _Checker:
    """Compares the outputs of one case with the reference; collects every figure before failing."""

    def __init__(self, entry, shape, case):
        self.key = dict(entry=entry, shape=shape, case=case)
        self.bad = []

    def check(self, output, buf, rows, ref, unit, nrad=None, entry=None, d=None):
        """``buf``: the device buffer of rows + 1 rows, the last one the guard; ``ref`` / ``unit`` [rows, ...]
        float64; ``nrad``: the columns are l-major blocks of nrad (figures per l), None: one figure."""
        rec0 = dict(self.key, output=output, rows=int(rows))
        if entry:
            rec0["entry"] = entry
        ref = np.asarray(ref, np.float64).reshape(rows, -1)
        unit = np.asarray(unit, np.float64).reshape(rows, -1)
        assert buf.shape[0] == rows + 1
        if not _untouched(buf[rows:]):
            self.bad.append((rec0, "guard row written"))
        got = buf[:rows].detach().cpu().double().numpy().reshape(rows, -1)
        assert got.shape == ref.shape, (got.shape, ref.shape)
        if not np.isfinite(got).all():
            self.bad.append((rec0, f"{int((~np.isfinite(got)).sum())} non-finite elements"))
            return
        err = np.abs(got - ref)
        assert (unit > 0).all()
        ratio = err / (br.K * unit)
        width = nrad or ref.shape[1]
        for l in range(ref.shape[1] // width):
            blk = slice(l * width, (l + 1) * width)
            w = np.unravel_index(np.argmax(ratio[:, blk]), ratio[:, blk].shape)
            rec = dict(rec0, l=l if nrad else None, ratio=float(ratio[:, blk].max()), abs_err=float(err[:, blk].max()),
                       abs_err_at_worst=float(err[:, blk][w]), bound_at_worst=float(br.K * unit[:, blk][w]),
                       scale=float(np.abs(ref[:, blk]).max()))
            if d is not None:  # the error curve over the distances (the short-bond sweep)
                rec["curve"] = [[float(d[i]), float(err[i, blk].max()), float(np.abs(ref[i, blk]).max())]
                                for i in range(0, rows, 16)]
            RECORD.append(rec)
            if not rec["ratio"] <= 1.0:
                self.bad.append((rec, "error above bound"))

    def same(self, what, a, b):
        if not torch.equal(_bits(a), _bits(b)):
            self.bad.append((dict(self.key, output=what), "not bitwise equal"))

    def done(self):
        brief = lambda rec: {k: v for k, v in rec.items() if k != "curve"}  # noqa: E731
        assert not self.bad, "\n".join(f"{why}: {brief(rec)}" for rec, why in self.bad)


# ------------------------------------------------------------------------------ references (computed once, shared)
@functools.lru_cache(maxsize=None)
def _grid(name, E=None):
    if name == "main":
        return br.main_grid(E or br.MAIN_E)
    return br.radial_grids()[name]


@functools.lru_cache(maxsize=None)
def _edges(name, E=None):
    """(pos, src, dst, fp64 dist) whose distances follow the grid (the golden molecules' own edges for ``golden``)."""
    if name == "golden":
        g = br.geometry("golden")
        pos, src, dst = g.pos, g.ei[0].astype(np.int32), g.ei[1].astype(np.int32)
    else:
        pos, src, dst = br.edge_star(_grid(name, E))
    return pos, src, dst, br.dist(pos, src, dst)


@functools.lru_cache(maxsize=64)
def _radial_ref(name, E, nsph, nrad, from_pos):
    d = _edges(name, E)[3] if from_pos else _grid(name, E)
    return br.bessel_env(d, nsph, nrad), br.radial_unit(d, nsph, nrad)


# ------------------------------------------------------------------------------ a. Bessel terms
def _bessel_env(cuda, d, nsph, nrad):
    from x2gnn._lib import call, ptr, stream_ptr

    E = d.shape[0]
    out, dd = _nan(cuda, E + 1, nsph * nrad), _dev(d, cuda)  # (inputs stay referenced until the call is made)
    call("x2g_bessel_env", ptr(dd), E, CUTOFF, nsph, nrad, ptr(out), stream_ptr())
    return out


def _edge_basis(cuda, pos, src, dst, freq, nsph, nrad, env=True, rbf=True, bes=True):
    """x2g_edge_basis with the chosen outputs (the others NULL); every buffer has a guard row."""
    from x2gnn._lib import call, ptr, stream_ptr

    E, R = src.shape[0], 0 if freq is None else freq.shape[0]
    o = dict(dist=_nan(cuda, E + 1), env=_nan(cuda, E + 1) if env else None,
             rbf=_nan(cuda, E + 1, max(R, 1)) if rbf else None, bes=_nan(cuda, E + 1, nsph * nrad) if bes else None)
    ins = [_dev(a, cuda) for a in (pos, src, dst)] + [_dev(freq, cuda) if R else None]
    assert ins[1].dtype == ins[2].dtype == torch.int32 and ins[0].shape == (int(max(src.max(), dst.max())) + 1, 3)
    call("x2g_edge_basis", ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), E, CUTOFF, ptr(ins[3]), R, nsph, nrad, ptr(o["dist"]),
         ptr(o["env"]), ptr(o["rbf"]), ptr(o["bes"]), stream_ptr())
    return o


def _radial_case(cuda, name, E, nsph, nrad):
    """x2g_bessel_env on the grid and x2g_edge_basis's Bessel output on positions with those distances."""
    d = _grid(name, E)
    E = d.shape[0]
    shape = f"{nsph}x{nrad}"
    ck = _Checker("x2g_bessel_env", shape, name)
    ref, unit = _radial_ref(name, E, nsph, nrad, False)
    ck.check("bessel_env", _bessel_env(cuda, d, nsph, nrad), E, ref, unit, nrad, d=d if name == "short" else None)
    pos, src, dst, d64 = _edges(name, E)
    ref, unit = _radial_ref(name, E, nsph, nrad, True)
    o = _edge_basis(cuda, pos, src, dst, br.perturbed_freq(6), nsph, nrad)
    ck.check("bessel_env", o["bes"], E, ref, unit, nrad, entry="x2g_edge_basis", d=d64 if name == "short" else None)
    ck.done()


@pytest.mark.parametrize("E", br.EDGE_COUNTS)
@pytest.mark.parametrize("nsph,nrad", br.SHAPES)
def test_bessel_env_shapes(cuda, nsph, nrad, E):
    """env(d) N_ln j_l(z_ln d / 5) from x2g_bessel_env and from x2g_edge_basis at every (num_spherical,
    num_radial) of basis_ref.SHAPES (num_spherical < 7 included) and E around the 64-edge block, E distances
    spread over [1.0, 4.9999]."""
    _radial_case(cuda, "main", E, nsph, nrad)


@pytest.mark.parametrize("name", ["golden", "short", "edge"])
@pytest.mark.parametrize("nsph,nrad", br.SHAPES)
def test_bessel_env_grids(cuda, nsph, nrad, name):
    """The same on the golden molecules' distances, the short-bond sweep [0.5, 1.0) (where the expanded form
    cancels and the bound widens with it: the measured error goes into the profile) and d = 5 (1 - 2^-20)."""
    _radial_case(cuda, name, None, nsph, nrad)


# ------------------------------------------------------------------------------ b. dist, env, rbf; NULL outputs
@pytest.mark.parametrize("name", ["golden", "main", "short", "edge"])
@pytest.mark.parametrize("R", [0, 1, 6, 16])
def test_edge_basis_outputs(cuda, R, name):
    """x2g_edge_basis: dist, env and rbf = sin(freq d / 5) env with R perturbed frequencies (R = 0: the rbf
    buffer stays untouched) next to the 7 x 6 Bessel terms; then env NULL, rbf_env NULL and bessel_env NULL in
    turn: each remaining output bitwise equal to the all-outputs call."""
    pos, src, dst, d64 = _edges(name)
    E = src.shape[0]
    freq = br.perturbed_freq(R) if R else None
    ck = _Checker("x2g_edge_basis", f"7x6 R={R}", name)
    full = _edge_basis(cuda, pos, src, dst, freq, 7, 6)
    ck.check("dist", full["dist"], E, d64, br.dist_unit(d64))
    ck.check("env", full["env"], E, br.envelope(d64), br.env_unit(d64))
    if R:
        ck.check("rbf", full["rbf"][:, :R], E, br.rbf(d64, freq), br.rbf_unit(d64, freq))
    else:
        assert _untouched(full["rbf"])
    ck.check("bessel_env", full["bes"], E, *_radial_ref(name, None, 7, 6, True), 6)
    for drop in ("env", "rbf", "bes"):
        o = _edge_basis(cuda, pos, src, dst, freq, 7, 6, **{drop: False})
        for k, t in o.items():
            if t is not None:
                ck.same(f"{k} with {drop} NULL", t, full[k])
        if drop == "bes" and R:  # (the single-row launch) against the reference as well
            ent = "x2g_edge_basis[bessel NULL]"
            ck.check("rbf", o["rbf"][:, :R], E, br.rbf(d64, freq), br.rbf_unit(d64, freq), entry=ent)
            ck.check("dist", o["dist"], E, d64, br.dist_unit(d64), entry=ent)
    ck.done()


# ------------------------------------------------------------------------------ c. frequency gradient
@pytest.mark.parametrize("R", [6, 16])
@pytest.mark.parametrize("E", br.FREQ_GRAD_E)
def test_freq_grad(cuda, E, R):
    """x2g_edge_basis_freq_grad = sum_e g env cos(freq d / 5) d / 5 for E up to 33 025 (the grid-stride loop runs
    twice, the second pass ragged), written and accumulated (X2G_ACCUM_WGRAD) onto a non-zero dfreq, bitwise equal
    run to run."""
    from x2gnn import _lib
    from x2gnn._lib import call, ptr, stream_ptr

    g, d, env, freq, base = br.freq_grad_case(E, R)
    gd, dd, ed, fd = (_dev(a, cuda) for a in (g, d, env, freq))
    ws_b = int(_lib.load().x2g_edge_basis_freq_grad_workspace(E, R))
    assert ws_b == br.freq_grad_blocks(E) * R * 4
    ws = torch.empty(ws_b, dtype=torch.uint8, device=cuda)
    ref = br.freq_grad(g, d, env, freq)
    ck = _Checker("x2g_edge_basis_freq_grad", f"R={R}", f"E={E}")
    for flags, name, start in ((0, "dfreq", None), (ACCUM_WGRAD, "dfreq[accum]", base)):
        runs = []
        for _ in range(2):
            out = _nan(cuda, 2, R)  # row 0: dfreq, row 1: the guard
            if start is not None:
                out[0] = _dev(start, cuda)
            call("x2g_edge_basis_freq_grad", ptr(gd), ptr(dd), ptr(ed), ptr(fd), E, R, CUTOFF, ptr(out), flags, ptr(ws),
                 ws_b, stream_ptr())
            runs.append(out)
        ck.same(name + " run to run", runs[0], runs[1])
        want = ref if start is None else ref + start.astype(np.float64)
        ck.check(name, runs[0], 1, want[None, :], br.freq_grad_unit(g, d, env, freq, start)[None, :])
    ck.done()


# ------------------------------------------------------------------------------ d. spherical basis
@functools.lru_cache(maxsize=None)
def _angular_ref(gname, path):
    """(theta32 or None, trip_src, cos, its unit, Y [T, 7], its unit) of a geometry: from the positions, or from
    the float32 angle with the source rows shuffled."""
    g = br.geometry(gname)
    if path == "pos":
        c, cu = br.cos_theta(g.pos, g.ai, g.aj, g.ak), br.cos_unit_pos(g.pos, g.ai, g.aj, g.ak)
        th32, src = None, g.trip_src
    else:
        th32 = br.theta(g.pos, g.ai, g.aj, g.ak).astype(F)
        c, cu = np.cos(th32.astype(np.float64)), br.cos_unit_theta(th32)
        src = np.random.default_rng(g.T).integers(0, g.E, g.T).astype(np.int32)
    return th32, src, c, cu, br.sph_y(c), br.sph_y_unit(c, cu)


@functools.lru_cache(maxsize=None)
def _geometry_radial(gname, nsph, nrad):
    d = br.geometry(gname).dist
    return br.bessel_env(d, nsph, nrad), br.radial_unit(d, nsph, nrad)


def _spherical(cuda, g, T, th32, src, radial, nsph, nrad, with_sbf=True):
    from x2gnn._lib import call, ptr, stream_ptr

    sbf = _nan(cuda, T + 1, nsph * nrad) if with_sbf else None
    cos_t, y = _nan(cuda, T + 1), _nan(cuda, T + 1, 8)
    if th32 is None:
        geo = [_dev(a, cuda) for a in (g.pos, g.ai[:T], g.aj[:T], g.ak[:T])] + [None]
        assert max(int(a[:T].max()) for a in (g.ai, g.aj, g.ak)) < g.pos.shape[0]
    else:
        geo = [None, None, None, None, _dev(th32[:T], cuda)]
    sd = _dev(src[:T], cuda)
    assert sd.dtype == torch.int32 and 0 <= int(src[:T].min()) and int(src[:T].max()) < radial.shape[0]
    assert radial.shape[1] == nsph * nrad and radial.is_contiguous()
    call("x2g_spherical_basis", *[ptr(t) for t in geo], ptr(sd), ptr(radial), T, nsph, nrad, ptr(sbf), ptr(cos_t),
         ptr(y), stream_ptr())
    return sbf, cos_t, y


@pytest.mark.parametrize("nrad", br.SBF_NRAD)
@pytest.mark.parametrize("nsph", br.SBF_NSPH)
def test_spherical_basis(cuda, nsph, nrad):
    """x2g_spherical_basis from positions and from given angles (trip_src shuffled there), num_radial 6 and 16
    (the templates) and 1, 5, 8 (the runtime instance), num_spherical 7, 3, 1, on the golden molecules, the
    collinear / right-angle / near-collinear triplets and the 40-neighbour star (whole, and its first 1, 255, 256,
    257 triplets): sbf against (fp64 Bessel terms of the distances)[trip_src] * Y_l0 with the radial rows taken from
    x2g_bessel_env (checked above), cos_theta, sph_y [T, 8] with column 7 exactly 1; and with sbf NULL (the
    factors alone) the same cos_theta and sph_y bit for bit."""
    shape = f"{nsph}x{nrad}"
    for gname in ("golden", "angles", "star"):
        g = br.geometry(gname)
        radial = _bessel_env(cuda, g.dist, nsph, nrad)[:g.E]
        rad, ru = _geometry_radial(gname, nsph, nrad)
        for path in ("pos", "theta"):
            th32, src, c, cu, yy, yu = _angular_ref(gname, path)
            for T in (g.T,) + (br.HEADS if gname == "star" else ()):
                ck = _Checker(f"x2g_spherical_basis[{path}]", shape, gname if T == g.T else f"{gname}[:{T}]")
                sbf, cos_t, y = _spherical(cuda, g, T, th32, src, radial, nsph, nrad)
                ck.check("cos_theta", cos_t, T, c[:T], cu[:T])
                ck.check("sph_y", y[:, :7], T, yy[:T], yu[:T], 1)
                if not bool((y[:T, 7] == 1.0).all()):
                    ck.bad.append((dict(ck.key, output="sph_y[:, 7]"), "not exactly 1"))
                ref = br.sbf(rad, src[:T], yy[:T, :nsph], nrad)
                unit = br.sbf_unit(rad, ru, src[:T], yy[:T, :nsph], yu[:T, :nsph], nrad)
                ck.check("sbf", sbf, T, ref, unit, nrad)
                none, cos2, y2 = _spherical(cuda, g, T, th32, src, radial, nsph, nrad, with_sbf=False)
                assert none is None
                ck.same("cos_theta with sbf NULL", cos2, cos_t)
                ck.same("sph_y with sbf NULL", y2, y)
                ck.done()


# ------------------------------------------------------------------------------ the profile
class _StopOnDeviceError:
    """(script mode) A failed bound is a figure to record and the run goes on; a HIP error ends it."""

    @staticmethod
    def pytest_exception_interact(node, call, report):
        if "HIP error" in str(call.excinfo.value):
            node.session.shouldstop = "HIP error: nothing more is launched"


def _write(path, all_rows=False):
    """Run every case of this module once and write the figures (module docstring)."""
    rc = pytest.main([os.path.abspath(__file__), "-m", "gpu", "-q", "-p", "no:cacheprovider"],
                     plugins=[_StopOnDeviceError()])
    rec = sys.modules["test_gpu_basis_fp64"].RECORD  # (the module as pytest imported it)
    f3 = lambda v: float(f"{v:.3e}")  # noqa: E731
    emu = br.emulation_report()
    head = dict(pytest_exit_code=int(rc), comparisons=len(rec),
                errors="|kernel - ref64| per element; ratio = max over the elements of error / (K * unit bound)",
                K=br.K, e32=br.E32,
                constants={k: dict(emulation_worst_over_unit=f3(v), fixed_against=br.EMULATION_RATIO[k],
                                   K_over_emulation=f3(br.K / v)) for k, v in sorted(emu.items())},
                cap=dict(level=br.CAP_LEVEL, allowed_share=br.CAP_SHARE,
                         share_of_bounds_above_level={k: {n: f3(s) if n == "share" else [f3(x) for x in s]
                                                          for n, s in v.items()} for k, v in br.cap_report().items()}))
    worst = {}
    for r in rec:
        worst[r["entry"]] = max(worst.get(r["entry"], 0.0), r["ratio"])
    head["worst_error_over_bound"] = {k: f3(v) for k, v in sorted(worst.items())}
    sweep_cols = ["entry", "shape", "l", "worst err/bound", "max abs err", "max |value|",
                  "curve [d, max_n abs err, max_n |value|]"]
    sweep = [[r["entry"], r["shape"], r["l"], f3(r["ratio"]), f3(r["abs_err"]), f3(r["scale"]),
              [[f3(v) for v in p] for p in r["curve"]]] for r in rec if "curve" in r and r["shape"] in ("7x6", "7x16")]
    if all_rows:
        cols = ["entry", "output", "shape", "case", "rows", "l", "ratio", "abs_err", "scale"]
        rows = [[f3(r[c]) if isinstance(r[c], float) else r[c] for c in cols] for r in rec]
    else:
        cols = ["entry", "output", "shape", "l", "comparisons", "worst err/bound", "worst in: case", "rows",
                "abs err there", "bound there", "max |value|"]
        agg = {}
        for r in rec:
            key = (r["entry"], r["output"], r["shape"], -1 if r["l"] is None else r["l"])
            a = agg.setdefault(key, dict(n=0, worst=None))
            a["n"] += 1
            if a["worst"] is None or r["ratio"] > a["worst"]["ratio"]:
                a["worst"] = r
        rows = []
        for (entry, output, shape, l), a in sorted(agg.items()):
            r = a["worst"]
            rows.append([entry, output, shape, None if l < 0 else l, a["n"], f3(r["ratio"]), r["case"], r["rows"],
                         f3(r["abs_err_at_worst"]), f3(r["bound_at_worst"]), f3(r["scale"])])
    with open(path, "w") as f:  # one row per line
        lines = lambda rr: ",\n".join(json.dumps(row) for row in rr)  # noqa: E731
        f.write("{\n" + "".join(f" {json.dumps(k)}: {json.dumps(v)},\n" for k, v in head.items()))
        f.write(f' "short_bond_sweep_columns": {json.dumps(sweep_cols)},\n "short_bond_sweep": [\n{lines(sweep)}\n],\n')
        f.write(f' "columns": {json.dumps(cols)},\n "rows": [\n{lines(rows)}\n]}}\n')
    return int(rc)


if __name__ == "__main__":
    if len(sys.argv) not in (3, 4) or sys.argv[1] != "--write" or sys.argv[3:] not in ([], ["--all-rows"]):
        sys.exit("usage: python tests/test_gpu_basis_fp64.py --write profiles/basis_fp64_err.json [--all-rows]")
    sys.exit(_write(sys.argv[2], all_rows=len(sys.argv) == 4))
