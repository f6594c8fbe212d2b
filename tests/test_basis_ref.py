"""The fp64 basis reference and its bounds (tests/basis_ref.py) made trustworthy on the CPU: equal to the
oracle's scipy evaluation and to the reference implementation's stored fp32 outputs, the numpy-float32 emulation
of the kernels' formulas inside every bound with the margin the constant K was fixed for, the bounds tight
enough on the main grid (the cap), and wide of the mark once a constant table is perturbed."""
import math

import numpy as np
import pytest
import torch

import basis_ref as br
from conftest import golden
from test_gpu_kernels import BASIS_TOL

from oracle import ref_cpu


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1.0))


@pytest.mark.parametrize("nsph,nrad", br.SHAPES)
def test_reference_equals_oracle(nsph, nrad):
    """basis_ref's values against oracle.ref_cpu's bessel_radial, envelope, sph_y0 (1e-12 of scale) and
    spherical_basis (which returns float32: to that rounding), on the golden geometry and the main grid."""
    g = br.geometry("golden")
    for d in (g.dist, br.main_grid(), br.short_grid()):
        assert _rel(br.bessel(d, nsph, nrad), ref_cpu.bessel_radial(d.astype(np.float64) / 5.0, nsph, nrad)) < 1e-12
        assert _rel(br.envelope(d), ref_cpu.envelope(d.astype(np.float64))) < 1e-12
    th = br.theta(g.pos, g.ai, g.aj, g.ak)
    c = br.cos_theta(g.pos, g.ai, g.aj, g.ak)
    assert np.abs(c - np.cos(th)).max() < 1e-12
    assert np.abs(br.sph_y(c, nsph) - ref_cpu.sph_y0(th, nsph)).max() < 1e-12
    ours = br.sbf(br.bessel_env(g.dist, nsph, nrad), g.trip_src, br.sph_y(np.cos(th), nsph), nrad)
    theirs = ref_cpu.spherical_basis(torch.from_numpy(g.dist).double(), torch.from_numpy(th),
                                     torch.from_numpy(g.trip_src).long(), nsph, nrad).numpy()
    assert np.all(np.abs(ours - theirs) <= 2.0 ** -24 * np.abs(ours) + 1e-30)


@pytest.mark.parametrize("fixture,nrad", [("basis.npz", 6), ("basis_7x16.npz", 16)])
def test_reference_reproduces_goldens(fixture, nrad):
    """The reference implementation's own float32 outputs (noisy at high l: BASIS_TOL) — this ties the two
    together, nothing more."""
    z = golden(fixture)
    g = br.geometry("golden")
    assert np.array_equal(g.trip_src, z["trip"][0])
    assert np.abs(g.dist - z["dist"]).max() <= 2e-6 * z["dist"].max()
    s = br.sbf(br.bessel_env(z["dist"], 7, nrad), z["trip"][0], br.sph_y(np.cos(z["theta"].astype(np.float64))), nrad)
    for l in range(7):
        blk = slice(nrad * l, nrad * (l + 1))
        tol = BASIS_TOL[l] + (2e-6 * np.abs(z["sbf"][:, blk]).max() if nrad == 16 else 0.0)
        assert np.abs(s[:, blk] - z["sbf"][:, blk]).max() < tol, l
    assert np.abs(br.theta(g.pos, g.ai, g.aj, g.ak) - z["theta"]).max() < 2e-6
    freq = math.pi * np.arange(1, nrad + 1, dtype=np.float32)
    np.testing.assert_allclose(br.rbf(z["dist"], freq), z["rbf"], rtol=1e-5, atol=5e-5)
    if "env" in z.files:
        np.testing.assert_allclose(br.envelope(z["dist"]), z["env"], rtol=2e-6, atol=2e-5)
        np.testing.assert_allclose(br.envelope(z["env_probe_d"][:4]), z["env_probe"][:4], rtol=2e-6, atol=2e-5)


def test_emulation_stays_inside_the_bounds():
    """The numpy-float32 emulation of the kernels' formulas on every grid and geometry the GPU test uses: per
    output its worst error in unit bounds is at most basis_ref.EMULATION_RATIO (the figure K was fixed against),
    and K is 2.6x to 6x that."""
    rep = br.emulation_report()
    print("worst |emulation - ref64| / unit bound:", {k: round(v, 3) for k, v in rep.items()})
    assert set(rep) == set(br.EMULATION_RATIO)
    for name, ratio in rep.items():
        assert ratio <= br.EMULATION_RATIO[name], (name, ratio)
        assert br.EMULATION_RATIO[name] <= 3.0 and br.K / br.EMULATION_RATIO[name] >= 2.6, name


def test_bounds_are_tight_on_the_main_grid():
    """The cap, from the reference alone: on the main grid (1.0 .. 4.9999 Angstrom) at most 2 % of the comparisons
    of any (entry point, output, shape) have a bound above 1e-3 of their column's largest |value|.  (All of those
    are at l >= 5 and short distances; the worst share per l is 7.4 % at l = 6 of the 7 x 1 shape, 1.2 % at
    7 x 6.)"""
    rep = br.cap_report()
    print("share of bounds above 1e-3 of the column scale:", {k: round(v["share"], 4) for k, v in rep.items()})
    for key, v in rep.items():
        assert v["share"] <= br.CAP_SHARE, (key, v)
    assert rep["x2g_bessel_env bessel_env 7x6"]["by_l"][6] <= 0.013
    assert max(rep["x2g_bessel_env bessel_env 7x6"]["by_l"][:6]) <= 0.001


PERTURBED = [("coef", (0, 2, 0), 1 + 1e-4, "bessel_env"), ("coef", (3, 2, 0), 1 + 1e-4, "bessel_env"),
             ("coef", (6, 2, 0), 1 + 1e-4, "bessel_env"), ("ycoef", (6, 2), 1 + 1e-4, "sph_y"),
             ("env6", None, 48.001 / 48.0, "env")]


@pytest.mark.parametrize("table,index,factor,output", PERTURBED)
def test_perturbed_constants_leave_the_bound(table, index, factor, output):
    """Self-check: the emulation with one constant off by 1e-4 (the envelope's 48 -> 48.001) is outside K unit
    bounds on the GPU test's grids, in the output that constant feeds (and in what is built on it)."""
    rep = br.emulation_report(br.Tables().perturbed(table, index, factor))
    print(f"{table}{index} x {factor}: worst error / bound", {k: round(v / br.K, 2) for k, v in rep.items()})
    assert rep[output] > br.K, (output, rep[output])
    if output != "sph_y":
        assert rep["bessel_env"] > br.K
    assert rep["sbf"] > br.K
    if table != "env6":  # the tables feed nothing else
        for name in ("dist", "env", "rbf", "cos_theta", "freq_grad"):
            assert rep[name] <= br.EMULATION_RATIO[name], name
