"""The fp64 statement of the atom-context chain (tests/atom_context_ref.py) against torch-float64 autograd of the
reference's lines (model.py:138-141 with the conv's lin_edge, gathered per triplet as the reference does), the
float32 emulation that fixes K, wrong variants that have to leave the bound, and the entry points' host-side
argument checks.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import atom_context_ref as ar

F = np.float32


def _torch_statement(i, dx_seed=3):
    """scatter_add over edge_index_0, edgenn, lin_edge in float64 with autograd; the gradient arrives per atom."""
    t = lambda a: None if a is None else torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    x, w0, b0, w1, b1, we = (t(i[k]) for k in ("x", "w0", "b0", "w1", "b1", "we"))
    N = len(i["rowptr"]) - 1
    src = torch.from_numpy(ar.edge_atom(i["rowptr"], i["E"]))
    atoms_rep = torch.zeros(N, ar.D, dtype=torch.float64).index_add(0, src, x)
    z0 = atoms_rep @ w0.T + (b0 if b0 is not None else 0)
    g = torch.nn.functional.silu(z0) @ w1.T + (b1 if b1 is not None else 0)
    tab = g @ we.T
    tab.backward(torch.tensor(np.asarray(i["d_tab"], np.float64)))
    return atoms_rep.detach().numpy(), z0.detach().numpy(), tab.detach().numpy(), x.grad.numpy()


def _close(got, want):
    scale = max(float(np.abs(want).max()), 1e-300)
    assert np.abs(got - want).max() <= 1e-12 * scale


@pytest.mark.parametrize("N,empty,bias", [(1, False, True), (17, False, True), (17, False, False), (33, False, True),
                                          (5, True, True)])
def test_statement_equals_torch_float64(N, empty, bias):
    i = ar.context_inputs(N, empty, bias)
    A, z0, tab, dx = _torch_statement(i)
    fwd = ar.context_fwd(i["x"], i["rowptr"], i["w0"], i["b0"], i["w1"], i["b1"], i["we"])
    bwd = ar.context_bwd(i["d_tab"], z0, i["rowptr"], i["E"], i["w0"], i["w1"], i["we"])
    _close(fwd["A"][0], A)
    _close(fwd["z0"][0], z0)
    _close(fwd["tab"][0], tab)
    if i["E"]:
        _close(bwd["dx"][0], dx)
    for v, u in list(fwd.values()) + list(bwd.values()):
        assert (u >= np.abs(v) * (1 - 1e-12)).all()  # a unit is never below its value's magnitude


def test_degrees():
    for N in ar.ATOMS:
        deg = ar.degrees(N)
        if N == 1:
            assert deg.tolist() == [3]
            continue
        assert deg[0] == 0 and deg[-1] == 0 and deg[N // 2] == 0 and deg.max() == ar.HUB_DEGREE
        assert (np.delete(deg, N // 2 + 1) <= 9).all()
    assert ar.ATOMS == (1, 15, 16, 17, 2 * ar.TILE - 1, 2 * ar.TILE + 1)
    i = ar.context_inputs(17, empty=True)
    assert i["E"] == 0 and i["x"].shape == (0, ar.D)
    fwd = ar.context_fwd(i["x"], i["rowptr"], i["w0"], i["b0"], i["w1"], i["b1"], i["we"])
    assert (fwd["A"][0] == 0).all() and (fwd["A"][1] == 0).all()  # unit 0: the kernel has to write exact zeros
    assert np.ptp(fwd["tab"][0], axis=0).max() == 0  # every row the bias-only row


def test_emulation_ratios_and_k():
    rep = ar.emulation_report()
    assert set(rep) == set(ar.K) == set(ar.EMULATION_RATIO) == set(ar.FAMILY.values())
    for fam, (r, output, case) in rep.items():
        print(f"{fam}: {r:.3f} ({output}, {case})")
        assert r <= ar.EMULATION_RATIO[fam], (fam, r, output, case)
        assert 4 * ar.EMULATION_RATIO[fam] <= ar.K[fam]
        assert ar.K[fam] == 2.0 ** round(np.log2(ar.K[fam])) and ar.K[fam] < 8 * ar.EMULATION_RATIO[fam] + 1


def _leaves(fam, got, ref_unit):
    return ar.ratio(got, *ref_unit) > ar.K[fam]


def test_wrong_variants_leave_the_bound():
    i = ar.context_inputs(33)
    wf = (i["w0"], i["b0"], i["w1"], i["b1"], i["we"])
    fwd = ar.context_fwd(i["x"], i["rowptr"], *wf)
    z0 = fwd["z0"][0].astype(F)
    bwd = ar.context_bwd(i["d_tab"], z0, i["rowptr"], i["E"], i["w0"], i["w1"], i["we"])
    assert not _leaves("tab", fwd["tab"][0], fwd["tab"])
    # a bias on lin_edge; edgenn's second bias dropped; the SiLU left out
    assert _leaves("tab", fwd["tab"][0] + np.asarray(i["b1"], np.float64), fwd["tab"])
    assert _leaves("tab", ar.context_fwd(i["x"], i["rowptr"], i["w0"], i["b0"], i["w1"], None, i["we"])["tab"][0],
                   fwd["tab"])
    lin = (fwd["z0"][0] @ np.asarray(i["w1"], np.float64).T + i["b1"]) @ np.asarray(i["we"], np.float64).T
    assert _leaves("tab", lin, fwd["tab"])
    # the pool one row short (the last out-edge of every atom left out)
    short = i["rowptr"].copy()
    A_short = np.stack([np.asarray(i["x"][short[a]:max(short[a + 1] - 1, short[a])], np.float64).sum(0)
                        for a in range(33)])
    assert _leaves("saved", A_short, fwd["A"])
    # the weights untransposed in the backward; SiLU' taken as the sigmoid alone
    wrong = ar.context_bwd(i["d_tab"], z0, i["rowptr"], i["E"], i["w0"].T, i["w1"].T, i["we"].T)
    assert _leaves("dgz", wrong["d_g"][0], bwd["d_g"]) and _leaves("dx", wrong["dx"][0], bwd["dx"])
    s = 1 / (1 + np.exp(-z0.astype(np.float64)))
    dh = bwd["d_g"][0] @ np.asarray(i["w1"], np.float64)
    assert _leaves("dgz", dh * s, bwd["d_z0"])
    # the broadcast shifted by one line node; += where = was asked
    assert _leaves("dx", np.roll(bwd["dx"][0], 1, axis=0), bwd["dx"])
    assert _leaves("dx", bwd["dx"][0] + i["dx_old"], bwd["dx"])
    # a 1e-5 relative perturbation of every output of the forward and of d_g / d_z0; dx and tab, three products
    # deep, carry units of several hundred times a typical value: 1e-3 there
    for fam, (v, u) in (("saved", fwd["A"]), ("saved", fwd["z0"]), ("saved", fwd["h"]), ("dgz", bwd["d_g"])):
        assert _leaves(fam, v * (1 + 1e-5), (v, u)), fam
    for fam, (v, u), eps in (("saved", fwd["g"], 1e-4), ("dgz", bwd["d_z0"], 1e-4), ("tab", fwd["tab"], 1e-3),
                             ("dx", bwd["dx"], 1e-3)):
        assert _leaves(fam, v * (1 + eps), (v, u)), fam


# ------------------------------------------------------------------------------------------------ the entry points
OK, EINVAL, EUNSUPPORTED = 0, 1001, 1002


def _fwd_args(**kw):
    p = ctypes.c_void_p(4096)  # 16-byte aligned, never dereferenced: every check fails (or N == 0 returns) first
    a = dict(x=p, rowptr=p, N=4, E=9, dim=128, w0=p, b0=p, w1=p, b1=p, we=p, tab=p, a_out=p, z0=p, h=p, g=p)
    a.update(kw)
    return tuple(a.values()) + (None,)


def _bwd_args(**kw):
    p = ctypes.c_void_p(4096)
    a = dict(d_tab=p, z0=p, rowptr=p, N=4, E=9, dim=128, w0=p, w1=p, we=p, d_g=p, d_z0=p, dx=p, accumulate=0)
    a.update(kw)
    return tuple(a.values()) + (None,)


ODD = ctypes.c_void_p(4096 + 4)
BIG = (1 << 31) // 512


@pytest.mark.parametrize("kw,want", [
    (dict(N=0), OK), (dict(N=0, E=0, x=None), OK),
    (dict(N=-1), EINVAL), (dict(E=-1), EINVAL), (dict(x=None), EINVAL), (dict(rowptr=None), EINVAL),
    (dict(w0=None), EINVAL), (dict(w1=None), EINVAL), (dict(we=None), EINVAL), (dict(tab=None), EINVAL),
    (dict(x=ODD), EINVAL), (dict(we=ODD), EINVAL), (dict(tab=ODD), EINVAL), (dict(z0=ODD), EINVAL),
    (dict(rowptr=ctypes.c_void_p(4098)), EINVAL),
    (dict(dim=64), EUNSUPPORTED), (dict(dim=256), EUNSUPPORTED), (dict(N=BIG), EUNSUPPORTED),
    (dict(E=BIG), EUNSUPPORTED),
])
def test_forward_argument_validation_without_gpu(kw, want):
    from x2gnn import _lib

    assert _lib.load().x2g_atom_context_fwd(*_fwd_args(**kw)) == want


@pytest.mark.parametrize("kw,want", [
    (dict(N=0), OK),
    (dict(N=-1), EINVAL), (dict(E=-1), EINVAL), (dict(d_tab=None), EINVAL), (dict(z0=None), EINVAL),
    (dict(rowptr=None), EINVAL), (dict(w0=None), EINVAL), (dict(d_g=None), EINVAL), (dict(d_z0=None), EINVAL),
    (dict(d_tab=ODD), EINVAL), (dict(dx=ODD), EINVAL), (dict(w1=ODD), EINVAL),
    (dict(dim=64), EUNSUPPORTED), (dict(N=BIG), EUNSUPPORTED), (dict(E=BIG), EUNSUPPORTED),
])
def test_backward_argument_validation_without_gpu(kw, want):
    from x2gnn import _lib

    assert _lib.load().x2g_atom_context_bwd(*_bwd_args(**kw)) == want


def test_binding_tables():
    from x2gnn import _lib

    names = {"x2g_atom_context_fwd", "x2g_atom_context_bwd"}
    assert set(_lib.ATOMCTX_SIGNATURES) == names == set(_lib.ATOMCTX_RESTYPES)
    for table in (_lib.SIGNATURES, _lib.STAGED_SIGNATURES, _lib.MULTI_SIGNATURES, _lib.CONV_SIGNATURES):
        assert not names & set(table)
    assert len(_lib.ATOMCTX_SIGNATURES["x2g_atom_context_fwd"]) == 16
    assert len(_lib.ATOMCTX_SIGNATURES["x2g_atom_context_bwd"]) == 14
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in names)
