"""The atom-context kernels (csrc/atom_context.hip, include/x2g_atomctx.h) through the raw ABI against their fp64
statement (tests/atom_context_ref.py), element by element, at the smallest shapes at which the tiling changes: 1, 15,
16, 17, 31 and 33 atoms (a tile of 16 atoms per workgroup, one workgroup per tile: the grid is never capped, so no
workgroup takes a second tile), out-degrees from 0..9 with the first, the last and an interior atom without
out-edges and one atom of degree 40, no line node at all, and no biases.

Bound (nothing taken from the code under test): every element has to be finite and within K * 2^-24 * unit of the
fp64 value (atom_context_ref: the units and how K was fixed against a float32 emulation on the CPU); where the unit
is 0 (the pooled row of an atom without out-edges) the kernel has to return exactly 0.  Every output buffer is
prefilled with NaN and carries one guard row that has to stay untouched bit for bit; inputs are seeded on the CPU.
The backward gets the fp64 z0 rounded to float32 (the statement's, not the kernel's), except in
``test_forward_backward_chain``.
"""
import ctypes

import numpy as np
import pytest
import torch

import atom_context_ref as ar

pytestmark = pytest.mark.gpu

OK, EINVAL, EUNSUPPORTED = 0, 1001, 1002
F = np.float32
D = ar.D


def _dev(a, cuda):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _nan(cuda, *shape):
    return torch.full(shape, float("nan"), device=cuda, dtype=torch.float32)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


_NAN_BITS = int(_bits(torch.full((1,), float("nan"), dtype=torch.float32))[0])


def _untouched(t):
    return bool((_bits(t) == _NAN_BITS).all())


def _lib():
    from x2gnn import _lib as lib

    return lib


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _Checker:
    """Compares the outputs of one case with the reference; collects every figure before failing."""

    def __init__(self, case):
        self.case, self.bad, self.worst = case, [], {}

    def check(self, output, buf, rows, ref_unit):
        """``buf``: rows + 1 leading entries, the last one the guard."""
        fam = ar.FAMILY[output.split()[0]]
        if not _untouched(buf[rows:]):
            self.bad.append(f"{output}: guard written")
        if rows == 0:
            return
        ref, unit = (np.asarray(a, np.float64).reshape(rows, -1) for a in ref_unit)
        got = buf[:rows].detach().cpu().double().numpy().reshape(rows, -1)
        r = ar.ratio(got, ref, unit) / ar.K[fam]
        self.worst[output] = max(r, self.worst.get(output, 0.0))
        if not r <= 1.0:
            self.bad.append(f"{output}: error / bound = {r:.3g} (family {fam})")

    def zero(self, output, t):
        if not bool((t == 0).all()):
            self.bad.append(f"{output}: not exactly zero")

    def same(self, output, a, b):
        if not torch.equal(_bits(a), _bits(b)):
            self.bad.append(f"{output}: not bitwise equal")

    def untouched(self, output, t):
        if not _untouched(t):
            self.bad.append(f"{output}: written")

    def status(self, output, rc, want=OK):
        if rc != want:
            self.bad.append(f"{output}: status {rc}, expected {want}")

    def done(self):
        print(self.case, {k: round(v, 4) for k, v in self.worst.items()})
        assert not self.bad, self.case + "\n" + "\n".join(self.bad)


def _weights(cuda, i):
    return {k: _dev(i[k], cuda) for k in ("w0", "b0", "w1", "b1", "we")}


def _fwd(cuda, i, w, keep=True, x=None):
    """(rc, tab, [A, z0, h, g]): every buffer N + 1 rows."""
    N = len(i["rowptr"]) - 1
    x = _dev(i["x"], cuda) if x is None else x
    tab = _nan(cuda, N + 1, D)
    kept = [_nan(cuda, N + 1, D) for _ in range(4)]
    rowptr = _dev(i["rowptr"], cuda)  # (held until the call returned: the launch is enqueued by then)
    rc = _lib().load().x2g_atom_context_fwd(
        _p(x) if i["E"] else None, _p(rowptr), N, i["E"], D, _p(w["w0"]), _p(w["b0"]), _p(w["w1"]),
        _p(w["b1"]), _p(w["we"]), _p(tab), *[_p(t) if keep else None for t in kept], _lib().stream_ptr())
    torch.cuda.synchronize()  # (the inputs live until the kernel has read them)
    return rc, tab, kept


def _bwd(cuda, i, w, z0, accumulate, want_dx=True):
    """(rc, d_g, d_z0, dx): dx E + 1 rows, holding dx_old when accumulating."""
    N, E = len(i["rowptr"]) - 1, i["E"]
    d_g, d_z0, dx = _nan(cuda, N + 1, D), _nan(cuda, N + 1, D), _nan(cuda, E + 1, D)
    if accumulate:
        dx[:E] = _dev(i["dx_old"], cuda)
    d_tab, z0, rowptr = _dev(i["d_tab"], cuda), _dev(z0, cuda), _dev(i["rowptr"], cuda)
    rc = _lib().load().x2g_atom_context_bwd(
        _p(d_tab), _p(z0), _p(rowptr), N, E, D, _p(w["w0"]), _p(w["w1"]), _p(w["we"]), _p(d_g), _p(d_z0),
        _p(dx) if want_dx else None, int(accumulate), _lib().stream_ptr())
    torch.cuda.synchronize()  # (the inputs live until the kernel has read them)
    return rc, d_g, d_z0, dx


@pytest.mark.parametrize("N,empty,bias", ar.cases())
def test_every_atom_count(cuda, N, empty, bias):
    """tab and the four saved operands; d_g, d_z0 and dx in both modes (written, and added onto old contents)."""
    i = ar.context_inputs(N, empty, bias)
    E = i["E"]
    w = _weights(cuda, i)
    ck = _Checker(f"N={N} E={E} bias={bias}")
    ref = ar.context_fwd(i["x"], i["rowptr"], i["w0"], i["b0"], i["w1"], i["b1"], i["we"])
    rc, tab, kept = _fwd(cuda, i, w)
    ck.status("fwd status", rc)
    ck.check("tab", tab, N, ref["tab"])
    for name, t in zip(("A", "z0", "h", "g"), kept):
        ck.check(name, t, N, ref[name])
    deg0 = np.diff(i["rowptr"]) == 0
    ck.zero("A of the atoms without out-edges", kept[0][:N][torch.from_numpy(deg0).to(cuda)])
    rc, tab2, kept2 = _fwd(cuda, i, w, keep=False)  # inference: nothing kept, the same table
    ck.status("fwd status (nothing kept)", rc)
    ck.same("tab (nothing kept)", tab2, tab)
    for t in kept2:
        ck.untouched("a saved operand that was not asked for", t)
    z0 = ref["z0"][0].astype(F)
    for accumulate in (0, 1):
        refb = ar.context_bwd(i["d_tab"], z0, i["rowptr"], E, i["w0"], i["w1"], i["we"],
                              i["dx_old"] if accumulate else None)
        rc, d_g, d_z0, dx = _bwd(cuda, i, w, z0, accumulate)
        ck.status("bwd status", rc)
        ck.check("d_g", d_g, N, refb["d_g"])
        ck.check("d_z0", d_z0, N, refb["d_z0"])
        ck.check("dx" + (" +=" if accumulate else " ="), dx, E, refb["dx"])
    rc, d_g2, d_z02, dx2 = _bwd(cuda, i, w, z0, 0, want_dx=False)  # dx not wanted
    ck.status("bwd status (no dx)", rc)
    ck.same("d_g (no dx)", d_g2, d_g)
    ck.same("d_z0 (no dx)", d_z02, d_z0)
    ck.untouched("dx that was not asked for", dx2)
    ck.done()


def test_forward_backward_chain(cuda):
    """The backward fed the forward's own float32 z0, twice from fresh buffers: the same bits both times, and within
    the bound of the statement evaluated at that z0."""
    i = ar.context_inputs(33)
    N, E = 33, i["E"]
    w = _weights(cuda, i)
    ck = _Checker("forward -> backward")
    outs = []
    for _ in range(2):
        rc, tab, kept = _fwd(cuda, i, w)
        ck.status("fwd", rc)
        z0 = kept[1][:N].cpu().numpy()
        rc, d_g, d_z0, dx = _bwd(cuda, i, w, z0, 0)
        ck.status("bwd", rc)
        outs.append((tab, *kept, d_g, d_z0, dx))
    for u, v in zip(*outs):
        ck.same("two runs", u, v)
    z0 = outs[0][2][:N].cpu().numpy()
    refb = ar.context_bwd(i["d_tab"], z0, i["rowptr"], E, i["w0"], i["w1"], i["we"])  # (at the kernel's own z0)
    ck.check("d_g", outs[0][5], N, refb["d_g"])
    ck.check("d_z0", outs[0][6], N, refb["d_z0"])
    ck.check("dx", outs[0][7], E, refb["dx"])
    ck.done()


def test_status_codes(cuda):
    """dim other than 128: X2G_EUNSUPPORTED; a NULL or misaligned pointer, a negative count: X2G_EINVAL; N == 0:
    X2G_OK; nothing is written in any of them."""
    lib, st = _lib().load(), _lib().stream_ptr()
    i = ar.context_inputs(17)
    N, E = 17, i["E"]
    w = _weights(cuda, i)
    x, rp, d_tab = _dev(i["x"], cuda), _dev(i["rowptr"], cuda), _dev(i["d_tab"], cuda)
    z0 = _dev(np.zeros((N, D), F), cuda)
    ck = _Checker("status codes")
    odd = lambda t: ctypes.c_void_p(t.data_ptr() + 4)  # noqa: E731
    for what, kw, want in (
            ("dim 64", dict(dim=64), EUNSUPPORTED), ("dim 256", dict(dim=256), EUNSUPPORTED),
            ("N = 2^22", dict(N=(1 << 31) // 512), EUNSUPPORTED), ("E = 2^22", dict(E=(1 << 31) // 512), EUNSUPPORTED),
            ("N < 0", dict(N=-1), EINVAL), ("E < 0", dict(E=-1), EINVAL), ("NULL x", dict(x=None), EINVAL),
            ("NULL rowptr", dict(rowptr=None), EINVAL), ("NULL we", dict(we=None), EINVAL),
            ("NULL tab", dict(tab=None), EINVAL), ("x + 4 bytes", dict(x=odd(x)), EINVAL),
            ("w0 + 4 bytes", dict(w0=odd(w["w0"])), EINVAL), ("N = 0", dict(N=0), OK)):
        tab, kept = _nan(cuda, N + 1, D), [_nan(cuda, N + 1, D) for _ in range(4)]
        a = dict(x=_p(x), rowptr=_p(rp), N=N, E=E, dim=D, w0=_p(w["w0"]), b0=_p(w["b0"]), w1=_p(w["w1"]),
                 b1=_p(w["b1"]), we=_p(w["we"]), tab=_p(tab))
        a.update(kw)
        ck.status("fwd " + what, lib.x2g_atom_context_fwd(*a.values(), *[_p(t) for t in kept], st), want)
        for t in (tab, *kept):
            ck.untouched(f"a forward output after {what}", t)
    for what, kw, want in (
            ("dim 64", dict(dim=64), EUNSUPPORTED), ("E = 2^22", dict(E=(1 << 31) // 512), EUNSUPPORTED),
            ("N < 0", dict(N=-1), EINVAL), ("NULL d_tab", dict(d_tab=None), EINVAL), ("NULL z0", dict(z0=None), EINVAL),
            ("NULL w1", dict(w1=None), EINVAL), ("d_tab + 4 bytes", dict(d_tab=odd(d_tab)), EINVAL),
            ("N = 0", dict(N=0), OK)):
        d_g, d_z0, dx = _nan(cuda, N + 1, D), _nan(cuda, N + 1, D), _nan(cuda, E + 1, D)
        a = dict(d_tab=_p(d_tab), z0=_p(z0), rowptr=_p(rp), N=N, E=E, dim=D, w0=_p(w["w0"]), w1=_p(w["w1"]),
                 we=_p(w["we"]))
        a.update(kw)
        ck.status("bwd " + what, lib.x2g_atom_context_bwd(*a.values(), _p(d_g), _p(d_z0), _p(dx), 0, st), want)
        for t in (d_g, d_z0, dx):
            ck.untouched(f"a backward output after {what}", t)
    ck.done()
