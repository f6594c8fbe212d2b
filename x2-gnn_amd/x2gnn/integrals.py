"""The first step of the reference's ``mapping``: ``geom_scf_6`` (scf.py:27-48), the overlap matrix S and the core
Hamiltonian H_core of a molecule from its geometry and a basis set, on the device (csrc/integrals.hip,
include/x2g_integrals.h).  The reference builds a pyscf RKS object for it but never runs an SCF: it takes
``get_ovlp()`` and ``get_hcore()``, the overlap, kinetic and nuclear-attraction integrals over contracted spherical
Gaussians.  With :mod:`x2gnn.graph` and :mod:`x2gnn.features` the whole input pipeline then runs on the GPU:
xyz -> bonds -> integrals -> features -> ``DeviceDataset``.  What the user brings is the basis set.

* :class:`Basis` holds a basis set as the flat tables the ABI takes, from pyscf's internal format
  (:meth:`Basis.from_pyscf`) or from NWChem text (:meth:`Basis.from_nwchem`), sorted and normalised as pyscf does.
  No basis-set library is shipped.
* :func:`one_electron_matrices` is the batched call: the matrices of M molecules, complete or only the atom-pair
  blocks of a pair list (the bonds), as an :class:`x2gnn.features.AOMatrices`.
* :func:`plan_one_electron` prepares that call without making it (a :class:`OneElectronLaunch`: its pair count,
  and ``run()`` to enqueue it, again if need be), for code that times or repeats the launch.
* :func:`geom_scf_6` has the reference's signature for one molecule, plus the basis.

The operation and its conventions are stated in include/x2g_integrals.h.  Everything is float64.  There is no CPU
implementation: without a GPU these calls raise.
"""
from __future__ import annotations

import ctypes
import math
import re

import numpy as np
import torch

from . import _lib
from .features import AO_PAD, AOMatrices

BOHR = 0.52917721092  # pyscf's (CODATA 2010): coordinates in angstrom are divided by it
MAX_L = 3
_L_OF = {"S": 0, "P": 1, "D": 2, "F": 3, "G": 4, "H": 5, "I": 6}
SYMBOLS = ("X H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Y "
           "Zr Nb Mo Tc Ru Rh Pd Ag Cd In Sn Sb Te I Xe").split()
_Z_OF = {s: z for z, s in enumerate(SYMBOLS) if z}


def _symbol(name) -> str:
    """'c', 'C1', ' C ' -> 'C'; ValueError for what is no element up to Xe."""
    s = re.sub(r"[^A-Za-z]", "", str(name)).capitalize()
    if s not in _Z_OF:
        raise ValueError(f"unknown element {name!r}")
    return s


def _radial_norm(alpha, l):
    """N with the integral of (N r^l exp(-alpha r^2))^2 r^2 over r equal to 1."""
    return math.sqrt(2.0 * (2.0 * alpha) ** (l + 1.5) / math.gamma(l + 1.5))


class Basis:
    """A basis set as flat tables (numpy, on the host; :meth:`device_tables` uploads them once per device).

    ``symbols``: the elements, in table order; per element its shells ``elem_shell[e]:elem_shell[e + 1]``, ordered by
    l and stably in input order within one l; per shell ``shell_l``, its primitives
    ``shell_prim[s]:shell_prim[s + 1]`` and ``shell_ao``, its first function counted from the atom's first; per
    primitive ``prim_exp`` and ``prim_coef``, the contraction coefficient times the primitive's radial normalisation,
    rescaled so that every contracted function has unit self-overlap.  ``elem_nao`` / ``elem_nshell``: functions and
    shells per element."""

    def __init__(self, shells_by_symbol: dict):
        """``shells_by_symbol``: {symbol: [(l, exponents, coefficients), ...]} with one coefficient per exponent.
        Use :meth:`from_pyscf` or :meth:`from_nwchem`."""
        self.symbols, elem_shell, shell_l, shell_prim, shell_ao, exps, coefs = [], [0], [], [0], [], [], []
        for name, shells in shells_by_symbol.items():
            sym = _symbol(name)
            if sym in self.symbols:
                raise ValueError(f"{sym}: given twice")
            if not shells:
                raise ValueError(f"{sym}: no shell")
            ao = 0
            for l, e, c in sorted(shells, key=lambda s: s[0]):  # (stable)
                e, c = np.asarray(e, np.float64).reshape(-1), np.asarray(c, np.float64).reshape(-1)
                if l > MAX_L or l < 0:
                    raise ValueError(f"{sym}: a shell with l = {l}; l <= {MAX_L} is supported")
                if e.size == 0 or e.shape != c.shape:
                    raise ValueError(f"{sym}: a shell with {e.size} exponents and {c.size} coefficients")
                if not bool((e > 0).all()) or not bool(np.isfinite(e).all()):
                    raise ValueError(f"{sym}: exponent {float(e.min())!r} is not positive")
                keep = c != 0
                if not keep.any():
                    raise ValueError(f"{sym}: a shell whose coefficients are all zero")
                e, c = e[keep], c[keep]
                d = c * np.array([_radial_norm(x, l) for x in e])
                # self-overlap of the contracted radial function
                pair = math.gamma(l + 1.5) / (2.0 * (e[:, None] + e[None, :]) ** (l + 1.5))
                d = d / math.sqrt(float(d @ pair @ d))
                shell_l.append(l)
                shell_ao.append(ao)
                ao += 2 * l + 1
                exps.append(e)
                coefs.append(d)
                shell_prim.append(shell_prim[-1] + e.size)
            if ao > AO_PAD:
                raise ValueError(f"{sym}: {ao} functions, more than {AO_PAD}")
            self.symbols.append(sym)
            elem_shell.append(len(shell_l))
        self.elem_shell = np.asarray(elem_shell, np.int32)
        self.shell_l = np.asarray(shell_l, np.int32)
        self.shell_prim = np.asarray(shell_prim, np.int32)
        self.shell_ao = np.asarray(shell_ao, np.int32)
        self.prim_exp = np.concatenate(exps) if exps else np.zeros(0, np.float64)
        self.prim_coef = np.concatenate(coefs) if coefs else np.zeros(0, np.float64)
        self.elem_nshell = np.diff(self.elem_shell).astype(np.int64)
        self.elem_nao = np.array([int((2 * self.shell_l[a:b] + 1).sum())
                                  for a, b in zip(self.elem_shell[:-1], self.elem_shell[1:])], np.int64)
        self.elem_of_z = np.full(len(SYMBOLS), -1, np.int64)
        for k, s in enumerate(self.symbols):
            self.elem_of_z[_Z_OF[s]] = k
        self._device = {}

    @classmethod
    def from_pyscf(cls, d: dict) -> "Basis":
        """From pyscf's internal format ``{symbol: [[l, [exp, c1, c2, ...], ...], ...]}`` (what ``mol._basis`` holds
        and ``pyscf.gto.basis.load`` returns per element): every coefficient column is one shell.  Raises ValueError
        naming the element for l > 3, more than 39 functions, a non-positive exponent or an empty element."""
        out = {}
        for name, entries in d.items():
            shells = []
            for entry in entries:
                l, rows = int(entry[0]), entry[1:]
                if rows and not isinstance(rows[0], (list, tuple, np.ndarray)):  # [l, kappa, [exp, ...], ...]
                    rows = rows[1:]
                rows = [list(r) for r in rows]
                if not rows or min(len(r) for r in rows) < 2 or len({len(r) for r in rows}) != 1:
                    raise ValueError(f"{name}: a shell needs rows of one length [exp, c1, ...], got {rows!r}")
                tab = np.asarray(rows, np.float64)
                shells += [(l, tab[:, 0], tab[:, k]) for k in range(1, tab.shape[1])]
            out[name] = shells
        return cls(out)

    @classmethod
    def from_nwchem(cls, text: str) -> "Basis":
        """From NWChem text, the format pyscf and the Basis Set Exchange ship: ``#`` comments, optional ``BASIS ...``
        and ``END`` lines, blocks headed ``<symbol> <S|P|D|F|SP>`` whose rows are ``exp c1 [c2 ...]`` (several
        columns: a general contraction, one shell per column; ``SP``: the first column is an s shell, the second a p
        shell), Fortran ``D`` exponents.  Raises ValueError as :meth:`from_pyscf` does."""
        out, rows, head = {}, [], None

        def close():
            if head is None:
                return
            sym, kind = head
            if not rows or len({len(r) for r in rows}) != 1 or len(rows[0]) < 2:
                raise ValueError(f"{sym}: a {kind} block needs rows of one length 'exp c1 ...'")
            tab = np.asarray(rows, np.float64)
            if kind == "SP":
                if tab.shape[1] != 3:
                    raise ValueError(f"{sym}: an SP block needs rows 'exp c_s c_p'")
                out[sym] += [(0, tab[:, 0], tab[:, 1]), (1, tab[:, 0], tab[:, 2])]
            else:
                out[sym] += [(_L_OF[kind], tab[:, 0], tab[:, k]) for k in range(1, tab.shape[1])]

        for raw in text.splitlines():
            line = raw.split("#", 1)[0].strip()
            if not line or line.upper().startswith("BASIS") or line.upper() == "END":
                continue
            toks = line.split()
            if toks[0][0].isalpha():
                close()
                if len(toks) != 2 or (toks[1].upper() != "SP" and toks[1].upper() not in _L_OF):
                    raise ValueError(f"cannot read the block header {line!r}")
                head, rows = (_symbol(toks[0]), toks[1].upper()), []
                out.setdefault(head[0], [])
            else:
                if head is None:
                    raise ValueError(f"numbers before any block header: {line!r}")
                rows.append([float(re.sub(r"[dD]", "e", t)) for t in toks])
        close()
        return cls(out)

    def __len__(self):
        return len(self.symbols)

    def table(self) -> np.ndarray:
        """The int32 array x2g_one_electron_blocks takes: elem_shell, shell_l, shell_prim, shell_ao end to end."""
        return np.ascontiguousarray(np.concatenate([self.elem_shell, self.shell_l, self.shell_prim, self.shell_ao])
                                    .astype(np.int32))

    def device_tables(self, device):
        """(table, prim_exp, prim_coef) on ``device``, uploaded once."""
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device)
                                      for a in (self.table(), self.prim_exp, self.prim_coef))
        return self._device[key]

    def elements(self, Z) -> np.ndarray:
        """int64 table indices of the atomic numbers ``Z``; ValueError for an element the basis does not hold."""
        Z = np.asarray(Z, np.int64).reshape(-1)
        if Z.size and (Z.min() < 1 or Z.max() >= len(SYMBOLS)):
            raise ValueError(f"atomic numbers must lie in [1, {len(SYMBOLS) - 1}]")
        e = self.elem_of_z[Z]
        if bool((e < 0).any()):
            raise ValueError(f"the basis has no element {SYMBOLS[int(Z[e < 0][0])]} (it has {', '.join(self.symbols)})")
        return e


def _host_ints(a, what):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    if a.dtype.kind not in "iu":
        raise TypeError(f"{what} must hold integers, got {a.dtype}")
    return a.astype(np.int64).reshape(-1)


def one_electron_matrices(pos: torch.Tensor, Z, atom_start, basis: Basis, pairs: torch.Tensor | None = None,
                          unit: float = BOHR) -> AOMatrices:
    """S and H_core of M molecules on the device, one launch (x2g_one_electron_blocks).

    ``pos`` float64 [N, 3] on the GPU, in angstrom (divided by ``unit`` in float64); ``Z`` int [N] (numpy or torch;
    it is read on the host, where the AO layout is made); ``atom_start`` int [M + 1].  In the result ``hcore`` is
    undivided and ``hcore_div`` is each molecule's sum of Z in float64, the neutral molecule's electron count that
    ``geom_scf_6`` divides by; ``ao_begin`` / ``ao_end`` / ``mat_start`` / ``mol_nao`` follow from the basis.

    ``pairs`` None: every unordered atom pair of every molecule, the diagonal included: complete matrices.
    Otherwise int64 [2, P] on the GPU, batch-global atom indices (e.g. the bonds): reduced there to unique unordered
    pairs, their blocks and the transposed blocks are written and every other element is 0.  One device reduction
    checks that every index is inside [0, N) and both atoms share a molecule; ValueError if not.  The pairs are
    launched heaviest first.  CPU tensors raise: there is no CPU implementation."""
    return plan_one_electron(pos, Z, atom_start, basis, pairs, unit).run()


class OneElectronLaunch:
    """One prepared x2g_one_electron_blocks call: ``matrices`` (the zero-filled :class:`AOMatrices` it writes),
    ``num_pairs`` (unique unordered atom pairs, 0 when there is nothing to launch) and :meth:`run`, which enqueues
    the launch on the current stream and returns ``matrices``; it may be run again (a timing loop does)."""

    __slots__ = ("matrices", "num_pairs", "_args", "_keep", "_device")

    def __init__(self, matrices, num_pairs, args, keep, device):
        self.matrices, self.num_pairs, self._args, self._keep, self._device = matrices, num_pairs, args, keep, device

    def run(self) -> AOMatrices:
        if self._args is not None:
            with torch.cuda.device(self._device):
                _lib.call("x2g_one_electron_blocks", *self._args, _lib.stream_ptr(self._device))
        return self.matrices


def plan_one_electron(pos, Z, atom_start, basis, pairs=None, unit=BOHR) -> OneElectronLaunch:
    """What :func:`one_electron_matrices` does up to the launch (same arguments, same checks): the host's layout, the
    uploads and the pair list, as a :class:`OneElectronLaunch` that keeps what the arguments point to alive."""
    from .graph import _atom_start

    if not torch.is_tensor(pos) or not pos.is_cuda:
        where = pos.device if torch.is_tensor(pos) else type(pos).__name__
        raise RuntimeError(f"one_electron_matrices needs pos on a GPU, it is on {where} (no CPU fallback by design)")
    if pos.dim() != 2 or pos.shape[1] != 3 or pos.dtype != torch.float64:
        raise ValueError(f"pos must be float64 [N, 3], got {pos.dtype} {tuple(pos.shape)}")
    dev = pos.device
    N = int(pos.shape[0])
    z = _host_ints(Z, "Z")
    if z.shape[0] != N:
        raise ValueError(f"Z has {z.shape[0]} entries for {N} atoms")
    start = _atom_start(atom_start, N)
    M = int(start.shape[0]) - 1
    counts = np.diff(start)
    elem = basis.elements(z)
    nao_atom = basis.elem_nao[elem]
    mol_of = np.repeat(np.arange(M, dtype=np.int64), counts)
    mol_nao = np.bincount(mol_of, weights=nao_atom, minlength=M).astype(np.int64) if M else np.zeros(0, np.int64)
    ends = np.cumsum(nao_atom)
    mol_off = np.concatenate([[0], np.cumsum(mol_nao)])[:-1]
    ao_end = ends - mol_off[mol_of] if N else np.zeros(0, np.int64)
    ao_begin = ao_end - nao_atom
    sizes = mol_nao ** 2
    mat_start = np.concatenate([[0], np.cumsum(sizes)])[:-1].astype(np.int64)
    total = int(sizes.sum())
    nelec = np.bincount(mol_of, weights=z.astype(np.float64), minlength=M) if M else np.zeros(0, np.float64)

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a.astype(dtype))).to(dev)

    ovlp = torch.zeros(total, dtype=torch.float64, device=dev)
    hcore = torch.zeros(total, dtype=torch.float64, device=dev)
    out = AOMatrices(ovlp, hcore, up(mat_start, np.int64), up(mol_nao, np.int32), up(nelec, np.float64),
                     up(ao_begin, np.int32), up(ao_end, np.int32), torch.from_numpy(start.copy()))
    atom_mol = up(mol_of, np.int32)
    nao_dev = up(nao_atom, np.int64)
    if pairs is None:
        parts = []
        for m in range(M):
            i, j = np.triu_indices(int(counts[m]))
            parts.append(np.stack([i, j]) + int(start[m]))
        pr = up(np.concatenate(parts, axis=1) if parts else np.zeros((2, 0), np.int64), np.int64)
    else:
        if not torch.is_tensor(pairs) or not pairs.is_cuda:
            raise RuntimeError("one_electron_matrices needs pairs on the GPU (no CPU fallback by design)")
        if pairs.dim() != 2 or pairs.shape[0] != 2:
            raise ValueError(f"pairs must be [2, P], got {tuple(pairs.shape)}")
        pr = pairs.to(device=dev, dtype=torch.int64)
        if pr.shape[1]:
            lo, hi = torch.minimum(pr[0], pr[1]), torch.maximum(pr[0], pr[1])
            outside = (lo < 0) | (hi >= N)
            lo_c, hi_c = lo.clamp(0, max(N - 1, 0)), hi.clamp(0, max(N - 1, 0))
            bad = outside | (atom_mol[lo_c] != atom_mol[hi_c]) if N else outside
            if bool(bad.any()):  # the one reduction read back
                raise ValueError("pairs must hold atom indices inside [0, N) whose two atoms share a molecule")
            key = torch.unique(lo * N + hi)
            pr = torch.stack([key // N, key % N])
    P = int(pr.shape[1])
    if P == 0 or total == 0:
        return OneElectronLaunch(out, 0, None, (), dev)
    # heaviest blocks first: a heavy-heavy pair costs several times an H-H pair, and the tail of the launch is then
    # made of the cheap ones (stable, so the order is a function of the pair set alone)
    order = torch.argsort(nao_dev[pr[0]] * nao_dev[pr[1]], descending=True, stable=True)
    pr = pr[:, order].contiguous()
    # a true float64 division, as numpy's on the host: by a Python scalar torch would multiply with the reciprocal
    bohr = torch.div(pos.detach(), torch.tensor(unit, dtype=torch.float64, device=dev)).contiguous()
    tab, pexp, pcoef = basis.device_tables(dev)
    host_tab = basis.table()
    charge, elem_dev, start_dev = up(z, np.int32), up(elem, np.int32), up(start, np.int64)
    p, i64 = _lib.ptr, ctypes.c_int64
    args = (p(tab), host_tab.ctypes.data_as(ctypes.c_void_p), p(pexp), p(pcoef), i64(len(basis)),
            i64(int(basis.shell_l.shape[0])), i64(int(basis.prim_exp.shape[0])), p(bohr), p(charge), p(elem_dev),
            p(atom_mol), p(out.ao_begin), p(start_dev), p(out.mat_start), p(out.mol_nao), i64(M), i64(N), i64(total),
            p(pr), i64(P), p(ovlp), p(hcore))
    # (what the pointers refer to stays alive with the launch object; once that is dropped, the caching allocator hands
    # the temporaries' memory out again on this stream only)
    return OneElectronLaunch(out, P, args, (host_tab, bohr, charge, elem_dev, start_dev, atom_mol, pr), dev)


def parse_geometry(geom: str):
    """(symbols, float64 [n, 3]) of an xyz record's text: the first two lines are skipped, as ``geom_scf_6`` skips
    them, and every other line is ``El x y z``.  The coordinates are parsed from the text in float64."""
    symbols, xyz = [], []
    for line in geom.strip().split("\n")[2:]:
        toks = line.replace("*^", "E").split()
        if not toks:
            continue
        if len(toks) != 4:
            raise ValueError(f"bad atom line {line!r}")
        symbols.append(_symbol(toks[0]))
        xyz.append([float(t) for t in toks[1:]])
    return symbols, np.asarray(xyz, np.float64).reshape(-1, 3)


def record_geometries(records):
    """(float64 [N_all, 3] positions in angstrom, int64 [M + 1] atom_start) of ``MolRecord``s, parsed from each
    record's text; ValueError naming the record whose text and ``Z`` disagree in length."""
    parts, counts = [], []
    for k, rec in enumerate(records):
        xyz = parse_geometry(rec.atom)[1]
        if xyz.shape[0] != int(rec.Z.shape[0]):
            raise ValueError(f"record {k} (idx {int(rec.idx.reshape(-1)[0])}): {xyz.shape[0]} atom lines in its text "
                             f"for {int(rec.Z.shape[0])} atoms")
        parts.append(xyz)
        counts.append(xyz.shape[0])
    pos = np.concatenate(parts) if parts else np.zeros((0, 3), np.float64)
    return pos, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def geom_scf_6(geom: str, basis: Basis, device="cuda"):
    """The reference's call for one molecule (scf.py:27), with the basis as an argument: ``(mat_ovlp,
    mat_hcore / nelectron, aoslice)``, the matrices as CPU float64 tensors [nao, nao] (the division in float64, by
    the neutral molecule's electron count) and ``aoslice`` int64 [n, 4] as pyscf's ``aoslice_by_atom()`` gives it:
    columns 0-1 each atom's shell range, columns 2-3 its AO range.  After the two skipped lines every line must be
    ``El x y z`` (a line with a fifth column, such as raw QM9's partial charges, raises ValueError, as pyscf rejects
    it), and a text without an atom line raises ValueError."""
    symbols, xyz = parse_geometry(geom)
    if not symbols:
        raise ValueError("geom_scf_6: the text holds no atom line after its first two lines")
    z = np.array([_Z_OF[s] for s in symbols], np.int64)
    n = len(symbols)
    ao = one_electron_matrices(torch.from_numpy(xyz).to(device), z, np.array([0, n]), basis)
    nao = int(ao.mol_nao[0])
    S = ao.ovlp.cpu().reshape(nao, nao)
    H = ao.hcore.cpu().reshape(nao, nao)
    elem = basis.elements(z)
    sh_end = np.cumsum(basis.elem_nshell[elem])
    aoslice = np.stack([sh_end - basis.elem_nshell[elem], sh_end, ao.ao_begin.cpu().numpy().astype(np.int64),
                        ao.ao_end.cpu().numpy().astype(np.int64)], axis=1).astype(np.int64)
    return S, H / int(z.sum()), aoslice
