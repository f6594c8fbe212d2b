"""The model's own input: the [E, 338] edge features of the reference's ``bi_gen_edge_feature_6`` (scf.py:50-119)
from overlap and core-Hamiltonian matrices, as one kernel (csrc/ao_features.hip, include/x2g_features.h).

The reference makes the matrices with pyscf (``geom_scf_6``) and then turns them into features with a Python loop
over edges.  This module is the second half: whoever has S and H_core from any integral code, pyscf elsewhere, a file
of matrices or :mod:`x2gnn.integrals` (the first half, on the device too), gets the real ``edge_attr`` on the device.

* :class:`AOMatrices` is the flat container the ABI takes: the matrices of M molecules end to end, each atom's AO
  range, and optionally the divisor of each molecule's H_core (the reference divides it by the electron count).
* :func:`ao_edge_features` is the batched call: any number of molecules' edges in one launch.
* :func:`bi_gen_edge_feature_6` has the reference's signature for one molecule, so a user's ``mapping`` function
  runs with its import changed and nothing else.

The operation is stated exactly in include/x2g_features.h, the reference's placement of a (9, 39) block at row 0
(its branch for that shape is never taken; the published weights were trained on the result) included.  There is
no CPU implementation: without a GPU these calls raise.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .synth import EDGE_FEATURES

AO_PAD = 39  # functions of a heavy atom in 6-311+G(3df,2p): the side of the reference's zero pad
# the 13 index groups of 0..38, rows and columns alike: 5 s, 4 p, 3 d and 1 f shells
AO_GROUPS = ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 8), (8, 11), (11, 14), (14, 17), (17, 22), (22, 27),
             (27, 32), (32, 39))
if 2 * len(AO_GROUPS) ** 2 != EDGE_FEATURES:
    raise AssertionError(f"2 x {len(AO_GROUPS)}^2 features do not match synth.EDGE_FEATURES = {EDGE_FEATURES}")

_FLAT = ("ovlp", "hcore", "mat_start", "mol_nao", "hcore_div", "ao_begin", "ao_end", "atom_start")


def _host(a, what):
    """``a`` (numpy or torch) as a numpy array on the host."""
    if torch.is_tensor(a):
        return a.detach().cpu().numpy()
    if isinstance(a, np.ndarray):
        return a
    raise TypeError(f"{what} must be a numpy array or a torch tensor, got {type(a).__name__}")


class AOMatrices:
    """The AO matrices of M molecules as flat arrays (torch tensors, all on one device except ``atom_start``):

    ``ovlp``, ``hcore`` float64, molecule m's [nao, nao] row-major matrix from element ``mat_start[m]`` (int64 [M]);
    ``mol_nao`` int32 [M]; ``hcore_div`` float64 [M] or None (``hcore`` is divided by it in float64 inside the
    kernel); ``ao_begin`` / ``ao_end`` int32 [N_all], each atom's AO range local to its molecule's matrix;
    ``atom_start`` int64 [M + 1] on the host, the prefix sum of the molecules' atom counts."""

    def __init__(self, ovlp, hcore, mat_start, mol_nao, hcore_div, ao_begin, ao_end, atom_start):
        self.ovlp, self.hcore, self.mat_start, self.mol_nao = ovlp, hcore, mat_start, mol_nao
        self.hcore_div, self.ao_begin, self.ao_end, self.atom_start = hcore_div, ao_begin, ao_end, atom_start

    @classmethod
    def from_molecules(cls, molecules) -> "AOMatrices":
        """From ``[(S, H, aoslice[, nelectron]), ...]``: S and H [nao, nao] float64 (numpy or torch), ``aoslice``
        [n_atoms, 4] as pyscf's ``aoslice_by_atom()`` returns it (columns 2 and 3: each atom's AO begin and end).
        With ``nelectron`` given (for every molecule or for none) H is stored as it is and divided in the kernel.
        Raises TypeError for a dtype other than float64 and ValueError, naming the molecule and the atom, for
        matrices that are not square or not of one shape and for an AO range that is empty, reversed, wider than
        39 or outside the matrix."""
        molecules = list(molecules)
        S_parts, H_parts, naos, divs, begins, ends, counts = [], [], [], [], [], [], []
        for m, mol in enumerate(molecules):
            if len(mol) not in (3, 4):
                raise ValueError(f"molecule {m}: expected (S, H, aoslice[, nelectron]), got {len(mol)} items")
            S, H, sl = _host(mol[0], f"molecule {m}: S"), _host(mol[1], f"molecule {m}: H"), _host(mol[2], "aoslice")
            for name, a in (("S", S), ("H", H)):
                if a.dtype != np.float64:
                    raise TypeError(f"molecule {m}: {name} must be float64, got {a.dtype}")
                if a.ndim != 2 or a.shape[0] != a.shape[1]:
                    raise ValueError(f"molecule {m}: {name} must be a square matrix, got shape {a.shape}")
            if S.shape != H.shape:
                raise ValueError(f"molecule {m}: S {S.shape} and H {H.shape} differ in shape")
            if sl.ndim != 2 or sl.shape[1] != 4 or sl.dtype.kind not in "iu":
                raise ValueError(f"molecule {m}: aoslice must be an integer [n_atoms, 4] array, got "
                                 f"{sl.dtype} {sl.shape}")
            nao = S.shape[0]
            b, e = sl[:, 2].astype(np.int64), sl[:, 3].astype(np.int64)
            for atom in range(len(b)):
                if not 0 <= b[atom] < e[atom] <= nao:
                    raise ValueError(f"molecule {m}, atom {atom}: AO range [{b[atom]}, {e[atom]}) is empty, reversed "
                                     f"or outside the {nao} x {nao} matrix")
                if e[atom] - b[atom] > AO_PAD:
                    raise ValueError(f"molecule {m}, atom {atom}: {e[atom] - b[atom]} AOs, more than {AO_PAD}")
            if len(mol) == 4:
                divs.append(float(mol[3]))
            S_parts.append(np.ascontiguousarray(S).reshape(-1))
            H_parts.append(np.ascontiguousarray(H).reshape(-1))
            naos.append(nao)
            begins.append(b)
            ends.append(e)
            counts.append(len(b))
        if divs and len(divs) != len(molecules):
            raise ValueError("nelectron must be given for every molecule or for none")

        def cat(parts, dtype):
            return torch.from_numpy(np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype))

        sizes = np.asarray(naos, np.int64) ** 2
        return cls(cat(S_parts, np.float64), cat(H_parts, np.float64),
                   torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)),
                   torch.from_numpy(np.asarray(naos, np.int32)),
                   torch.from_numpy(np.asarray(divs, np.float64)) if divs else None,
                   cat(begins, np.int32), cat(ends, np.int32),
                   torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)))

    def __len__(self):
        return int(self.mol_nao.shape[0])

    @property
    def device(self):
        return self.ovlp.device

    @property
    def num_atoms(self):
        return int(self.ao_begin.shape[0])

    def atom_mol(self) -> torch.Tensor:
        """int32 [N_all] on the matrices' device: the molecule of each atom, for all molecules in their order."""
        counts = self.atom_start[1:] - self.atom_start[:-1]
        return torch.repeat_interleave(torch.arange(len(self), dtype=torch.int32), counts).to(self.device)

    def slice(self, lo: int, hi: int) -> "AOMatrices":
        """Molecules ``lo`` to ``hi`` (exclusive) as a container of their own."""
        if not 0 <= lo <= hi <= len(self):
            raise IndexError(f"molecules [{lo}, {hi}) of {len(self)}")
        a0, a1 = int(self.atom_start[lo]), int(self.atom_start[hi])
        nao = self.mol_nao[lo:hi].to(torch.int64)
        m0 = int(self.mat_start[lo]) if lo < hi else 0
        m1 = int(self.mat_start[hi - 1]) + int(nao[-1]) ** 2 if lo < hi else 0
        return AOMatrices(self.ovlp[m0:m1], self.hcore[m0:m1], self.mat_start[lo:hi] - m0, self.mol_nao[lo:hi],
                          None if self.hcore_div is None else self.hcore_div[lo:hi], self.ao_begin[a0:a1],
                          self.ao_end[a0:a1], self.atom_start[lo:hi + 1] - a0)

    def to(self, device) -> "AOMatrices":
        """A copy with every array on ``device`` (``atom_start`` stays on the host)."""
        return AOMatrices(*(getattr(self, k) if k == "atom_start" or getattr(self, k) is None
                            else getattr(self, k).to(device) for k in _FLAT))

    def save(self, path):
        """An ``.npz`` of the flat arrays (``hcore_div`` left out when there is none)."""
        arrays = {k: getattr(self, k).detach().cpu().numpy() for k in _FLAT if getattr(self, k) is not None}
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path) -> "AOMatrices":
        with np.load(path, allow_pickle=False) as z:
            return cls(*(torch.from_numpy(z[k]) if k in z.files else None for k in _FLAT))


def ao_edge_features(ao: AOMatrices, edge_index: torch.Tensor, atom_mol: torch.Tensor,
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """``edge_attr`` float32 [E, 338] on the device, one launch (x2g_ao_edge_features).  ``edge_index`` int64
    [2, E] holds indices into ``atom_mol`` / ``ao.ao_begin`` (batch-global, edges in any order); ``atom_mol`` [N] is
    the molecule of each atom (``ao.atom_mol()`` when the batch is every molecule of ``ao`` in order).  An edge the
    kernel finds invalid (see the header) gets a NaN row.  CPU tensors raise: there is no CPU implementation.

    ``out``: a contiguous float32 [E, 338] tensor on the matrices' device, e.g. a row slice of a dataset's
    ``edge_attr``; the rows are written there and ``out`` is returned (ValueError for another shape, dtype, device
    or layout).  Without it a new tensor is returned."""
    for name, t in (("ao", ao.ovlp), ("edge_index", edge_index), ("atom_mol", atom_mol)):
        if not t.is_cuda:
            raise RuntimeError(f"ao_edge_features needs GPU tensors, {name} is on {t.device} (no CPU fallback by "
                               f"design; AOMatrices.to(device))")
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"edge_index must be [2, E], got {tuple(edge_index.shape)}")
    if atom_mol.dim() != 1 or atom_mol.shape[0] != ao.num_atoms:
        raise ValueError(f"atom_mol has shape {tuple(atom_mol.shape)} for {ao.num_atoms} atoms")
    E = int(edge_index.shape[1])
    if out is None:
        out = torch.empty((E, EDGE_FEATURES), device=ao.device, dtype=torch.float32)
    elif (not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (E, EDGE_FEATURES)
          or out.device != ao.device or not out.is_contiguous()):
        what = f"{out.dtype} {tuple(out.shape)} on {out.device}" if torch.is_tensor(out) else type(out).__name__
        raise ValueError(f"out must be a contiguous float32 [{E}, {EDGE_FEATURES}] tensor on {ao.device}, got {what}")
    if E == 0:
        return out
    ei = edge_index.to(torch.int64).contiguous()
    am = atom_mol.to(torch.int32).contiguous()
    p = _lib.ptr
    with torch.cuda.device(ao.device):
        _lib.call("x2g_ao_edge_features", p(ao.ovlp), p(ao.hcore), p(ao.mat_start), p(ao.mol_nao), p(ao.hcore_div),
                  p(ao.ao_begin), p(ao.ao_end), p(am), p(ei), ctypes.c_int64(len(ao)), ctypes.c_int64(ao.num_atoms),
                  ctypes.c_int64(E), p(out), _lib.stream_ptr(ao.device))
    # (ei and am may be temporaries: the caching allocator hands their memory out again on this stream only)
    return out


def bi_gen_edge_feature_6(mat_ovlp, mat_hcore, aoslice, edge_index, Z=None) -> torch.Tensor:
    """The reference's call for one molecule (scf.py:50): ``mat_hcore`` already divided, as ``geom_scf_6`` returns
    it; ``Z`` unused, as there.  Inputs on the CPU are uploaded, and the rows come back as a CPU float32 tensor, as
    the reference's are; inputs on a GPU give the rows on that GPU."""
    ei = edge_index if torch.is_tensor(edge_index) else torch.as_tensor(np.asarray(edge_index))
    on = [t.device for t in (mat_ovlp, mat_hcore, ei) if torch.is_tensor(t) and t.is_cuda]
    device = on[0] if on else torch.device("cuda")
    ao = AOMatrices.from_molecules([(mat_ovlp, mat_hcore, aoslice)]).to(device)
    out = ao_edge_features(ao, ei.to(device=device, dtype=torch.int64).reshape(2, -1), ao.atom_mol())
    return out if on else out.cpu()
