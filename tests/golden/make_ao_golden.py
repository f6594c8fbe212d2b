"""Generate ``ao_features.npz`` by running the REFERENCE's ``bi_gen_edge_feature_6`` (scf.py:50-119; test
infrastructure).  Run where the reference tree is present, like make_golden.py:

    python tests/golden/make_ao_golden.py

scf.py imports pyscf at module level (``gto.Mole`` objects for nine elements, built on import) but
``bi_gen_edge_feature_6`` uses nothing of it.  A stub ``pyscf`` written here stands in: ``gto.Mole`` as an empty class
whose ``build()`` does nothing, and empty ``dft`` and ``lib`` modules.  The reference file is not modified, and
``sys.dont_write_bytecode`` keeps ``__pycache__`` out of its tree.

Three seeded molecules of random symmetric matrices whose magnitudes span seven decades (tests/ao_features_ref.py):
  a  AO counts [39, 9, 9, 39, 9], all 20 directed edges: every placement branch, the (9, 39) block included
  b  [9, 9]: H2-like, two edges
  c  [39, 13, 1, 9], all 12 directed edges: the "every other shape" branch at sizes that are neither 9 nor 39
H is divided by an electron count in float64 here, as ``geom_scf_6`` does (scf.py:48), and the divided matrix is what
the reference function gets.  Stored per molecule ``k``: ``k.S``, ``k.H`` (undivided), ``k.nelectron``, ``k.Hdiv``,
``k.aoslice``, ``k.edge_index`` and ``k.out``, the reference's float32 [E, 338].  Data only.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import ao_features_ref as ar  # noqa: E402
from ref_import import REF  # noqa: E402

CASES = {"a": ([39, 9, 9, 39, 9], 42, 501), "b": ([9, 9], 2, 502), "c": ([39, 13, 1, 9], 30, 503)}


def install_stub_pyscf():
    class Mole:
        def build(self):
            return self

    pyscf = types.ModuleType("pyscf")
    pyscf.gto = types.ModuleType("pyscf.gto")
    pyscf.gto.Mole = Mole
    pyscf.dft = types.ModuleType("pyscf.dft")
    pyscf.lib = types.ModuleType("pyscf.lib")
    for mod in (pyscf, pyscf.gto, pyscf.dft, pyscf.lib):
        sys.modules[mod.__name__] = mod


def import_reference_scf():
    if not os.path.isdir(REF):
        raise RuntimeError("reference tree not present (fixture generation runs only where it is)")
    sys.dont_write_bytecode = True
    install_stub_pyscf()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import scf  # noqa: E402

    return scf


def main():
    scf = import_reference_scf()
    out = {}
    for name, (counts, nelectron, seed) in CASES.items():
        rng = np.random.default_rng(seed)
        nao = int(sum(counts))
        S, H = ar.random_symmetric(rng, nao), ar.random_symmetric(rng, nao)
        aoslice = ar.aoslice_of(counts)
        edge_index = ar.all_directed_edges(len(counts))
        Hdiv = torch.from_numpy(H) / nelectron  # scf.py:48: mat_hcore / nelectrons, float64
        rows = scf.bi_gen_edge_feature_6(torch.from_numpy(S), Hdiv, aoslice, torch.from_numpy(edge_index), None)
        assert rows.dtype == torch.float32 and tuple(rows.shape) == (edge_index.shape[1], ar.ROW)
        out.update({f"{name}.S": S, f"{name}.H": H, f"{name}.nelectron": np.int64(nelectron),
                    f"{name}.Hdiv": Hdiv.numpy(), f"{name}.aoslice": aoslice, f"{name}.edge_index": edge_index,
                    f"{name}.out": rows.numpy()})
    path = os.path.join(HERE, "ao_features.npz")
    np.savez(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
