"""The graph the edge features sit on, built where they are needed: the reference's radius graph
(atom_graph.py:32-45, ``calculate_Dij`` + ``gen_bonds_mini``) of any number of molecules in two launches on the
device (csrc/radius_graph.hip, include/x2g_graph.h), with the per-atom and per-molecule counts a dataset caches.

The operation, its float32 Gram form and its edge order are stated in include/x2g_graph.h.  There is no CPU
implementation: without a GPU :func:`radius_graph` raises (``datasets.bonds(datasets.distance_matrix(R))`` is the
host's form of the same bonds, one molecule at a time).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib


class RadiusGraph:
    """What :func:`radius_graph` returns.  On the device: ``edge_index`` int64 [2, E] (molecule-local ids, sorted by
    (molecule, i, j)), ``edge_index_global`` (the same plus each molecule's ``atom_start``) or None, ``degree`` int32
    [N], ``row_start`` int64 [N + 1] (the exclusive scan of ``degree``; edge rows of atom a: ``row_start[a]`` to
    ``row_start[a + 1]``).  On the host, numpy, one entry per molecule: ``edges``, ``triplets`` (sum of d (d - 1)),
    ``max_degree`` (all int64) and ``last_bonded`` (int32: the highest local atom id with an edge, -1 for none)."""

    __slots__ = ("edge_index", "edge_index_global", "degree", "row_start", "edges", "triplets", "max_degree",
                 "last_bonded")

    def __init__(self, edge_index, edge_index_global, degree, row_start, edges, triplets, max_degree, last_bonded):
        self.edge_index, self.edge_index_global, self.degree, self.row_start = (edge_index, edge_index_global, degree,
                                                                                row_start)
        self.edges, self.triplets, self.max_degree, self.last_bonded = edges, triplets, max_degree, last_bonded

    @property
    def num_edges(self) -> int:
        return int(self.edge_index.shape[1])


def _atom_start(atom_start, N):
    """``atom_start`` as a host int64 array, checked: starts at 0, never decreases, ends at ``N``."""
    a = atom_start.detach().cpu().numpy() if torch.is_tensor(atom_start) else np.asarray(atom_start)
    if a.ndim != 1 or a.shape[0] < 1 or a.dtype.kind not in "iu":
        raise ValueError(f"atom_start must be an integer [M + 1] array, got {a.dtype} {a.shape}")
    a = np.ascontiguousarray(a.astype(np.int64))
    if int(a[0]) != 0 or int(a[-1]) != N or bool((np.diff(a) < 0).any()):
        raise ValueError(f"atom_start must start at 0, never decrease and end at the {N} atoms of pos "
                         f"(starts at {int(a[0])}, ends at {int(a[-1])})")
    return a


def radius_graph(pos: torch.Tensor, atom_start, cutoff: float = 5.0, global_ids: bool = False) -> RadiusGraph:
    """The radius graph of M molecules: ``pos`` float32 [N, 3] on the GPU, ``atom_start`` int64 [M + 1] (numpy or
    torch, checked on the host: starts at 0, never decreases, ends at N; empty molecules allowed).  An edge (i, j)
    of a molecule: ``0 < d(i, j) < cutoff`` in the reference's float32 Gram form (include/x2g_graph.h).  Two
    launches (x2g_radius_graph_count, x2g_radius_graph_fill) around the one host read: E and the four per-molecule
    arrays, in one copy.  ``global_ids``: also return ``edge_index_global``, what ``ao_edge_features`` takes.
    CPU tensors raise: there is no CPU implementation."""
    if not torch.is_tensor(pos) or not pos.is_cuda:
        where = pos.device if torch.is_tensor(pos) else type(pos).__name__
        raise RuntimeError(f"radius_graph needs pos on a GPU, it is on {where} (no CPU fallback by design)")
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError(f"pos must be [N, 3], got {tuple(pos.shape)}")
    dev = pos.device
    N = int(pos.shape[0])
    start = _atom_start(atom_start, N)
    M = int(start.shape[0]) - 1
    if N == 0 or M == 0:
        empty = torch.zeros((2, 0), dtype=torch.int64, device=dev)
        return RadiusGraph(empty, empty.clone() if global_ids else None,
                           torch.zeros(N, dtype=torch.int32, device=dev), torch.zeros(N + 1, dtype=torch.int64, device=dev),
                           np.zeros(M, np.int64), np.zeros(M, np.int64), np.zeros(M, np.int64), np.full(M, -1, np.int32))
    xyz = pos.detach().to(torch.float32).contiguous()
    start_d = torch.from_numpy(start).to(dev)
    # one int64 allocation: row_start [N + 1], then the per-molecule outputs, so that what the host needs
    # (row_start[N] = E and the four [M] arrays) is one contiguous run and one copy
    words = torch.empty(N + 1 + 3 * M + (M + 1) // 2, dtype=torch.int64, device=dev)
    row_start, mol_edges, mol_trips, mol_max, tail = torch.split(words, [N + 1, M, M, M, (M + 1) // 2])
    last = tail.view(torch.int32)[:M]
    degree = torch.empty(N, dtype=torch.int32, device=dev)
    lib, p = _lib.load(), _lib.ptr
    ws = torch.empty(max(int(lib.x2g_radius_graph_count_workspace(N)), 8), dtype=torch.uint8, device=dev)
    i64, f32 = ctypes.c_int64, ctypes.c_float
    with torch.cuda.device(dev):
        _lib.call("x2g_radius_graph_count", p(xyz), p(start_d), i64(N), i64(M), f32(cutoff), p(degree), p(row_start),
                  p(mol_edges), p(mol_trips), p(mol_max), p(last), p(ws), ctypes.c_size_t(ws.numel()),
                  _lib.stream_ptr(dev))
        host = words[N:].cpu().numpy()  # the one read (it waits for the count)
        E = int(host[0])
        edges, triplets, max_degree = (host[1 + k * M:1 + (k + 1) * M].copy() for k in range(3))
        last_bonded = host[1 + 3 * M:].view(np.int32)[:M].copy()
        edge_local = torch.empty((2, E), dtype=torch.int64, device=dev)
        edge_global = torch.empty((2, E), dtype=torch.int64, device=dev) if global_ids else None
        if E:
            _lib.call("x2g_radius_graph_fill", p(xyz), p(start_d), p(row_start), i64(N), i64(M), f32(cutoff), i64(E),
                      p(edge_local), p(edge_global), _lib.stream_ptr(dev))
    # (xyz and start_d may be temporaries: the caching allocator hands their memory out again on this stream only)
    return RadiusGraph(edge_local, edge_global, degree, row_start, edges, triplets, max_degree, last_bonded)
