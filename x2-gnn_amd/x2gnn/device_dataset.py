"""A dataset that lives on the GPU: every training batch is assembled there (x2g_batch_assemble).

The reference's loop collates a fresh batch on the host every step and copies it over (trainer.py:37-48);
on this card that is the slowest part of a step — the 28 MB ``edge_attr`` [E, 338] concatenation, its
worker-to-parent hand-off and its H2D copy.  All of QM9's ``edge_attr`` is 28-50 GB against 288 GB of HBM,
so :class:`DeviceDataset` keeps the collated dataset resident (PyG's ``InMemoryDataset`` layout: concatenated
tensors, per-molecule slices, ``edge_index`` not incremented) and builds a batch from a list of molecule
indices with one ragged-gather launch.  Per batch the host touches O(B) integers (cached per-molecule sizes)
and uploads one block of 5 B + 2 int64; nothing is read back.

``batch(indices)`` returns the same ``Batch``, key for key, as ``collate([mols[i] for i in indices]).to(device)``
gives with ``data.HOST_SCHEDULE`` False: the center kernels' schedule is made on the device by the plan.
"""
from __future__ import annotations

import numpy as np
import torch

from .data import Batch, molecule_targets
from .padding import Capacity, solve_capacity

_RING = 4  # pinned staging slots for the offset block: a slot is rewritten only after its copy has finished


def molecule_stats(nodes, edges, edge_index):
    """Per-molecule (triplets int64 [M], max out-degree int64 [M], symmetric bool [M]) of a concatenated dataset
    with molecule-local ``edge_index`` (int64 [2, E_all]), vectorised over the whole dataset: equal to
    ``synth.triplet_count``, ``np.bincount(src).max()`` and ``data._is_symmetric`` called molecule by molecule
    (which takes minutes at 130k molecules).  Raises ValueError when a local atom id lies outside its molecule."""
    nodes = np.asarray(nodes, dtype=np.int64)
    edges = np.asarray(edges, dtype=np.int64)
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    M, n_all, e_all = len(nodes), int(nodes.sum()), int(edges.sum())
    if ei.shape[1] != e_all:
        raise ValueError(f"edge_index has {ei.shape[1]} edges, the per-molecule counts sum to {e_all}")
    if e_all == 0:
        return np.zeros(M, np.int64), np.zeros(M, np.int64), np.ones(M, bool)
    atom_start = np.concatenate([[0], np.cumsum(nodes)])[:-1]
    mol = np.repeat(np.arange(M, dtype=np.int64), edges)  # the molecule of each edge
    if bool(((ei < 0) | (ei >= nodes[mol])).any()):
        raise ValueError("edge_index must hold molecule-local atom ids inside each molecule")
    src, dst = ei[0] + atom_start[mol], ei[1] + atom_start[mol]  # dataset-wide atom ids: keys never cross molecules
    deg = np.bincount(src, minlength=n_all)
    key, rev = src * n_all + dst, dst * n_all + src
    order = np.argsort(key, kind="stable")  # (molecule-major: a molecule's atoms are consecutive)
    skey = key[order]
    pos = np.searchsorted(skey, rev)
    has_rev = skey[np.minimum(pos, e_all - 1)] == rev  # np.isin(rev, key), on the sort the duplicate test needs
    # triplets: sum over e = (a->b) of |N_out(b) \ {a}|
    trips = np.bincount(mol, weights=(deg[dst] - has_rev).astype(np.float64), minlength=M).astype(np.int64)
    owner = np.repeat(np.arange(M, dtype=np.int64), nodes)
    max_deg = np.zeros(M, np.int64)
    np.maximum.at(max_deg, owner, deg)
    # symmetric: no directed edge twice (data._is_symmetric sends such a multigraph down the generic path), and
    # every reverse present — with distinct edges that makes the forward and reverse sets equal
    dup = np.bincount(mol[order][1:][skey[1:] == skey[:-1]], minlength=M) > 0
    missing = np.bincount(mol[~has_rev], minlength=M) > 0
    return trips, max_deg, ~(dup | missing)


class DeviceDataset:
    """The collated dataset on one GPU; see the module docstring.

    Host caches (numpy, one entry per molecule): ``nodes``, ``edges``, ``triplets``, ``max_degree``,
    ``symmetric`` and the prefix sums ``atom_start`` / ``edge_start`` ([M + 1]).  Device tensors: ``x`` int64
    [N_all], ``atom_pos`` f32 [N_all, 3], ``edge_index`` int64 [2, E_all] (molecule-local), ``edge_attr`` f32
    [E_all, F] or None, ``y`` f32 [M] (K > 1 targets per molecule: [M, K], gathered per batch by one
    ``index_select`` on the uploaded molecule ids instead of by the assemble kernel), ``mol_trips`` int64 [M]."""

    def __init__(self, mols, device):
        """``mols``: molecule dicts as :func:`x2gnn.data.collate` takes them (``y``: one value each, or the same
        K values each)."""
        M = len(mols)
        nodes = np.fromiter((len(m["x"]) for m in mols), dtype=np.int64, count=M)
        edges = np.fromiter((int(m["edge_num"]) for m in mols), dtype=np.int64, count=M)

        def cat(parts, dtype, tail):
            return np.concatenate(parts) if parts else np.zeros((0,) + tail, dtype)

        x = cat([np.asarray(m["x"], dtype=np.int64).reshape(-1) for m in mols], np.int64, ())
        pos = cat([np.asarray(m["atom_pos"], dtype=np.float32).reshape(-1, 3) for m in mols], np.float32, (3,))
        ei = (np.concatenate([np.asarray(m["edge_index"], dtype=np.int64).reshape(2, -1) for m in mols], axis=1)
              if M else np.zeros((2, 0), np.int64))
        attr = (np.concatenate([np.asarray(m["edge_attr"], dtype=np.float32) for m in mols])
                if M and "edge_attr" in mols[0] else None)
        y = molecule_targets(mols)
        self._init(nodes, edges, x, pos, ei, attr, y, device)

    @classmethod
    def from_collated(cls, dataset, device, num_target=1):
        """From a :class:`x2gnn.datasets.CollatedDataset` (a PyG ``InMemoryDataset`` processed file) after
        ``prepare_target``, so that ``y`` is one value per molecule; with ``num_target`` = K > 1 after
        ``prepare_targets``, ``y`` [M, K]."""
        st, sl = dataset.data._store, dataset.slices
        M = len(dataset)
        y = st["y"]
        if int(num_target) > 1:
            if y.dim() != 2 or tuple(y.shape) != (M, int(num_target)):
                raise ValueError(f"y must be [M, K] = [{M}, {int(num_target)}] (run datasets.prepare_targets first), "
                                 f"got {tuple(y.shape)}")
        elif y.dim() != 1 or int(y.shape[0]) != M:
            raise ValueError(f"y must be [M] = [{M}] (run datasets.prepare_target first), got {tuple(y.shape)}")
        nodes = np.diff(sl["x"].numpy().astype(np.int64))
        edges = np.diff(sl["edge_index"].numpy().astype(np.int64))
        attr = st["edge_attr"].to(torch.float32).numpy() if "edge_attr" in st else None
        self = cls.__new__(cls)
        self._init(nodes, edges, st["x"].to(torch.int64).numpy().reshape(-1),
                   st["atom_pos"].to(torch.float32).numpy().reshape(-1, 3),
                   st["edge_index"].to(torch.int64).numpy().reshape(2, -1), attr,
                   y.to(torch.float32).numpy(), device)
        return self

    @classmethod
    def from_records(cls, records, ao, device, cutoff=5.0, max_edges_per_launch=1 << 18):
        """The dataset ``DeviceDataset(datasets.records_to_data(records, ao, device, cutoff), device)`` builds, every
        device tensor and every host cache equal, made without that path's round trip: ``x``, ``atom_pos`` and ``y``
        are uploaded once, one :func:`x2gnn.graph.radius_graph` call makes the bonds of the whole set on the device,
        ``edge_attr`` is allocated once there and filled through ``ao_edge_features(out=...)`` (as many whole
        molecules as fit ``max_edges_per_launch`` edges per launch, only their matrices on the device at a time),
        and the caches are the kernel's per-molecule counts: no recount, ``symmetric`` all True by construction, no
        feature row ever on the host.

        ``records``: :class:`x2gnn.datasets.MolRecord`; ``ao``: :class:`x2gnn.features.AOMatrices`, molecule k
        belonging to ``records[k]``, or a :class:`x2gnn.integrals.Basis`: each chunk's matrices are then computed on
        the device (:func:`x2gnn.integrals.one_electron_matrices`, only the atom-pair blocks of that chunk's bonds)
        from positions parsed from ``rec.atom`` in float64, as ``geom_scf_6`` takes them, so that nothing but
        positions, ``Z`` and labels is uploaded.  The reference's check ``aoslice.shape[0] == edge_index.max() + 1``
        (qm9_allprop.py:15; the atom count for a molecule without an edge) raises ValueError naming the record
        before any feature launch, a molecule count that differs raises ValueError, and a device that is no GPU
        raises RuntimeError: there is no CPU implementation."""
        from .features import ao_edge_features
        from .graph import radius_graph
        from .integrals import Basis, one_electron_matrices, record_geometries
        from .synth import EDGE_FEATURES

        records = list(records)
        basis = ao if isinstance(ao, Basis) else None
        if basis is None and len(ao) != len(records):
            raise ValueError(f"{len(ao)} molecules of AO matrices for {len(records)} records")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"DeviceDataset.from_records needs a GPU, got device {device} (no CPU fallback by "
                               f"design; datasets.records_to_data is the reference's path)")
        M = len(records)
        nodes = np.fromiter((int(r.Z.shape[0]) for r in records), dtype=np.int64, count=M)

        def cat(parts, dtype, tail):
            return np.concatenate(parts) if parts else np.zeros((0,) + tail, dtype)

        x = cat([np.asarray(r.Z, dtype=np.int64).reshape(-1) for r in records], np.int64, ())
        pos = cat([np.asarray(r.R.to(torch.float32), dtype=np.float32).reshape(-1, 3) for r in records], np.float32,
                  (3,))
        y = molecule_targets([{"y": r.Label} for r in records])
        if int(nodes.sum()) != len(x) or len(pos) != len(x):
            raise ValueError("per-molecule sizes do not match the concatenated tensors")

        self = cls.__new__(cls)
        self.device = device
        self.nodes = nodes
        self.atom_start = np.concatenate([[0], np.cumsum(nodes)]).astype(np.int64)

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(device)

        self.x, self.atom_pos, self.y = up(x), up(pos), up(y)
        g = radius_graph(self.atom_pos, self.atom_start, cutoff)
        if basis is None:
            ao_start = ao.atom_start.numpy().astype(np.int64)
        else:
            pos64, ao_start = record_geometries(records)
            pos64 = up(pos64)
        top = np.where(g.last_bonded >= 0, g.last_bonded.astype(np.int64) + 1, nodes)
        bad = np.flatnonzero(np.diff(ao_start) != top)
        if bad.size:
            k = int(bad[0])
            raise ValueError(f"record {k} (idx {int(records[k].idx.reshape(-1)[0])}): aoslice has "
                             f"{int(ao_start[k + 1] - ao_start[k])} atoms, the bonds reach atom {int(top[k]) - 1}")
        self.edges, self.triplets, self.max_degree = g.edges, g.triplets, g.max_degree
        self.symmetric = np.ones(M, bool)  # the edge test is bitwise symmetric in (i, j): every edge has its reverse
        self.edge_start = np.concatenate([[0], np.cumsum(self.edges)]).astype(np.int64)
        self.edge_index = g.edge_index
        self.num_features = EDGE_FEATURES if M else 0
        self.edge_attr = (torch.empty((int(self.edge_start[-1]), EDGE_FEATURES), dtype=torch.float32, device=device)
                          if M else None)
        lo = 0
        while lo < M:
            hi, total = lo + 1, int(self.edges[lo])
            while hi < M and total + int(self.edges[hi]) <= max_edges_per_launch:
                total += int(self.edges[hi])
                hi += 1
            if total:
                e0, e1 = int(self.edge_start[lo]), int(self.edge_start[hi])
                # local ids -> the chunk's atom numbering, which is the matrices' (ao.atom_start), not the records'
                shift = torch.repeat_interleave(up(ao_start[lo:hi] - ao_start[lo]), up(self.edges[lo:hi]),
                                                output_size=total)
                bonds = self.edge_index[:, e0:e1] + shift
                if basis is None:
                    part = ao.slice(lo, hi).to(device)
                else:
                    a0, a1 = int(ao_start[lo]), int(ao_start[hi])
                    part = one_electron_matrices(pos64[a0:a1], x[a0:a1], ao_start[lo:hi + 1] - a0, basis, pairs=bonds)
                ao_edge_features(part, bonds, part.atom_mol(), out=self.edge_attr[e0:e1])
            lo = hi
        self.mol_trips = up(self.triplets)
        self._stage, self._slot, self._debug_fill = None, 0, None
        return self

    def _init(self, nodes, edges, x, pos, ei, attr, y, device):
        self.device = torch.device(device)
        self.nodes, self.edges = nodes, edges
        if int(nodes.sum()) != len(x) or len(pos) != len(x) or len(y) != len(nodes):
            raise ValueError("per-molecule sizes do not match the concatenated tensors")
        if attr is not None and (attr.ndim != 2 or attr.shape[0] != ei.shape[1]):
            raise ValueError(f"edge_attr has shape {attr.shape} for {ei.shape[1]} edges")
        self.triplets, self.max_degree, self.symmetric = molecule_stats(nodes, edges, ei)
        self.atom_start = np.concatenate([[0], np.cumsum(nodes)]).astype(np.int64)
        self.edge_start = np.concatenate([[0], np.cumsum(edges)]).astype(np.int64)
        self.num_features = int(attr.shape[1]) if attr is not None else 0

        def up(a):  # the one H2D copy of each concatenated tensor
            return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

        self.x, self.atom_pos, self.edge_index, self.y = up(x), up(pos), up(ei), up(y)
        self.edge_attr = up(attr) if attr is not None else None
        self.mol_trips = up(self.triplets)
        self._stage = None  # _RING x (pinned int64 buffer, event of the last copy out of it), made on first use
        self._slot = 0
        self._debug_fill = None  # tests: (int, float) sentinels written over every output before the launch

    def __len__(self):
        return int(self.nodes.shape[0])

    # ------------------------------------------------------------------------------------------ one batch
    def _indices(self, indices):
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        M = len(self)
        bad = (idx < -M) | (idx >= M)
        if bad.any():
            raise IndexError(f"molecule index {int(idx[bad][0])} out of range for a dataset of {M}")
        return np.where(idx < 0, idx + M, idx)

    def _upload(self, block):
        """The offset block on the device: through a pinned staging slot, non-blocking.  The ring's slot is
        rewritten only once the copy last issued from it has finished (an event; _RING batches later it has).
        Under graph capture no event is waited for or recorded (neither is legal there); the captured copy reads
        the slot when the graph is replayed, so such a graph replays the batch only until the ring comes round."""
        n = int(block.shape[0])
        capturing = torch.cuda.is_current_stream_capturing()
        if self._stage is None or self._stage[0][0].shape[0] < n:
            # every slot at once, so that a warmed-up caller allocates nothing later (e.g. under graph capture)
            self._stage = [(torch.empty(max(n, 1024), dtype=torch.int64, pin_memory=True), torch.cuda.Event())
                           for _ in range(_RING)]
        slot = self._stage[self._slot]
        if not capturing:
            slot[1].synchronize()  # (returns at once for an event never recorded)
        self._slot = (self._slot + 1) % _RING
        slot[0][:n].numpy()[:] = block
        dev = torch.empty(n, dtype=torch.int64, device=self.device)
        dev.copy_(slot[0][:n], non_blocking=True)
        if not capturing:
            slot[1].record(torch.cuda.current_stream(self.device))
        return dev

    def _assemble(self, idx, atoms_only=False):
        """Launch x2g_batch_assemble for the (validated) molecule indices; returns the outputs by name and the
        per-molecule host sizes.  ``atoms_only``: the atom and molecule outputs alone (no edges)."""
        from ._lib import call, ptr, stream_ptr

        B = int(idx.shape[0])
        nodes = self.nodes[idx]
        edges = np.zeros(B, np.int64) if atoms_only else self.edges[idx]
        N, E = int(nodes.sum()), int(edges.sum())
        block = np.empty(5 * B + 2, np.int64)
        block[:B] = self.atom_start[idx]
        block[B:2 * B] = self.edge_start[idx]
        block[2 * B:3 * B] = idx
        block[3 * B] = 0
        np.cumsum(nodes, out=block[3 * B + 1:4 * B + 1])
        block[4 * B + 1] = 0
        np.cumsum(edges, out=block[4 * B + 2:])
        dev = self.device
        F = 0 if atoms_only else self.num_features
        # fresh per call (the eager step's autograd holds on to a batch past the next one): one allocation per
        # dtype, the outputs are views of it; edge_attr on its own (16-byte aligned whatever E and N are)
        i64 = torch.empty(2 * N + (B + 1) + 2 * E + 2 * B, dtype=torch.int64, device=dev)
        i32 = torch.empty(4 * E + N + 2 * (B + 1), dtype=torch.int32, device=dev)
        f32 = torch.empty(3 * N + B, dtype=torch.float32, device=dev)
        attr = torch.empty((E, F), dtype=torch.float32, device=dev) if F else None
        if self._debug_fill is not None:
            i64.fill_(self._debug_fill[0])
            i32.fill_(self._debug_fill[0])
            f32.fill_(self._debug_fill[1])
            if attr is not None:
                attr.fill_(self._debug_fill[1])
        x, batch, p, ei, edge_num, trips = torch.split(i64, [N, N, B + 1, 2 * E, B, B])
        src, dst, src_t, dst_t, atom_t, mol_ptr, line_ptr = torch.split(i32, [E, E, E, E, N, B + 1, B + 1])
        pos, y = torch.split(f32, [3 * N, B])
        off = self._upload(block)
        wide = self.y.dim() == 2  # K targets per molecule: the kernel gathers no y (both pointers NULL)
        call("x2g_batch_assemble", ptr(self.x), ptr(self.atom_pos), ptr(self.edge_index),
             int(self.edge_index.shape[1]), ptr(self.edge_attr) if F else None, F, None if wide else ptr(self.y),
             ptr(self.mol_trips), ptr(off), B, N, E, ptr(x), ptr(pos), ptr(batch), ptr(p), ptr(ei), ptr(attr),
             ptr(edge_num), None if wide else ptr(y), ptr(src), ptr(dst), ptr(src_t), ptr(dst_t), ptr(atom_t),
             ptr(mol_ptr), ptr(line_ptr), ptr(trips), stream_ptr(dev))
        if wide:  # the molecule ids are the offset block's third run
            y = self.y.index_select(0, off[2 * B:3 * B])
        out = {"x": x, "atom_pos": pos.view(N, 3), "edge_index": ei.view(2, E), "edge_attr": attr,
               "edge_num": edge_num, "y": y, "batch": batch, "ptr": p, "_x2g_edge_src": src, "_x2g_edge_dst": dst,
               "_x2g_mol_ptr": mol_ptr, "_x2g_line_ptr": line_ptr, "_x2g_dst_type": dst_t, "_x2g_src_type": src_t,
               "_x2g_atom_type": atom_t, "_x2g_mol_trips": trips}
        return out, nodes, edges

    def batch(self, indices) -> Batch:
        """The collated batch of molecules ``indices`` (any sequence, any order, repeats allowed) on the device.
        An index outside the dataset raises IndexError before anything is launched."""
        idx = self._indices(indices)
        if idx.shape[0] == 0:
            raise ValueError("a batch needs at least one molecule")
        out, nodes, edges = self._assemble(idx)
        b = Batch()
        object.__setattr__(b, "_meta", {"nodes": nodes, "edges": edges, "triplets": self.triplets[idx]})
        st = b._store
        for k in ("x", "atom_pos", "edge_index", "edge_attr", "edge_num", "y", "batch", "ptr", "_x2g_edge_src",
                  "_x2g_edge_dst", "_x2g_mol_ptr", "_x2g_line_ptr", "_x2g_dst_type", "_x2g_src_type",
                  "_x2g_atom_type"):  # (data.collate's keys, in its order)
            if out[k] is not None:
                st[k] = out[k]
        st["_x2g_symmetric"] = bool(self.symmetric[idx].all())
        st["_x2g_mol_trips"] = out["_x2g_mol_trips"]
        st["_x2g_max_mol_atoms"] = int(nodes.max())
        st["_x2g_max_degree"] = int(self.max_degree[idx].max())
        st["_x2g_device_schedule"] = True  # GraphPlan.from_atom_batch: ops.center_schedule, no O(N) host work
        return b

    def shard_batch(self, indices, world: int, rank: int):
        """This rank's share of the global batch ``indices`` (``dist.collate_shard``'s device counterpart):
        (local Batch, local molecule count, global molecule count), the shard from ``dist.shard_by_triplets``
        over the cached triplet counts, the local batch carrying the global batch's atomic numbers
        (``_x2g_count_z``: gathered by the same kernel's atom path)."""
        from .dist import shard_by_triplets

        idx = self._indices(indices)
        mine = shard_by_triplets(self.triplets[idx], world)[rank]
        b = self.batch(idx[mine])
        b._store["_x2g_count_z"] = self._assemble(idx, atoms_only=True)[0]["x"]
        return b, len(mine), int(idx.shape[0])

    # ------------------------------------------------------------------------------------------ training order
    def reordered(self, order):
        """A new dataset holding the molecules ``order`` (indices into this one; any sequence, repeats and
        subsets allowed), in that order: what ``DeviceDataset([mols[i] for i in order], device)`` builds, caches
        included, made once from host prefix sums and one device ``index_select`` per tensor (no host copy of the
        data and no recount of the triplets; while it runs both datasets' ``edge_attr`` are resident).

        The reference permutes the dataset once and cuts its three splits from the permutation, unshuffled
        (trainer.py:23-27), so every batch of every epoch is the same run of the permuted order:
        ``ds.reordered(perm)`` stores the dataset in that order, every batch of ``loader(B, shuffle=False,
        indices=split)`` is then a contiguous run of molecules, and its ``edge_attr`` rows one contiguous slab
        ``edge_attr[edge_start[i]:edge_start[i + B]]`` of the dataset."""
        idx = self._indices(order)
        new = type(self).__new__(type(self))
        new.device = self.device
        new.nodes, new.edges = self.nodes[idx], self.edges[idx]
        new.triplets, new.max_degree, new.symmetric = self.triplets[idx], self.max_degree[idx], self.symmetric[idx]
        new.atom_start = np.concatenate([[0], np.cumsum(new.nodes)]).astype(np.int64)
        new.edge_start = np.concatenate([[0], np.cumsum(new.edges)]).astype(np.int64)
        new.num_features = self.num_features

        def gather(start, new_start, counts):
            # source row of every new row: the molecule's old start carried over its rows, plus the row's offset
            g = np.repeat(start[idx] - new_start[:-1], counts) + np.arange(int(new_start[-1]), dtype=np.int64)
            return torch.from_numpy(g).to(self.device)

        atoms = gather(self.atom_start, new.atom_start, new.nodes)
        rows = gather(self.edge_start, new.edge_start, new.edges)
        mols = torch.from_numpy(idx).to(self.device)
        new.x, new.atom_pos = self.x.index_select(0, atoms), self.atom_pos.index_select(0, atoms)
        new.edge_index = self.edge_index.index_select(1, rows)
        new.edge_attr = self.edge_attr.index_select(0, rows) if self.edge_attr is not None else None
        new.y, new.mol_trips = self.y.index_select(0, mols), self.mol_trips.index_select(0, mols)
        new._stage, new._slot, new._debug_fill = None, 0, None
        return new

    # ------------------------------------------------------------------------------------------ fixed shape
    def capacity(self, index_lists, fillers=1) -> Capacity:
        """The one shape (:class:`x2gnn.padding.Capacity`) every batch of ``index_lists`` can be padded to by
        ``fillers`` filler molecules (:func:`x2gnn.padding.filler_plan`), from the cached per-molecule sizes
        (nothing touches the device).  Every list must have the same length; the molecules must all be symmetric
        (the padded path is the molecular center-kernel path); ValueError otherwise, and where no shape within
        the fillers' reach exists."""
        from . import ops

        lists = [self._indices(i) for i in index_lists]
        if not lists or lists[0].shape[0] == 0:
            raise ValueError("capacity needs at least one non-empty index list")
        if any(i.shape[0] != lists[0].shape[0] for i in lists):
            raise ValueError("every index list of a capacity must have the same length (drop or step the ragged "
                             "last batch of an epoch on its own)")
        pool = np.unique(np.concatenate(lists))
        if not bool(self.symmetric[pool].all()):
            raise ValueError("the padded path takes symmetric molecules only (every edge with its reverse, none twice)")
        # (no filler molecule above ops.MOL_ROWPTR_MAX_ATOMS atoms, the per-molecule line-graph builder's bound)
        return solve_capacity([self.nodes[i].sum() for i in lists], [self.edges[i].sum() for i in lists],
                              [self.triplets[i].sum() for i in lists], int(self.max_degree[pool].max()), int(fillers),
                              int(lists[0].shape[0]), int(self.nodes[pool].max()), ops.MOL_ROWPTR_MAX_ATOMS)

    # ------------------------------------------------------------------------------------------ one epoch
    def loader(self, batch_size, shuffle=True, seed=0, drop_last=False, indices=None):
        """An iterable over one epoch of batches: a host permutation (seeded numpy generator) of ``indices``
        (default: every molecule; e.g. a train / validation split), cut into ``batch_size`` pieces."""
        return _Epoch(self, int(batch_size), shuffle, seed, drop_last, indices)


class _Epoch:
    def __init__(self, ds, batch_size, shuffle, seed, drop_last, indices):
        if batch_size < 1:
            raise ValueError("batch_size must be positive")
        pool = np.arange(len(ds), dtype=np.int64) if indices is None else ds._indices(indices)
        self.order = np.random.default_rng(seed).permutation(pool) if shuffle else pool
        self.ds, self.batch_size, self.drop_last = ds, batch_size, drop_last

    def index_lists(self):
        """The epoch's batches as index arrays (what ``__iter__`` assembles)."""
        n, bs = len(self.order), self.batch_size
        stop = n - n % bs if self.drop_last else n
        return [self.order[i:i + bs] for i in range(0, stop, bs)]

    def __len__(self):
        n, bs = len(self.order), self.batch_size
        return n // bs if self.drop_last else (n + bs - 1) // bs

    def __iter__(self):
        for idx in self.index_lists():
            yield self.ds.batch(idx)
