"""Device operators of the hot path: thin wrappers over libx2g.so + their autograd rules.

Every function here runs on the GPU through the C ABI (include/x2g.h) on PyTorch's current
stream; inputs must be CUDA (HIP) tensors.  There is deliberately no CPU fallback.

Operator                     replaces (reference / un-vendored dependency)
---------------------------  ----------------------------------------------------------------
``vertex_to_edge``           edge_graph.vertex_to_edge_2 (edge_graph.py:12-30), scipy on CPU
``bessel_env`` /             F_B_2D.forward (angular_basis_layer.py:80-93) + poly_envelop
``spherical_basis``          (envelop.py:16-21) + the angle code of xgnn.py:61-65
``sbf_attention``            SBFTransformerConv.propagate/message/softmax/aggregate + skip
                             (sbftransformer_conv.py:99-162; PyG MessagePassing, utils.softmax)
``segment_sum``              torch_scatter.scatter_add with a sorted index (readout.py:37,
                             model.py:190) and its backward gather
``segment_softmax``          torch_geometric.utils.softmax
``graph_layer_norm``         torch_geometric.nn.LayerNorm(mode='graph') (model.py:161,183)
"""
from __future__ import annotations

import contextlib
import ctypes
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from .data import CENTER_SF_MAX_ROWS

_C = _lib.CONSTS  # the #defines of include/x2g.h, by name without the X2G_ prefix
EDGE_NONE, EDGE_PER_TRIPLET, EDGE_PER_DST = _C["EDGE_NONE"], _C["EDGE_PER_TRIPLET"], _C["EDGE_PER_DST"]


def rows_fit(rows, width):
    """True when a [rows, width] fp32 array is addressable by the kernels' 32-bit BYTE offsets
    (buffer-resource loads / stores: num_records is a byte count below 2^31)."""
    return int(rows) * int(width) * 4 < 2 ** 31


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("x2gnn device ops need GPU tensors (no CPU fallback by design)")


def _f32(t):
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.to(torch.float32).contiguous()


def _i32(t):
    return t if t.dtype == torch.int32 and t.is_contiguous() else t.to(torch.int32).contiguous()


# ---------------------------------------------------------------------------------- line graph
MOL_ROWPTR_MAX_ATOMS = 16384  # x2g_vertex_to_edge_sym_mol's per-molecule degree histogram (64 KB of LDS)


class LineGraph:
    """Triplet structure of one collated batch (all int32, on the device).

    trip_rowptr/trip_src/trip_dst: CSR by destination line node, in the reference's order.
    atom_i/atom_j/atom_k: the three atoms of each triplet (xgnn.py:52 edge_i/edge_j/edge_k).
    src_rowptr/src_perm: the same triplets grouped by source line node (built on first use).
    """

    def __init__(self, edge_src, edge_dst, num_nodes, num_triplets, symmetric=False, with_transpose=None,
                 molecules=None):
        """``with_transpose`` (default: symmetric and grad enabled, i.e. a backward will ask for
        ``src_csr``): build the by-source lists with the line graph (x2g_line_graph_sym_build,
        three launches for both instead of five).  ``molecules`` = (mol_ptr int32 [B+1], line_ptr int32
        [B+1], triplets per molecule int64 [B], largest molecule's atom count) of a symmetric batch whose
        edges stay inside their molecules: the row pointers one workgroup per molecule
        (x2g_vertex_to_edge_sym_mol, two launches), the transpose left to ``src_csr`` (the center-atom
        backward never reads it)."""
        self.symmetric = bool(symmetric)  # caller-asserted: b->a present for every a->b (x2g_*_sym)
        if molecules is not None and (not self.symmetric or int(molecules[3]) > MOL_ROWPTR_MAX_ATOMS
                                      or int(molecules[2].shape[0]) < 1):
            molecules = None
        if with_transpose is None:
            with_transpose = self.symmetric and torch.is_grad_enabled() and molecules is None
        self.E = int(edge_src.shape[0])
        self.N = int(num_nodes)
        self.T = int(num_triplets)
        self.edge_src, self.edge_dst = edge_src, edge_dst
        dev = edge_src.device
        i32 = dict(dtype=torch.int32, device=dev)
        self.atom_rowptr = torch.empty(self.N + 1, **i32)
        self.trip_rowptr = torch.empty(self.E + 1, **i32)
        self.trip_src = torch.empty(self.T, **i32)
        self.trip_dst = torch.empty(self.T, **i32)
        self.atom_j = torch.empty(self.T, **i32)
        self.atom_i = torch.empty(self.T, **i32)
        self.atom_k = torch.empty(self.T, **i32)
        self._declare_optional()
        self.order_status = None  # built here in order: nothing to check
        ws_bytes = int(_lib.load().x2g_vertex_to_edge_workspace(self.E, self.N))
        self._ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        if self.symmetric:  # (written by the same emission grid)
            self.edge_rev, self.rev_trip = torch.empty(self.E, **i32), torch.empty(self.E, **i32)
        if molecules is not None:
            mol_ptr, line_ptr, trips, max_atoms = molecules
            call("x2g_vertex_to_edge_sym_mol", ptr(edge_src), ptr(edge_dst), self.E, self.N, self.T, ptr(mol_ptr),
                 ptr(line_ptr), ptr(trips), int(trips.shape[0]), int(max_atoms), ptr(self.atom_rowptr),
                 ptr(self.trip_rowptr), ptr(self.trip_src), ptr(self.trip_dst), ptr(self.atom_j), ptr(self.atom_i),
                 ptr(self.atom_k), ptr(self.edge_rev), ptr(self.rev_trip), stream_ptr())
            return
        if with_transpose and self.symmetric:
            self._src_rowptr = torch.empty(self.E + 1, **i32)
            self._src_perm = torch.empty(self.T, **i32)
            self._src_dst = torch.empty(self.T, **i32)
            call("x2g_line_graph_sym_build", ptr(edge_src), ptr(edge_dst), self.E, self.N, self.T,
                 ptr(self.atom_rowptr), ptr(self.trip_rowptr), ptr(self.trip_src), ptr(self.trip_dst),
                 ptr(self.atom_j), ptr(self.atom_i), ptr(self.atom_k), ptr(self._src_rowptr), ptr(self._src_perm),
                 ptr(self._src_dst), ptr(self.edge_rev), ptr(self.rev_trip), ptr(self._ws), ws_bytes, stream_ptr())
            return
        if self.symmetric:
            call("x2g_vertex_to_edge_sym", ptr(edge_src), ptr(edge_dst), self.E, self.N, self.T, ptr(self.atom_rowptr),
                 ptr(self.trip_rowptr), ptr(self.trip_src), ptr(self.trip_dst), ptr(self.atom_j), ptr(self.atom_i),
                 ptr(self.atom_k), ptr(self.edge_rev), ptr(self.rev_trip), ptr(self._ws), ws_bytes, stream_ptr())
            return
        call("x2g_vertex_to_edge", ptr(edge_src), ptr(edge_dst), self.E, self.N, self.T, ptr(self.atom_rowptr),
             ptr(self.trip_rowptr), ptr(self.trip_src), ptr(self.trip_dst), ptr(self.atom_j), ptr(self.atom_i),
             ptr(self.atom_k), ptr(self._ws), ws_bytes, stream_ptr())

    def _declare_optional(self):
        """Every field a line graph may go without, at its empty value (the constructors, GraphPlan, collate's
        schedules and spherical_basis fill them in)."""
        self._src_rowptr = self._src_perm = self._src_dst = None  # the by-source lists (src_csr)
        # per-line-node element rows of the x2g_vertex_to_edge line graph (GraphPlan sets them):
        # dst_type[e] = Z of e's destination atom = the edge row of every triplet into e, and
        # src_type[s] = Z of s's source atom = the same row for every triplet out of s
        self.dst_type = self.src_type = None
        # per-line-node atom rows of a per-atom edge table (SBFTransformerV2; GraphPlan sets them to the line
        # graph's own edge_dst / edge_src): dst_atom[e] = e's destination atom = the table row of every triplet
        # into e, src_atom[s] = s's source atom = the same row for every triplet out of s
        self.dst_atom = self.src_atom = None
        self._atom_pack_info = None  # pack_info with the atom itself as its edge-table row (atom_pack_info)
        # degree bound of the center atoms (host metadata; set by GraphPlan, None = unknown) and each atom's
        # element row (int32 [N]: the key of the center-atom edge-term gradient)
        self.max_degree = None
        self.atom_type = None
        # symmetric graphs: each edge's reverse and where its triplet block starts, for the center-atom
        # attention kernels
        self.edge_rev = self.rev_trip = None
        # the center kernels' workgroups (collate's; None: the identity): int32 [N] the atoms by decreasing
        # degree (one per workgroup), and the fused forward's packs (data.center_packs): int32 [N] the atoms
        # unit by unit, int32 [P + 1] the units' bounds in it, the largest row count of the units after the
        # first center_hubs (single atoms of more rows than the fused forward's LDS image holds: the tiled form)
        self.center_order = self.pack_order = self.center_packs = self.center_rows = self.pack_info = None
        self.center_hubs = 0
        self.center_mixed = False  # the schedule is x2g_center_schedule's (hub units among the packs)
        # spherical_basis' factors (sbf, rbf_env, Y[T, 8]) and the arguments of its unwritten lazy rows
        self.sbf_factors = self.sbf_pending = None
        # host counts per molecule (line nodes, triplets[, atoms]: GraphPlan) and _infer_tiles' lists by tile size
        self.mol_counts = None
        self._infer_tile_cache = {}

    @classmethod
    def from_triplets(cls, triplet_index, num_line_nodes: int):
        """Wrap an existing triplet index [2, T] whose row 1 is sorted ascending (as vertex_to_edge_2
        emits it).  Nothing is read back: the order is checked on the device and a violation is
        flagged in ``order_status`` (int32 [1]; see ``order_violated``), the row pointer staying in
        range either way."""
        lg = cls.__new__(cls)
        lg.E, lg.N, lg.T = int(num_line_nodes), None, int(triplet_index.shape[1])
        lg.edge_src = lg.edge_dst = lg.atom_rowptr = None
        lg.atom_i = lg.atom_j = lg.atom_k = None
        lg.trip_src = _i32(triplet_index[0])
        lg.trip_dst = _i32(triplet_index[1])
        lg.trip_rowptr, lg.order_status = csr_rowptr_checked(lg.trip_dst, lg.E)
        lg.symmetric = False
        lg._declare_optional()
        ws_bytes = int(_lib.load().x2g_vertex_to_edge_workspace(lg.E, 0))
        lg._ws = torch.empty(ws_bytes, dtype=torch.uint8, device=lg.trip_src.device)
        return lg

    def atom_pack_info(self):
        """``pack_info`` for a per-atom edge table: its fourth column, the edge-table row of the atom's first
        out-edge (the element row collate and x2g_center_schedule fill in), is the atom's own index (column 0).
        None without a ``pack_info``."""
        if self._atom_pack_info is None and self.pack_info is not None:
            info = self.pack_info.view(-1, 4).clone()
            info[:, 3] = info[:, 0]
            self._atom_pack_info = info.view(-1)
        return self._atom_pack_info

    def src_csr(self):
        """(src_rowptr [E+1], src_perm [T]): the triplets grouped by source line node; ``src_dst``
        [T] (each source-major position's destination) is built with them."""
        if self._src_rowptr is None:
            dev = self.trip_src.device
            self._src_rowptr = torch.empty(self.E + 1, dtype=torch.int32, device=dev)
            self._src_perm = torch.empty(self.T, dtype=torch.int32, device=dev)
            self._src_dst = torch.empty(self.T, dtype=torch.int32, device=dev)
            if self.symmetric:  # lists written in order from the degrees (no atomics, no segment sort)
                call("x2g_line_graph_transpose_sym", ptr(self.edge_src), ptr(self.edge_dst), ptr(self.atom_rowptr),
                     ptr(self.trip_rowptr), self.E, ptr(self._src_rowptr), ptr(self._src_perm), ptr(self._src_dst),
                     ptr(self._ws), self._ws.numel(), stream_ptr())
            else:
                call("x2g_line_graph_transpose", ptr(self.trip_src), ptr(self.trip_dst), self.T, self.E,
                     ptr(self._src_rowptr), ptr(self._src_perm), ptr(self._src_dst), ptr(self._ws),
                     self._ws.numel(), stream_ptr())
        return self._src_rowptr, self._src_perm

    @property
    def src_dst(self):
        self.src_csr()
        return self._src_dst

    def order_violated(self) -> bool:
        """True when the triplet destinations handed to ``from_triplets`` were not sorted (one sync)."""
        return self.order_status is not None and bool(self.order_status.item())

    def triplet_index(self):
        """int64 [2, T] (row 0 = source line node id(b->k), row 1 = destination id(a->b))."""
        return torch.stack([self.trip_src.long(), self.trip_dst.long()])


def vertex_to_edge(edge_index, num_nodes: int, num_triplets: int, symmetric: bool = False) -> LineGraph:
    """Build the line graph of a (src, dst)-sorted directed edge list on the device
    (``symmetric``: the caller asserts b->a exists for every a->b)."""
    _need_cuda(edge_index)
    ei = _i32(edge_index)
    return LineGraph(ei[0].contiguous(), ei[1].contiguous(), num_nodes, num_triplets, symmetric)


def csr_rowptr(sorted_keys, num_segments: int):
    _need_cuda(sorted_keys)
    keys = _i32(sorted_keys)
    out = torch.empty(num_segments + 1, dtype=torch.int32, device=keys.device)
    call("x2g_csr_rowptr", ptr(keys), keys.numel(), num_segments, ptr(out), stream_ptr())
    return out


def csr_rowptr_checked(keys, num_segments: int):
    """(rowptr [num_segments + 1], status int32 [1]) for keys assumed sorted and in range: no host
    read; status is 1 on the device when the assumption fails (x2g_csr_rowptr_checked)."""
    _need_cuda(keys)
    k = _i32(keys.reshape(-1))
    out = torch.empty(num_segments + 1, dtype=torch.int32, device=k.device)
    status = torch.empty(1, dtype=torch.int32, device=k.device)
    call("x2g_csr_rowptr_checked", ptr(k), k.numel(), num_segments, ptr(out), ptr(status), stream_ptr())
    return out, status


# ---------------------------------------------------------------------------------- basis
def bessel_env(dist, cutoff: float = 5.0, num_spherical: int = 7, num_radial: int = 6):
    """[E] distances -> [E, num_spherical * num_radial] env(d) * N_ln j_l(z_ln d / cutoff)."""
    _need_cuda(dist)
    d = _f32(dist)
    out = torch.empty(d.shape[0], num_spherical * num_radial, dtype=torch.float32, device=d.device)
    call("x2g_bessel_env", ptr(d), d.shape[0], float(cutoff), num_spherical, num_radial, ptr(out), stream_ptr())
    return out


class _EdgeBasis(torch.autograd.Function):
    """dist, env, rbf_env = sin(freq * d / cutoff) * env, bessel_env in one kernel
    (x2g_edge_basis); the backward gives the RadialBasis.frequencies gradient."""

    @staticmethod
    def forward(ctx, freq, pos, lg, cutoff, nsph, nrad):
        E, R = lg.E, freq.shape[0]
        f32 = dict(dtype=torch.float32, device=pos.device)
        dist, env = torch.empty(E, **f32), torch.empty(E, **f32)
        rbf, bes = torch.empty(E, R, **f32), torch.empty(E, nsph * nrad, **f32)
        call("x2g_edge_basis", ptr(_f32(pos)), ptr(lg.edge_src), ptr(lg.edge_dst), E, float(cutoff), ptr(_f32(freq)), R,
             nsph, nrad, ptr(dist), ptr(env), ptr(rbf), ptr(bes), stream_ptr())
        ctx.save_for_backward(dist, env, freq)
        ctx.freq_param = freq  # the Parameter object itself (grad_sink looks at its attributes)
        ctx.cutoff = float(cutoff)
        ctx.mark_non_differentiable(dist, env, bes)
        ctx.set_materialize_grads(False)
        return dist, env, rbf, bes

    @staticmethod
    def backward(ctx, _gd, _ge, grbf, _gb):
        if grbf is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        dist, env, freq = ctx.saved_tensors
        E, R = dist.shape[0], freq.shape[0]
        lib = _lib.load()
        dest = _WGradDest([ctx.freq_param], dist.device)
        (dfreq,) = dest.bufs
        ws_bytes = int(lib.x2g_edge_basis_freq_grad_workspace(E, R))
        call("x2g_edge_basis_freq_grad", ptr(_f32(grbf)), ptr(dist), ptr(env), ptr(freq), E, R, ctx.cutoff, ptr(dfreq),
             dest.flags(E), ptr(dest.workspace(ws_bytes)), ws_bytes, stream_ptr())
        if dest.deferral:
            dest.queue((0, int(lib.x2g_edge_basis_freq_grad_splits(E)), R, 0, dfreq, None))
        return (*dest.grads(), None, None, None, None, None)


def edge_basis(pos, lg: LineGraph, freq, cutoff: float = 5.0, num_spherical: int = 7, num_radial: int = 6):
    """(dist [E], env [E], rbf_env [E, R] = sin(freq d / cutoff) env, bessel_env [E, num_spherical *
    num_radial]) for the line graph's directed edges; rbf_env carries the gradient to ``freq``
    (xgnn.py:49-53,66-70)."""
    _need_cuda(pos, freq)
    return _EdgeBasis.apply(freq, pos, lg, cutoff, int(num_spherical), int(num_radial))


def spherical_basis(pos, lg: LineGraph, rbf_env, want_cos=False, num_spherical: int = 7, num_radial: int = 6,
                    lazy=False):
    """[T, S] sbf = rbf_env[src] * Y_l0(theta) (S = num_spherical * num_radial, l-major), theta from
    the triplet's atom positions.

    When gradients are being recorded the two factors are kept on the line graph
    (``lg.sbf_factors = (sbf, rbf_env, Y[T, 8])``): the attention backward then folds lin_sbf's
    weight gradient per source line node instead of materialising d(lin_sbf(sbf)) [T, D]
    (csrc/attention_fold.inc)."""
    _need_cuda(pos, rbf_env)
    pos = _f32(pos)
    rbf_env = _f32(rbf_env)
    S = num_spherical * num_radial
    out = torch.empty(lg.T, S, dtype=torch.float32, device=pos.device)
    cos_t = torch.empty(lg.T, dtype=torch.float32, device=pos.device) if want_cos else None
    # the factors are kept for the factorised backward and for the fused-projection center forward (which
    # also runs without grad, in inference: its source-tiled form takes every degree up to the center kernels'
    # bound)
    sf_fits = lg.max_degree is not None and lg.max_degree <= CENTER_MAX_DEGREE
    fold = _FOLD_SBF and (num_spherical, num_radial) == FOLD_BASIS and (torch.is_grad_enabled() or sf_fits)
    ylm = torch.empty(lg.T, 8, dtype=torch.float32, device=pos.device) if fold else None
    # lazy (the model's own forward): only the factors are written; the [T, S] rows are filled by
    # materialize_sbf when a consumer reads them (the fused center forward never does: 586 MB per step at
    # config 5, 33 MB at config 2)
    lazy = lazy and fold and not want_cos
    call("x2g_spherical_basis", ptr(pos), ptr(lg.atom_i), ptr(lg.atom_j), ptr(lg.atom_k), None, ptr(lg.trip_src),
         ptr(rbf_env), lg.T, num_spherical, num_radial, None if lazy else ptr(out), ptr(cos_t), ptr(ylm),
         stream_ptr())
    lg.sbf_factors = (out, rbf_env, ylm) if ylm is not None else None
    lg.sbf_pending = (out, pos, rbf_env, num_spherical, num_radial) if lazy else None
    return (out, cos_t) if want_cos else out


# The model's own forward asks spherical_basis for the factors only (lazy sbf rows): False = always write
# the [T, S] rows (a constant: bench.py --no-lazy-sbf and the parity tests flip it).
LAZY_SBF = True


def materialize_sbf(lg, sbf):
    """Fill the [T, S] sbf rows a lazy spherical_basis left unwritten, if ``sbf`` is them (every consumer that
    reads sbf values, rather than its factors, calls this first)."""
    pend = lg.sbf_pending
    if pend is None or pend[0] is not sbf:
        return sbf
    out, pos, rbf_env, ns, nr = pend
    call("x2g_spherical_basis", ptr(pos), ptr(lg.atom_i), ptr(lg.atom_j), ptr(lg.atom_k), None, ptr(lg.trip_src),
         ptr(rbf_env), lg.T, ns, nr, ptr(out), None, None, stream_ptr())
    lg.sbf_pending = None
    return sbf


def spherical_basis_from_angles(theta, trip_src, rbf_env, num_spherical: int = 7, num_radial: int = 6):
    """[T, S] sbf = rbf_env[trip_src] * Y_l0(theta) for given angles (F_B_2D signature)."""
    _need_cuda(theta, trip_src, rbf_env)
    th = _f32(theta)
    src = _i32(trip_src)
    out = torch.empty(th.shape[0], num_spherical * num_radial, dtype=torch.float32, device=th.device)
    call("x2g_spherical_basis", None, None, None, None, ptr(th), ptr(src), ptr(_f32(rbf_env)), th.shape[0],
         num_spherical, num_radial, ptr(out), None, None, stream_ptr())
    return out


# ---------------------------------------------------------------------------------- attention
FOLD_BASIS = (7, 6)  # the (num_spherical, num_radial) the folded kernels are compiled for (sbf_dim 42)
CENTER_MAX_DEGREE = _C["CENTER_MAX_DEGREE"]
# the source-tiled forward's dropout instances hold at most 4 destinations per owner (x2g_staged.h)
DROPOUT_TILED_MAX_DEGREE = 64

# The module switches are constants, not environment reads: each exists because a parity test flips it to check
# the shipped path against the plain one (paths measured slower and without such a test are deleted).
# _attention_route reads them at every call.
#   switch        False selects                                                        flipped by
#   _LN_FUSE      no per-row (mean, M2) statistics from the attention forward for the  test_fused_variants_
#                 row chain's fused graph LayerNorm (x2g_chain_fwd_ln): the separate   equal_separate
#                 LayerNorm kernels after the conv (model.py:46)
#   _LN_BWD_ROWS  the two-pass LayerNorm backward instead of per-molecule sums from    the same test
#                 the chain backward's per-row sums (x2g_graph_layernorm_bwd_rows)
#   _SRC_G        g_t = d loss / d a_t [T, H] written by the destination pass and      the same test
#                 read by the folded source pass, which otherwise recomputes it
#   _FOLD_SBF     spherical_basis keeps no factors, so no route has them: the plain    test_factorised_sbf_
#                 backward + [T, D] d_sbfproj + T-row weight GEMM (the drop-in conv    backward_equals_two_pass
#                 API takes it anyway: its sbf is any [T, 42] tensor)
#   _CENTER       the destination-major kernels everywhere                             test_operator_routes
#   _CENTER_BWD   the center forward with the destination-major backward passes        test_gpu_attention_route.py
#   _CENTER_SF    S projected first and read (x2g_sbf_project + x2g_sbf_attention_     test_gpu_attention_route.py
#                 fwd_center) instead of rebuilt from the sbf factors per center atom
#   _CENTER_P     the fused forward hands the center backward every S row (T x 512 B)  test_operator_routes
#                 instead of each source's P rows (E x 3.5 KB), from which the
#                 backward rebuilds S_t = b + sum_l Y_l(t) P_s[l] bit for bit
#   _PACK_FWD     one atom per workgroup in the fused forward instead of collate's     test_gpu_attention_route.py
#                 packs (16 owners per workgroup keep 90 % instead of 57 % of them
#                 busy).  The backward is always one atom per workgroup: packed, its
#                 phase barriers waited for the longest member (4 % slower, profiles/r5k_*)
#   INFER_TILE    (a size, below) without grad and with more triplets than this, the   test_inference_tiled_
#                 S-reading forward runs tile by tile                                  projection_equals_whole
_LN_FUSE = True
_LN_BWD_ROWS = True
_SRC_G = True
_FOLD_SBF = True
_CENTER = True
_CENTER_BWD = True
_CENTER_SF = True
_CENTER_P = True
_PACK_FWD = True


def _center_split(lg):
    """(order, pack_ptr, info, launches): the fused forward's units and the launches that cover them, each
    (entry, unit0, n_units, rows, skip_rows): with collate's packs the first ``center_hubs`` units (single
    atoms of more than CENTER_SF_MAX_ROWS rows, by decreasing degree) take the source-tiled form and the rest
    (at most ``center_rows`` rows each) the untiled one; with a device-made schedule (x2g_center_schedule:
    hubs among the packs) both forms run over all units, each leaving out the other's (skip_rows / max_rows);
    without either (unpacked) every atom is a unit by decreasing degree, all of them tiled when any exceeds
    the bound."""
    sf, tiled = "x2g_sbf_attention_fwd_center_sf", "x2g_sbf_attention_fwd_center_sf_tiled"
    packs = lg.center_packs
    if not _PACK_FWD or packs is None or lg.pack_order is None or lg.center_rows is None:
        rows = max(int(lg.max_degree), 1)
        if rows > CENTER_SF_MAX_ROWS:
            return lg.center_order, None, None, [(tiled, 0, lg.N, lg.max_degree, 0)]
        return lg.center_order, None, None, [(sf, 0, lg.N, rows, 0)]
    units, rows = int(packs.shape[0]) - 1, max(int(lg.center_rows), 1)
    if lg.center_mixed:
        launches = [(sf, 0, units, CENTER_SF_MAX_ROWS, 0)]
        if lg.max_degree > CENTER_SF_MAX_ROWS:
            launches.insert(0, (tiled, 0, units, lg.max_degree, CENTER_SF_MAX_ROWS))
    else:
        hubs = int(lg.center_hubs or 0)
        launches = [(tiled, 0, hubs, lg.max_degree, 0)] if hubs else []
        if units > hubs:
            launches.append((sf, hubs, units - hubs, rows, 0))
    return lg.pack_order, packs, lg.pack_info, launches


def center_schedule(atom_rowptr, src_row, num_atoms: int):
    """The center kernels' schedule made on the device (x2g_center_schedule): (center_order [N], pack_order [N],
    pack_ptr [N + 1], atom_info [N * 4]) — the same kind data.center_packs makes on the host (best fit per
    window of 64 atoms, the units by decreasing largest degree); its hub units lead the packs, which the
    launches find on the device (LineGraph.center_mixed)."""
    n = int(num_atoms)
    dev = atom_rowptr.device
    off = 4 * ((3 * n + 1 + 3) // 4)  # atom_info 16-byte aligned after the order / pack order / pack_ptr
    buf = torch.empty(off + 4 * n, dtype=torch.int32, device=dev)
    c_order, p_order, p_ptr = torch.split(buf[:3 * n + 1], [n, n, n + 1])
    info = buf[off:off + 4 * n]
    lib = _lib.load()
    ws_b = int(lib.x2g_center_schedule_workspace(n))
    ws = torch.empty(ws_b, dtype=torch.uint8, device=dev)
    call("x2g_center_schedule", ptr(atom_rowptr), ptr(src_row), n, ptr(c_order), ptr(p_order), ptr(p_ptr),
         ptr(info), ptr(ws), ws_b, stream_ptr())
    return c_order, p_order, p_ptr, info


def _center_launch(launches, common, outs, drop=()):
    """``drop``: (p, key pointer, salt) — the launches take the staged dropout entries (x2g_staged.h)."""
    for entry, u0, n, rows, skip in launches:
        name = entry + "_drop" if drop else entry
        if entry.endswith("_tiled"):
            call(name, *common, u0, n, rows, skip, *outs, *drop)
        else:
            call(name, *common, u0, n, rows, *outs, *drop)


def _unit_rows_lds(rows):  # csrc/attention_center.hip unit_rows_lds
    return ((3 * rows + 2 * 32 + 4) * 4 + 15) // 16 * 16


def _center_sf_split(lg, factors, D):
    """_center_split(lg) when the fused-projection center forward applies, else None: the sbf factors are this
    call's and every untiled launch's LDS image fits (the units of more rows than the untiled form's bound take
    its source-tiled form)."""
    if not (_CENTER_SF and factors is not None and factors[1] is not None and D == 128 and lg.max_degree is not None):
        return None
    split = _center_split(lg)
    fits = all(e.endswith("_tiled") or _unit_rows_lds(r) + 4776 * r <= 160 * 1024 for e, _, _, r, _ in split[3])
    return split if fits else None


def _center_sf_ok(lg, factors, D):
    """Whether the fused-projection center forward applies (_center_sf_split)."""
    return _center_sf_split(lg, factors, D) is not None


def _center_bwd_ok(lg, heads, s_rows=False):
    """Whether the center-atom backward takes this line graph (its element rows known, the LDS image of the
    largest atom's block within 160 KB, and its T-row arrays within the kernel's 32-bit buffer offsets:
    the S rows T x 512 B when ``s_rows``, else the P-row form's (g, a) scratch T x heads x 8 B)."""
    row_bytes = 128 * 4 if s_rows else heads * 8
    return (_CENTER_BWD and getattr(lg, "atom_type", None) is not None and lg.max_degree is not None and
            lg.T * row_bytes < 2 ** 31 and
            _lib.load().x2g_sbf_attention_bwd_center_lds(lg.max_degree, heads) <= 160 * 1024)


def _center_rows(lg, edge_mode, edge_row, D, channels):
    """(ok, src_row): whether the center-atom forward applies to this call, and the per-source edge-table
    row it reads for EDGE_PER_DST (the center atom's element: lg.src_type, valid when the caller's
    per-destination rows are the line graph's own dst_type; the center atom itself, lg.src_atom, for a per-atom
    table whose per-destination rows are lg.dst_atom)."""
    if (not _CENTER or lg.edge_rev is None or lg.max_degree is None
            or lg.max_degree > CENTER_MAX_DEGREE or D != 128 or channels % 4 or edge_mode == EDGE_PER_TRIPLET):
        return False, None
    if edge_mode == EDGE_PER_DST:
        if _atom_table(lg, edge_row):
            return True, lg.src_atom
        if edge_row is None or lg.src_type is None or edge_row is not lg.dst_type:
            return False, None
        return True, lg.src_type
    return True, None


def _atom_table(lg, edge_row):
    """Whether ``edge_row`` addresses a per-atom edge table: the line graph's own (dst_atom, src_atom) pair."""
    return (edge_row is not None and getattr(lg, "src_atom", None) is not None
            and edge_row is getattr(lg, "dst_atom", None))


class _Route(NamedTuple):
    """Which attention kernels one sbf_attention call runs and what its forward keeps (_attention_route)."""
    factors: Optional[tuple]  # (radial [E, 42], Y [T, 8]) when sbf is their product and the folded kernels take it
    src_row: object  # the center kernels' per-source edge-table row (EDGE_PER_DST), else None
    forward: str  # "fused" (lin_sbf inside the center forward) | "center" | "dst" (both read S rows)
    order: object  # fused: _center_split's units ...
    packs: object
    info: object
    launches: Optional[list]  # ... and the launches that cover them
    tiles: Optional[list]  # the S-reading forward's inference tiles (_infer_tiles); None: all rows at once
    backward: Optional[str]  # None (no backward follows) | "center_p" | "center_s" | "dst_fold" | "dst_plain"
    alpha: bool  # the forward writes the logits [T, H]
    sproj: bool  # ... the S rows [T, D] (tiled: one tile's)
    sbf_p: bool  # ... the sources' P rows [E, 7, D]
    rstats: bool  # ... the per-row (mean, M2) of the output, for a graph LayerNorm fused into the next row chain
    reads_sbf: bool  # the sbf rows themselves are read (materialize_sbf), not only their factors
    dropout_refusal: Optional[str]  # with dropout: None when this route has the staged dropout entries, else why not
    atom_table: bool = False  # the edge table has one row per atom (lg.dst_atom / lg.src_atom), not per element


def _attention_route(lg, edge_mode, edge_rows, edge_row, heads, channels, own_sbf, sbf_dim, keeps, keep_alpha,
                     dropout, grad_enabled):
    """The one decision of which kernels an sbf_attention call runs, from the line graph, the call's shape and the
    switches in the table above as they stand now (nothing is cached: tests flip a switch between two calls).
    ``edge_rows``: the edge table's row count (None without one); ``own_sbf``: sbf is lg.sbf_factors' product;
    ``keeps``: a backward will follow; ``keep_alpha``: the caller wants the logits; ``dropout``: it is set.

    Forward: the fused center forward where the center kernels take the call (_center_rows), the factors are the
    call's and the launches fit (_center_sf_split); else S = lin_sbf(sbf) is projected once per layer, right before
    the attention kernel reads its rows, by the center forward or else the destination-major one — tile by tile
    without grad beyond INFER_TILE triplets.  Backward: without factors the plain destination-major passes;
    with them the center backward from the fused forward's P rows, else from S rows, else the destination-major
    fold passes.  The logits are stored for a caller who wants them and for every backward but the P-row one,
    which recomputes them from rows it stages (the center forwards skip the store otherwise: 223 MB per layer
    in config 5's inference, 12 MB written and read back per layer in config 2's training)."""
    D = heads * channels
    center, src_row = _center_rows(lg, edge_mode, edge_row, D, channels)
    # a per-atom table: more than 16 rows, which only the fold passes refuse (the folded source pass stages the
    # per-destination edge table in LDS), so it has the factors where the center kernels run both ways (the S-row
    # backward's bound is the tighter of the two: asked once, either center backward may then follow), and else
    # none: the plain two-pass backward
    atom_table = edge_mode == EDGE_PER_DST and _atom_table(lg, edge_row)
    wide = edge_mode == EDGE_PER_DST and (edge_row is None or edge_rows is None or edge_rows > 16)
    if wide and atom_table and center and (not keeps or _center_bwd_ok(lg, heads, s_rows=True)):
        wide = False
    factors = None
    if (own_sbf and edge_mode != EDGE_PER_TRIPLET and D in (32, 64, 128) and sbf_dim == FOLD_BASIS[0] * FOLD_BASIS[1]
            and not wide):
        factors = lg.sbf_factors[1], lg.sbf_factors[2]
    split = _center_sf_split(lg, factors, D) if center else None
    if split is not None and atom_table and split[2] is not None:
        split = (split[0], split[1], lg.atom_pack_info(), split[3])  # (the atom as its own edge-table row)
    fused = split is not None
    backward = None
    if keeps and factors is None:
        backward = "dst_plain"
    elif keeps and fused and _CENTER_P and _center_bwd_ok(lg, heads):
        backward = "center_p"
    elif keeps:
        backward = "center_s" if center and _center_bwd_ok(lg, heads, s_rows=True) else "dst_fold"
    refusal = None
    if dropout:
        refusal = _dropout_refusal(lg, edge_mode, D, channels, center, factors, fused, keeps and backward != "center_p")
    tiles = None
    if not (fused or dropout or grad_enabled) and lg.T > INFER_TILE and lg.E > 0:
        tiles = _infer_tiles(lg, INFER_TILE)
        # whole molecules: a tile's atoms own exactly its triplets, so the center forward can take it
        center = center and all(t[4] is not None for t in tiles)
    return _Route(factors, src_row, "fused" if fused else "center" if center else "dst", *(split or (None,) * 4),
                  tiles, backward, alpha=keep_alpha or not center or (keeps and backward != "center_p"),
                  sproj=not fused or backward in ("center_s", "dst_fold"), sbf_p=backward == "center_p",
                  rstats=_LN_FUSE and D == 128, reads_sbf=not fused, dropout_refusal=refusal, atom_table=atom_table)


def _dropout_refusal(lg, edge_mode, D, channels, center, factors, fused, no_p_backward):
    """Attention dropout runs on one route only, the fused center forward and the P-row center backward: None
    for it, else the first condition that fails."""
    if not (_CENTER and _CENTER_SF and _CENTER_P):
        return "the center kernels are switched off (ops._CENTER / _CENTER_SF / _CENTER_P)"
    if edge_mode == EDGE_PER_TRIPLET:
        return "per-triplet edge_attr (the center kernels take no edge term or one row per destination, edge_row)"
    if lg.edge_rev is None or lg.max_degree is None:
        return "a line graph that is not symmetric (no edge_rev / rev_trip: not built by vertex_to_edge)"
    if lg.max_degree > CENTER_MAX_DEGREE:
        return f"a degree above CENTER_MAX_DEGREE ({lg.max_degree} > {CENTER_MAX_DEGREE})"
    if D != 128 or channels % 4:
        return f"heads * channels = {D} (compiled: 128, channels a multiple of 4)"
    if lg.max_degree > DROPOUT_TILED_MAX_DEGREE:
        return (f"a degree above {DROPOUT_TILED_MAX_DEGREE} ({lg.max_degree}): the source-tiled forward has no "
                "dropout instance for it")
    if not center:
        return ("edge_row is not the line graph's own destination elements (dst_type) or, for a per-atom table, "
                "destination atoms (dst_atom)")
    if factors is None or factors[1] is None:
        return "the sbf factors are absent (sbf is not the line graph's own radial x angular product)"
    if not fused:
        return "a unit beyond the fused center forward's LDS image"
    if no_p_backward:
        return ("the P-row center backward does not take this line graph (atom_type absent, T * heads * 8 >= 2^31, or "
                "the largest block's LDS image above 160 KiB)")
    return None


def _off(t, nbytes):
    return None if t is None else t.data_ptr() + nbytes


def _attention_forward(route, q, k, v, skip, edge, sbf, w_sbf, b_sbf, lg, edge_mode, edge_row, heads, channels,
                       drop=()):
    """The route's forward launches: (the fp32 operands a backward saves, (out, alpha, smax, sden, rstats), the
    S rows, the P rows).  ``drop``: _center_launch's."""
    q, k, v, skip = _f32(q), _f32(k), _f32(v), _f32(skip)
    sbf, w_sbf, b_sbf = _f32(sbf), _f32(w_sbf), _f32(b_sbf)
    edge = _f32(edge) if edge is not None else None
    E, T, D, H = q.shape[0], lg.T, heads * channels, heads
    f32 = dict(dtype=torch.float32, device=q.device)
    out = torch.empty(E, D, **f32)
    alpha = torch.empty(T, H, **f32) if route.alpha else None
    smax, sden = torch.empty(E, H, **f32), torch.empty(E, H, **f32)
    rstats = torch.empty(E, 2, **f32) if route.rstats else None
    sproj = sbf_p = None
    st = stream_ptr()
    if route.reads_sbf:
        materialize_sbf(lg, sbf)
    if route.forward == "fused":
        if route.sbf_p:
            sbf_p = torch.empty(E, 7, D, **f32)
        elif route.sproj:
            sproj = torch.empty(T, D, **f32)
        common = (ptr(q), ptr(k), ptr(v), ptr(skip), ptr(edge), ptr(route.src_row), edge_mode, ptr(route.factors[0]),
                  ptr(route.factors[1]), ptr(w_sbf), ptr(b_sbf), ptr(lg.atom_rowptr), ptr(lg.edge_rev),
                  ptr(lg.rev_trip), ptr(route.order), ptr(route.packs), ptr(route.info))
        outs = (E, T, heads, channels, ptr(out), ptr(alpha), ptr(smax), ptr(sden), ptr(rstats), ptr(sproj),
                ptr(sbf_p), st)
        _center_launch(route.launches, common, outs, drop)
        return (q, k, v, edge, sbf, b_sbf), (out, alpha, smax, sden, rstats), sproj, sbf_p
    # S = lin_sbf(sbf) [T, D] (or one tile's rows of it) right before the attention kernel reads them (so they
    # are still in the MALL: sbf pointer = S, weight pointer NULL) instead of re-projecting per triplet
    whole = route.tiles is None
    tiles = [(0, E, 0, T, (0, lg.N))] if whole else route.tiles
    sproj = torch.empty(max(t[3] - (t[2] & ~1) for t in tiles), D, **f32)
    fb, ib = 4, 4  # bytes per float32 / int32 element
    for e0, e1, t0, t1, atoms in tiles:
        ta = t0 & ~1  # from an even row: the projection's fast path wants 16-byte aligned sbf blocks
        call("x2g_sbf_project", _off(sbf, ta * sbf.shape[1] * fb), t1 - ta, sbf.shape[1], ptr(w_sbf), ptr(b_sbf), D,
             ptr(sproj), st)
        if route.forward == "center":  # the tile's atoms own exactly its triplets (S rows t - ta)
            call("x2g_sbf_attention_fwd_center", ptr(q), ptr(k), ptr(v), ptr(skip), ptr(edge), ptr(route.src_row),
                 edge_mode, ptr(sproj), ta, ptr(lg.atom_rowptr), ptr(lg.edge_rev), ptr(lg.rev_trip),
                 ptr(lg.center_order) if whole else None, atoms[0], atoms[1] - atoms[0], lg.max_degree, E, T, heads,
                 channels, ptr(out), ptr(alpha), ptr(smax), ptr(sden), ptr(rstats), st)
            continue
        # the kernel reads S at absolute triplet indices t in [t0, t1): hand it the base S - ta rows;
        # everything per destination edge is offset by e0, everything per triplet / per source edge
        # is indexed absolutely (edge: a table under edge_row, else one row per destination edge)
        e_edge = _off(edge, e0 * D * fb) if edge_mode == EDGE_PER_DST and edge_row is None else ptr(edge)
        e_row = _off(edge_row, e0 * ib) if whole or edge_mode == EDGE_PER_DST else None
        call("x2g_sbf_attention_fwd_stats" if rstats is not None else "x2g_sbf_attention_fwd",
             _off(q, e0 * D * fb), ptr(k), ptr(v), _off(skip, e0 * D * fb), e_edge, e_row, edge_mode,
             _off(sproj, -ta * D * fb), None, None, _off(lg.trip_rowptr, e0 * ib), ptr(lg.trip_src), e1 - e0, T, heads,
             channels, D, _off(out, e0 * D * fb), ptr(alpha), _off(smax, e0 * H * fb), _off(sden, e0 * H * fb),
             *((_off(rstats, e0 * 2 * fb),) if rstats is not None else ()), st)
    return (q, k, v, edge, sbf, b_sbf), (out, alpha, smax, sden, rstats), sproj, sbf_p


class _SBFAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, skip, edge, sbf, w_sbf, b_sbf, lg, edge_mode, edge_row, heads, channels, route,
                dropout=None):
        # its gradient is read only by the table chain's backward, which flushes deferred sums first
        pending = getattr(edge, "_x2g_keyed_pending", None)
        ctx.defer_edge = _DEFER_KEYED and pending is not None and ctx.needs_input_grad[4]
        ctx.keyed_pending = pending
        # attention dropout (p, key int64 [2] on the device, salt): the staged entries; the backward regenerates
        # the mask from the key saved here
        drop, drop_key = (), None
        if dropout is not None:
            drop_key = dropout[1]
            drop = (float(dropout[0]), ptr(drop_key), int(dropout[2]))
        ctx.dropout = None if dropout is None else (drop[0], drop[2])
        (q, k, v, edge, sbf, b_f32), outs, sproj, sbf_p = _attention_forward(
            route, q, k, v, skip, edge, sbf, w_sbf, b_sbf, lg, edge_mode, edge_row, heads, channels, drop)
        out, alpha, smax, sden, rstats = outs
        if route.factors is not None:  # the factorised backward never reads sbf itself
            ctx.save_for_backward(q, k, v, edge, *route.factors, sproj, alpha, smax, sden, sbf_p,
                                  b_f32 if sbf_p is not None else None, drop_key)
        else:
            ctx.save_for_backward(q, k, v, edge, sbf, None, sproj, alpha, smax, sden, None, None, None)
        ctx.route = route
        ctx.w_param, ctx.b_param = w_sbf, b_sbf
        ctx.lg, ctx.edge_mode, ctx.edge_row, ctx.heads, ctx.channels = lg, edge_mode, edge_row, heads, channels
        ctx.edge_shape = None if edge is None else edge.shape
        # (one call: a second mark_non_differentiable replaces the first's set)
        ctx.mark_non_differentiable(*(t for t in (alpha, smax, sden, rstats) if t is not None))
        # the logits / max / denominator outputs never receive gradients: do not let autograd
        # materialise zero-filled [T, H] / [E, H] tensors for them (three fill launches per layer)
        ctx.set_materialize_grads(False)
        return out, alpha, smax, sden, rstats

    @staticmethod
    def backward(ctx, dout, _da=None, _dm=None, _ds=None, _dr=None):
        # (with factors, the saved sbf is the radial factor rbf_env [E, 42])
        q, k, v, edge, sbf, ylm, sproj, alpha, smax, sden, sbf_p, b_sbf, drop_key = ctx.saved_tensors
        lg, mode, heads, channels, form = ctx.lg, ctx.edge_mode, ctx.heads, ctx.channels, ctx.route.backward
        dout = _f32(dout)
        E, T, D = q.shape[0], lg.T, heads * channels
        f32 = dict(dtype=torch.float32, device=q.device)
        dq, dk, dv = torch.empty(E, D, **f32), torch.empty(E, D, **f32), torch.empty(E, D, **f32)
        st = stream_ptr()
        if form == "dst_plain":
            dlogit = torch.empty(T, heads, **f32)
            dproj = torch.empty(T, D, **f32)
            rows = {EDGE_PER_TRIPLET: T, EDGE_PER_DST: E}.get(mode)  # the edge term's gradient: per triplet / destination
            d_edge = None if rows is None else torch.empty(rows, D, **f32)
            call("x2g_sbf_attention_bwd_dst", ptr(q), ptr(k), ptr(v), ptr(edge), ptr(ctx.edge_row), mode, ptr(sproj),
                 None, None, ptr(lg.trip_rowptr), ptr(lg.trip_src), ptr(alpha), ptr(smax), ptr(sden), ptr(dout), E, T,
                 heads, channels, D, ptr(dq), ptr(d_edge), ptr(dlogit), ptr(dproj), st)
            src_rowptr, src_perm = lg.src_csr()
            call("x2g_sbf_attention_bwd_src", ptr(q), ptr(sproj), None, None, ptr(src_rowptr), ptr(src_perm),
                 ptr(lg.trip_dst), ptr(alpha), ptr(smax), ptr(sden), ptr(dlogit), ptr(dout), E, T, heads, channels, D,
                 ptr(dk), ptr(dv), st)
            if not ctx.needs_input_grad[4]:
                d_edge = None
            elif mode == EDGE_PER_DST and ctx.route.atom_table:
                # a per-atom table: the destinations' gradients summed by target atom, each segment in row
                # order (x2g_segment_reduce_perm)
                d_edge = scatter_add(d_edge, ctx.edge_row, ctx.edge_shape[0])
            elif mode == EDGE_PER_DST and ctx.edge_row is not None:
                # rows of the edge table are shared by many destinations: sum d_edge per table row
                d_edge = keyed_row_sum(d_edge, ctx.edge_row, ctx.edge_shape[0])
            materialize_sbf(lg, sbf)
            # lin_sbf's dW / db (None where summed into the gradient bucket)
            dw, db = linear_wgrad(dproj, sbf, w_param=ctx.w_param, b_param=ctx.b_param)
            return dq, dk, dv, dout, d_edge, None, dw, db, None, None, None, None, None, None, None
        gfold = torch.empty(E, 8, D, **f32)
        if form in ("center_p", "center_s"):
            # one launch for both passes, per center atom (csrc/attention_center.hip); the edge term's
            # gradient comes per center atom and is summed by the atoms' elements
            want_edge = mode == EDGE_PER_DST and ctx.needs_input_grad[4]
            d_edge = torch.empty(lg.N, D, **f32) if want_edge else None
            g_work = torch.empty(2, T, heads, **f32)
            # (with dropout: the forward's p, salt and key — the mask is regenerated, never stored)
            drop = () if ctx.dropout is None else (ctx.dropout[0], ptr(drop_key), ctx.dropout[1])
            call("x2g_sbf_attention_bwd_center_drop" if drop else "x2g_sbf_attention_bwd_center", ptr(q), ptr(k),
                 ptr(v), ptr(edge), ptr(ctx.route.src_row), mode, ptr(sproj), ptr(sbf_p), ptr(b_sbf), ptr(ylm),
                 ptr(lg.atom_rowptr), ptr(lg.edge_rev), ptr(lg.rev_trip), ptr(lg.center_order), ptr(alpha), ptr(smax),
                 ptr(sden), ptr(dout), lg.N, lg.max_degree, E, T, heads, channels, ptr(dq), ptr(dk), ptr(dv),
                 ptr(gfold), ptr(d_edge), ptr(g_work), st, *drop)
            key = None if ctx.route.atom_table else lg.atom_type  # (a per-atom table: d_edge is its gradient)
        else:  # "dst_fold"
            # g[T, H] (d loss / d a_t): the source pass recomputes it from rows it holds anyway (_SRC_G)
            g = None if _SRC_G else torch.empty(T, heads, **f32)
            prob = torch.empty(T, heads, **f32)
            rho = torch.empty(E, heads, **f32)
            d_edge = torch.empty(E, D, **f32) if mode == EDGE_PER_DST else None
            call("x2g_sbf_attention_bwd_dst_g", ptr(q), ptr(k), ptr(v), ptr(edge), ptr(ctx.edge_row), mode, ptr(sproj),
                 ptr(lg.trip_rowptr), ptr(lg.trip_src), ptr(alpha), ptr(smax), ptr(sden), ptr(dout), E, T, heads,
                 channels, ptr(dq), ptr(d_edge), ptr(g), ptr(prob), ptr(rho), st)
            src_rowptr, src_perm = lg.src_csr()
            rows = 0 if edge is None else edge.shape[0]
            # the edge row per SOURCE (constant over a source segment) when the rows are the line graph's
            # own destination elements
            src_row = lg.src_type if (ctx.edge_row is not None and ctx.edge_row is lg.dst_type) else None
            call("x2g_sbf_attention_bwd_src_fold", ptr(q), ptr(v), ptr(edge), ptr(ctx.edge_row), ptr(src_row), rows,
                 mode, ptr(sproj), ptr(ylm), ptr(src_rowptr), ptr(src_perm), ptr(lg.src_dst), ptr(lg.trip_dst),
                 ptr(prob), ptr(g), ptr(rho), ptr(dout), E, T, heads, channels, ptr(dk), ptr(dv), ptr(gfold), st)
            if not ctx.needs_input_grad[4]:
                d_edge = None  # (written by the kernel; no consumer: the table's gradient is not wanted)
            key = ctx.edge_row  # d_edge per destination: summed by the destinations' table rows, if it has them
        if d_edge is not None and key is not None:
            if ctx.defer_edge:
                d_edge = keyed_row_sum_deferred(d_edge, key, ctx.edge_shape[0], ctx.keyed_pending)
            else:
                d_edge = keyed_row_sum(d_edge, key, ctx.edge_shape[0])
        # lin_sbf's dW / db (None where summed into the gradient bucket)
        dw, db = sbf_radial_wgrad(gfold, sbf, ctx.w_param, ctx.b_param)
        return dq, dk, dv, dout, d_edge, None, dw, db, None, None, None, None, None, None, None


def sbf_radial_wgrad(gfold, radial, w_param=None, b_param=None):
    """(dW_sbf [D, 42], db_sbf [D]) from the source-folded gradient G [E, 8, D] and the radial
    factor rbf_env [E, 42] (x2g_sbf_radial_wgrad); (None, None) when lin_sbf's parameters are given and
    bucket-backed: summed into the bucket (_WGradDest)."""
    E, _, D = gfold.shape
    dest = _WGradDest([w_param, b_param], gfold.device, shapes=[(D, 42), (D,)])
    dw, db = dest.bufs
    lib = _lib.load()
    ws_bytes = int(lib.x2g_sbf_radial_wgrad_workspace(E, D))
    call("x2g_sbf_radial_wgrad", ptr(gfold), ptr(_f32(radial)), E, D, ptr(dw), ptr(db), dest.flags(E),
         ptr(dest.workspace(ws_bytes)), ws_bytes, stream_ptr())
    if dest.deferral:
        dest.queue((0, int(lib.x2g_sbf_radial_wgrad_splits(E)), D * 42, D, dw, db))
    return dest.grads()


class _EmbeddingTable(torch.autograd.Function):
    """Embedding rows per element with torch.embedding_renorm_ (in place) and the
    scale_grad_by_freq / padding_idx gradient rules, one launch each way (csrc/embedding.hip)."""

    @staticmethod
    def forward(ctx, weight, z, max_norm, padding_idx, scale_grad):
        V, D = weight.shape
        if weight.dtype != torch.float32 or not weight.is_contiguous():
            raise ValueError("embedding weight must be contiguous fp32")
        zz = z if z.dtype == torch.int64 and z.is_contiguous() else z.to(torch.int64).contiguous()
        table = torch.empty_like(weight)
        counts = torch.empty(V, dtype=torch.float32, device=weight.device)
        call("x2g_embedding_table", ptr(weight), ptr(zz), zz.numel(), V, D, float(max_norm or 0.0), ptr(counts),
             ptr(table), stream_ptr())
        ctx.save_for_backward(counts)
        ctx.w_param, ctx.pad, ctx.scale = weight, (-1 if padding_idx is None else int(padding_idx)), bool(scale_grad)
        return table

    @staticmethod
    def backward(ctx, g):
        (counts,) = ctx.saved_tensors
        V, D = counts.shape[0], g.shape[1]
        dest = _WGradDest([ctx.w_param], g.device)
        (dw,) = dest.bufs
        call("x2g_embedding_table_bwd", ptr(_f32(g)), ptr(counts) if ctx.scale else None, V, D, ctx.pad, ptr(dw),
             ACCUM_WGRAD if dest.acc else 0, stream_ptr())  # (no slabs: nothing to defer)
        return (*dest.grads(), None, None, None, None)


def embedding_table(weight, z, max_norm, padding_idx, scale_grad_by_freq):
    """Rows of ``weight`` per element (see _EmbeddingTable); renormalises the used rows in place."""
    _need_cuda(weight, z)
    return _EmbeddingTable.apply(weight, z, max_norm, padding_idx, scale_grad_by_freq)


DenseFwdGroup = _lib.STRUCTS["x2g_dense_fwd_group"]
DenseBwdGroup = _lib.STRUCTS["x2g_dense_bwd_group"]
HeadGroup = _lib.STRUCTS["x2g_head_group"]


def _dp(t):
    return t.data_ptr() if t is not None else None


class _ReadoutMLPs(torch.autograd.Function):
    """sum_g mlp_g(feat_g) for the trunk's readouts (readout.py:25-31,42 / 55-62,76, summed in
    model.py:41,50): every readout's Linear+SiLU, Linear+SiLU, Linear(D,1) run as three batched
    launches (blockIdx.y = readout) instead of three per readout, and the sum over readouts is
    fused into the last one; backward likewise (the weight-gradient slab sums deferred)."""

    @staticmethod
    def forward(ctx, G, pool, *args):
        feats, params = args[:G], args[G:]
        W1, B1, W2, B2, W3, B3 = (params[i::6] for i in range(6))
        R, D = feats[0].shape
        ctx.pool = pool
        dev = feats[0].device
        f32 = dict(dtype=torch.float32, device=dev)
        xs = [_f32(f) for f in feats]
        z1 = [torch.empty(R, D, **f32) for _ in range(G)]
        h2 = [torch.empty(R, D, **f32) for _ in range(G)]
        z2 = [torch.empty(R, D, **f32) for _ in range(G)]
        st = stream_ptr()
        ctx.chain = _readout_chain_ok(R, D, G, W1, B1, W2, B2)
        if ctx.chain:  # both hidden layers of every readout: one x2g_chain_fwd_batch launch
            grad = _keeps(ctx)  # inference: no transposed weights, no T-layout inputs
            tf = int(_lib.load().x2g_chain_t_floats(R, D))
            WT = torch.empty(G, 2, D, D, **f32) if grad else None
            in_t = torch.empty(G, 2, tf, **f32) if grad else None

            def wt(g, i):
                return WT[g, i].data_ptr() if grad else None

            # (as _ChainFn: the flat launch reads each readout's input rows row-major, no T plane 0)
            ctx.rm0 = WGRAD_X_ROWMAJOR and grad
            f0 = CHAIN_SILU | (CHAIN_IN0_ROWMAJOR if ctx.rm0 else 0)
            stages = [(ChainStage * 2)(ChainStage(_dp(W1[g]), _dp(B1[g]), _dp(z1[g]), None, wt(g, 0), f0),
                                       ChainStage(_dp(W2[g]), _dp(B2[g]), _dp(z2[g]), _dp(h2[g]), wt(g, 1), CHAIN_SILU))
                      for g in range(G)]
            jobs = (ChainFwdJob * G)(*[ChainFwdJob(_dp(xs[g]), None, ctypes.addressof(stages[g]),
                                                   in_t[g].data_ptr() if grad else None) for g in range(G)])
            call("x2g_chain_fwd_batch", jobs, G, 2, R, D, st)
            out = _heads_fwd(h2, W3, B3, G, R, D, pool, f32, st)
            if grad:
                ctx.save_for_backward(*h2, *z1, *z2, WT, in_t, *(xs if ctx.rm0 else ()))
            ctx.G, ctx.params = G, params
            return out
        h1 = [torch.empty(R, D, **f32) for _ in range(G)]
        for (src, w, b, y, z) in ((xs, W1, B1, h1, z1), (h1, W2, B2, h2, z2)):
            grp = (DenseFwdGroup * G)(*[DenseFwdGroup(_dp(src[g]), _dp(w[g]), _dp(b[g]), None, _dp(y[g]), _dp(z[g]))
                                        for g in range(G)])
            call("x2g_dense_fwd_batched", grp, G, R, D, D, ACT_SILU, st)
        out = _heads_fwd(h2, W3, B3, G, R, D, pool, f32, st)
        ctx.save_for_backward(*xs, *h1, *z1, *h2, *z2)
        ctx.G, ctx.params = G, params
        return out

    @staticmethod
    def backward(ctx, dout):
        G = ctx.G
        saved = ctx.saved_tensors
        if ctx.chain:
            h2, z1, z2 = (saved[i * G:(i + 1) * G] for i in range(3))
            WT, in_t = saved[3 * G], saved[3 * G + 1]
        else:
            xs, h1, z1, h2, z2 = (saved[i * G:(i + 1) * G] for i in range(5))
        W1, B1, W2, B2, W3, B3 = (ctx.params[i::6] for i in range(6))
        R, D = h2[0].shape
        dev = h2[0].device
        f32 = dict(dtype=torch.float32, device=dev)
        lib = _lib.load()
        st = stream_ptr()
        K = W3[0].shape[0]
        dout = _f32(dout.reshape(-1))
        # head: dh2_g = dout w3_g; dW3_g, db3_g
        dh2 = [torch.empty(R, D, **f32) for _ in range(G)]
        dest3 = _WGradDest(list(W3) + list(B3), dev)
        dw3, db3 = dest3.bufs[:G], dest3.bufs[G:]
        g3 = dest3.grads()
        if K > 1:  # the K-target heads (x2g_multi.h): dout [R or n_seg, K]
            seg_rowptr, n_seg = ctx.pool if ctx.pool is not None else (None, 0)
            ws_bytes = int(lib.x2g_readout_heads_k_bwd_workspace(R, D, K, G))
            hflags, ws = dest3.flags(R), dest3.workspace(ws_bytes)
            call("x2g_readout_heads_k_bwd", ptr(dout), ptr(seg_rowptr), n_seg, _ptrs(h2), _ptrs(W3), _ptrs(dh2),
                 _ptrs(dw3), _ptrs(db3), G, R, D, K, hflags, ptr(ws), ws_bytes, st)
            if dest3.deferral:  # readout g's slabs: splits x (K*D weights, then K biases) floats
                splits = int(lib.x2g_readout_heads_k_bwd_splits(R))
                dest3.queue(*[(g * splits * (K * D + K) * 4, splits, K * D, K, dw3[g], db3[g]) for g in range(G)])
            heads = None
        else:
            heads = (HeadGroup * G)(*[HeadGroup(_dp(h2[g]), _dp(W3[g]), None, _dp(dh2[g]), _dp(dw3[g]), _dp(db3[g]))
                                      for g in range(G)])
            ws_bytes = int(lib.x2g_readout_head_bwd_workspace(R, D, G))
            hflags, ws = dest3.flags(R), dest3.workspace(ws_bytes)
            if ctx.pool is not None:  # dout per molecule, broadcast to its rows inside the head kernel
                seg_rowptr, n_seg = ctx.pool
                call("x2g_readout_head_pool_bwd", ptr(dout), ptr(seg_rowptr), n_seg, heads, G, R, D, hflags, ptr(ws),
                     ws_bytes, st)
            else:
                call("x2g_readout_head_bwd", ptr(dout), heads, G, R, D, hflags, ptr(ws), ws_bytes, st)
            if dest3.deferral:  # readout g's slabs: splits x (D weights + 1 bias) floats, one readout after another
                splits = int(lib.x2g_readout_head_bwd_splits(R))
                dest3.queue(*[(g * splits * (D + 1) * 4, splits, D, 1, dw3[g], db3[g]) for g in range(G)])
        if ctx.chain:  # both hidden layers' data gradients in one launch; dW / db from the T layout
            dfeat = [torch.empty(R, D, **f32) for _ in range(G)]
            dz_t = torch.empty_like(in_t)
            stages = [(ChainBwdStage * 2)(ChainBwdStage(_dp(W1[g]), WT[g, 0].data_ptr(), _dp(z1[g]), None, CHAIN_SILU),
                                          ChainBwdStage(_dp(W2[g]), WT[g, 1].data_ptr(), _dp(z2[g]), None, CHAIN_SILU))
                      for g in range(G)]
            jobs = (ChainBwdJob * G)(*[ChainBwdJob(_dp(dh2[g]), None, ctypes.addressof(stages[g]), _dp(dfeat[g]), None,
                                                   dz_t[g].data_ptr()) for g in range(G)])
            call("x2g_chain_bwd_batch", jobs, G, 2, R, D, st)
            pg = []
            for g in range(G):
                dws, dbs = chain_wgrad(in_t[g], dz_t[g], R, [W1[g], W2[g]], [B1[g], B2[g]],
                                       x0=saved[3 * G + 2 + g] if ctx.rm0 else None)
                pg += [dws[0], dbs[0], dws[1], dbs[1], g3[g], g3[G + g]]
            return (None, None, *dfeat, *pg)
        grads = {}
        # layer 2 then layer 1: dz = dy * SiLU'(z), dx = dz W, dW / db
        dy = dh2
        for (layer, x_in, z, W, B) in ((2, h1, z2, W2, B2), (1, xs, z1, W1, B1)):
            dx = [torch.empty(R, D, **f32) for _ in range(G)]
            dest = _WGradDest(list(W) + list(B), dev)
            dw, db = dest.bufs[:G], dest.bufs[G:]
            grp = (DenseBwdGroup * G)(*[DenseBwdGroup(_dp(dy[g]), _dp(z[g]), _dp(x_in[g]), _dp(W[g]), _dp(dx[g]), None,
                                                      _dp(dw[g]), _dp(db[g])) for g in range(G)])
            wsz = int(lib.x2g_dense_bwd_workspace(R, D, D))
            call("x2g_dense_bwd_batched", grp, G, R, D, D, ACT_SILU, dest.flags(R), ptr(dest.workspace(wsz * G)),
                 wsz * G, st)
            if dest.deferral:  # readout g's slabs lead its own x2g_dense_bwd_workspace share
                splits = int(lib.x2g_dense_bwd_splits(R, D, D))
                dest.queue(*[(g * wsz, splits, D * D, D, dw[g], db[g]) for g in range(G)])
            grads[layer] = dest.grads()
            dy = dx
        dfeat = dy
        pg = []
        for g in range(G):
            pg += [grads[1][g], grads[1][G + g], grads[2][g], grads[2][G + g], g3[g], g3[G + g]]
        return (None, None, *dfeat, *pg)


def _ptrs(ts):
    """A host array of the tensors' device pointers (None -> NULL), as x2g_multi.h's entries take them."""
    return (ctypes.c_void_p * len(ts))(*[_dp(t) for t in ts])


def _heads_fwd(h2, W3, B3, G, R, D, pool, f32, st):
    """The readouts' last layers summed over readouts: Linear(D, 1) through x2g_readout_head_(pool_)fwd, a
    Linear(D, K) with K > 1 through x2g_readout_heads_k_fwd -> [R or n_seg, K]."""
    K = W3[0].shape[0]
    if K == 1:
        heads = (HeadGroup * G)(*[HeadGroup(_dp(h2[g]), _dp(W3[g]), _dp(B3[g]), None, None, None) for g in range(G)])
        return _head_fwd(heads, G, R, D, pool, f32, st)
    seg_rowptr, n_seg = pool if pool is not None else (None, 0)
    out = torch.empty(R if pool is None else n_seg, K, **f32)
    call("x2g_readout_heads_k_fwd", _ptrs(h2), _ptrs(W3), _ptrs(B3), G, R, D, K, ptr(seg_rowptr), n_seg, ptr(out), st)
    return out


def _head_fwd(heads, G, R, D, pool, f32, st):
    """sum_g head_g(h_g) -> [R, 1] per row, or [n_seg, 1] summed per segment of rows with the pool
    (x2g_readout_head_pool_fwd: the global add pool fused)."""
    if pool is None:
        out = torch.empty(R, 1, **f32)
        call("x2g_readout_head_fwd", heads, G, R, D, ptr(out), st)
        return out
    seg_rowptr, n_seg = pool
    out = torch.empty(n_seg, 1, **f32)
    call("x2g_readout_head_pool_fwd", heads, G, R, D, ptr(seg_rowptr), n_seg, ptr(out), st)
    return out


# the readouts' two hidden layers as one batched row-chain launch each way (x2g_chain_*_batch) where
# compiled; two batched dense launches each way otherwise
CHAIN_MAX_JOBS = _C["CHAIN_MAX_JOBS"]
ChainFwdJob = _lib.STRUCTS["x2g_chain_fwd_job"]
ChainBwdJob = _lib.STRUCTS["x2g_chain_bwd_job"]


def _readout_chain_ok(R, D, G, *weights):
    if not _CHAIN or D != 128 or not 1 <= G <= CHAIN_MAX_JOBS or not rows_fit(R, 128):
        return False
    for ws in weights:
        for w in ws:
            if w is not None and (w.dtype != torch.float32 or not w.is_contiguous() or w.data_ptr() % 16):
                return False
    return all(tuple(w.shape) == (128, 128) for ws in (weights[0], weights[2]) for w in ws)


def readout_mlps_supported(feats, mlps):
    """True when _ReadoutMLPs covers these readouts (same row count and width, the 3-layer
    Linear/SiLU/Linear/SiLU/Linear(D,K) MLP with biases, the same K <= 16 targets in every readout, G <= 8,
    compiled widths)."""
    from .layers import Linear as _Lin
    G = len(feats)
    if G < 1 or G > 8 or not all(f.is_cuda and f.dim() == 2 and f.shape == feats[0].shape for f in feats):
        return False
    R, D = feats[0].shape
    if D % 4 or D <= 8 or D > 128 or (D // 4) & (D // 4 - 1) or not rows_fit(R, 128):
        return False
    for m in mlps:
        mods = list(m)
        if len(mods) != 5 or not all(isinstance(mods[i], _Lin) for i in (0, 2, 4)):
            return False
        if not all(isinstance(mods[i], torch.nn.SiLU) for i in (1, 3)):
            return False
        if any(mods[i].bias is None for i in (0, 2, 4)):
            return False
        if tuple(mods[0].weight.shape) != (D, D) or tuple(mods[2].weight.shape) != (D, D):
            return False
        K = mods[4].weight.shape[0]
        if tuple(mods[4].weight.shape) != (K, D) or not 1 <= K <= HEADS_K_MAX_TARGETS:
            return False
        if K != list(mlps[0])[4].weight.shape[0]:
            return False
    return True


HEADS_K_MAX_TARGETS = 16  # x2g_readout_heads_k_max_targets()


def readout_mlps(feats, mlps, pool=None):
    """sum_g mlp_g(feats[g]) -> [R, K] (see _ReadoutMLPs; K = 1 for the single-target models); with
    ``pool = (seg_rowptr int32 [S+1], S)`` the rows' sums per segment -> [S, K] instead (the global add pool after AtomWise, model.py:53, fused into the
    head launch each way)."""
    params = []
    for m in mlps:
        mods = list(m)
        params += [mods[0].weight, mods[0].bias, mods[2].weight, mods[2].bias, mods[4].weight, mods[4].bias]
    if pool is not None:
        pool = (_i32(pool[0]), int(pool[1]))
    return _apply(_ReadoutMLPs, len(feats), pool, *feats, *params)


def keyed_row_sum(src, key, num_keys: int):
    """out[k] = sum of src rows r with key[r] == k (unsorted key): the gradient of table[key]."""
    _need_cuda(src, key)
    src = _f32(src)
    R, D = src.shape
    if num_keys > 16 or D % 4 or D > 256 or (D // 4) & (D // 4 - 1):  # outside the compiled kernel
        onehot = torch.nn.functional.one_hot(key.long(), num_keys).to(torch.float32)
        return linear_wgrad(src, onehot, bias=False)[0].t().contiguous()
    out = torch.empty(num_keys, D, dtype=torch.float32, device=src.device)
    ws_bytes = int(_lib.load().x2g_keyed_row_sum_workspace(R, D, num_keys))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=src.device)
    call("x2g_keyed_row_sum", ptr(src), ptr(_i32(key)), R, D, num_keys, ptr(out), 0, ptr(ws), ws_bytes, stream_ptr())
    return out


# Keyed row sums whose results are only read by the element-table chain's backward (every conv's
# per-destination edge gradient -> its lin_edge table rows): queued here and run as ONE batched
# launch (x2g_keyed_row_sum_batch) when _TableChainFn.backward starts, instead of a partial + a
# slab-sum launch per layer.  The queue belongs to the table chain's forward (one per model call,
# ``table_chain``), not to the module: two models, threads or streams never share it.  False sums
# each immediately.
_DEFER_KEYED = True
KEYED_MAX_JOBS = _C["KEYED_MAX_JOBS"]


def keyed_row_sum_deferred(src, key, num_keys: int, pending: list):
    """keyed_row_sum(src, key, num_keys) into a buffer filled when ``pending`` (the table chain's
    queue) is flushed by flush_keyed(pending)."""
    src = _f32(src)
    R, D = src.shape
    if R == 0 or num_keys > 16 or D % 4 or D > 256 or (D // 4) & (D // 4 - 1):
        return keyed_row_sum(src, key, num_keys)
    out = torch.empty(num_keys, D, dtype=torch.float32, device=src.device)
    pending.append((src, _i32(key), int(num_keys), out))
    return out


def flush_keyed(pending: list):
    """Run every keyed row sum queued on ``pending`` (one partial + one slab-sum launch per group
    of jobs that share keys and shape)."""
    if not pending:
        return
    items = list(pending)
    pending.clear()
    groups = {}
    for src, key, nk, out in items:
        groups.setdefault((key.data_ptr(), tuple(src.shape), nk), []).append((src, key, nk, out))
    lib = _lib.load()
    for (_, (R, D), nk), items in groups.items():
        for j0 in range(0, len(items), KEYED_MAX_JOBS):
            part = items[j0:j0 + KEYED_MAX_JOBS]
            n = len(part)
            srcs = (ctypes.c_void_p * n)(*[it[0].data_ptr() for it in part])
            outs = (ctypes.c_void_p * n)(*[it[3].data_ptr() for it in part])
            wsb = int(lib.x2g_keyed_row_sum_batch_workspace(R, D, nk, n))
            ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=part[0][0].device)
            call("x2g_keyed_row_sum_batch", srcs, outs, n, ptr(part[0][1]), R, D, nk, 0, ptr(ws), wsb, stream_ptr())


# Inference (grad mode off) with many triplets: S = lin_sbf(sbf) [T, D] is projected and consumed one
# range of destination edges at a time (whole destination segments, at most INFER_TILE triplets),
# so no more than [INFER_TILE, D] of it exists at once.  Sized for 288 GB of HBM: 2^24 triplets are an
# 8.6 GB tile, so config 5 (T = 3.49M, S 1.8 GB per layer) runs whole — one projection and one center
# forward per layer: 8.00 ms per step against 9.11 tiled at 2^19 (seven tiles, 14 launches per layer
# with their ramps and drains; profiles/r5ab_c5_tile.log) and 10.75 at 2^17 (round 4).
INFER_TILE = 1 << 24


def _infer_tiles(lg, tmax):
    """[(e0, e1, t0, t1, atoms)] destination-edge ranges of at most ``tmax`` triplets each (a longer
    segment gets a range of its own), cached on the line graph.  With the batch's per-molecule
    counts (``lg.mol_counts``, set by GraphPlan from host metadata) the ranges are whole molecules,
    found without touching the device, so a captured graph can be recorded from a fresh line
    graph (``atoms``: the range's atoms when the counts give them, else None); otherwise (the drop-in
    conv API) from the row pointer, read back once."""
    cache = lg._infer_tile_cache
    if tmax in cache:
        return cache[tmax]
    counts = lg.mol_counts
    ap = None
    if counts is not None:
        ec, tc = counts[0], counts[1]
        ep = np.concatenate([[0], np.cumsum(ec)])
        rp = np.concatenate([[0], np.cumsum(tc)])
        if len(counts) > 2:  # atoms per molecule: each tile's atom range too (center-atom kernels)
            ap = np.concatenate([[0], np.cumsum(counts[2])])
            if ap[-1] != lg.N:
                ap = None
        # the host metadata must describe this line graph, or a tile could split a destination
        # segment or run past E / T: otherwise take the row pointer itself (one read-back)
        if ep[-1] != lg.E or rp[-1] != lg.T or (np.asarray(ec) < 0).any() or (np.asarray(tc) < 0).any():
            counts = None
    if counts is None:
        rp = lg.trip_rowptr.cpu().numpy().astype("int64")
        ep = np.arange(lg.E + 1, dtype=np.int64)
        ap = None
    n = len(rp) - 1
    tiles, i = [], 0
    while i < n:
        j = int(np.searchsorted(rp, rp[i] + tmax, side="right")) - 1  # furthest j with rp[j] - rp[i] <= tmax
        j = min(max(j, i + 1), n)
        if ep[j] > ep[i]:
            atoms = (int(ap[i]), int(ap[j])) if ap is not None else None
            tiles.append((int(ep[i]), int(ep[j]), int(rp[i]), int(rp[j]), atoms))
        i = j
    cache[tmax] = tiles
    return tiles


def sbf_attention(q, k, v, skip, edge, sbf, w_sbf, b_sbf, lg: LineGraph, heads: int, channels: int,
                  edge_mode: int = EDGE_PER_TRIPLET, edge_row=None, return_attention=False, dropout=None):
    """Fused SBFTransformerConv message/softmax/aggregate/skip (see csrc/attention.hip).

    With ``return_attention`` also returns the softmax probabilities [T, heads] (the
    reference's ``return_attention_weights`` alpha: the softmax before dropout).

    ``dropout``: None or ``(p, key, salt)`` — attention dropout of probability ``p`` in [0, 1) with the
    counter-based mask of include/x2g_staged.h: ``key`` an int64 [2] device tensor (seed, step) that the caller
    does not change in place afterwards (the backward regenerates the forward's mask from it), ``salt`` the
    layer's index.  It runs on the fused center forward and the P-row center backward only; any other route
    raises NotImplementedError.  ``p == 0`` is no dropout: today's calls."""
    _need_cuda(q, k, v, skip, sbf)
    if dropout is not None:
        p_drop, key, salt = dropout
        if not 0.0 <= float(p_drop) < 1.0:
            raise ValueError(f"dropout probability {p_drop} outside [0, 1)")
        if float(p_drop) == 0.0:
            dropout = None
        elif not (torch.is_tensor(key) and key.is_cuda and key.dtype == torch.int64 and key.numel() == 2
                  and key.is_contiguous()):
            raise ValueError("dropout key: an int64 [2] device tensor (seed, step)")
        else:
            dropout = (float(p_drop), key, int(salt) & 0xFFFFFFFF)
    if edge is None:
        edge_mode = EDGE_NONE
    if edge_row is not None:
        edge_row = _i32(edge_row)
    grad = torch.is_grad_enabled()
    # (what _keeps answers inside the forward: autograd fills needs_input_grad from requires_grad alone)
    keeps = grad and any(t is not None and t.requires_grad for t in (q, k, v, skip, edge, sbf, w_sbf, b_sbf))
    route = _attention_route(lg, edge_mode, None if edge is None else edge.shape[0], edge_row, heads, channels,
                             lg.sbf_factors is not None and lg.sbf_factors[0] is sbf, sbf.shape[1], keeps,
                             return_attention, dropout is not None, grad)
    if route.dropout_refusal is not None:
        raise NotImplementedError("attention dropout is compiled for the center kernels only: "
                                  + route.dropout_refusal)
    if route.tiles is not None:  # (inference only: no autograd node)
        out, alpha, smax, sden, rstats = _attention_forward(route, q, k, v, skip, edge, sbf, w_sbf, b_sbf, lg, edge_mode,
                                                            edge_row, heads, channels)[1]
    else:
        out, alpha, smax, sden, rstats = _apply(_SBFAttention, q, k, v, skip, edge, sbf, w_sbf, b_sbf, lg, edge_mode,
                                                edge_row, heads, channels, route, dropout)
    if rstats is not None:  # for a graph LayerNorm fused into the consumer (ops.row_chain(ln=...))
        out._x2g_rowstats = rstats
    if not return_attention:
        return out
    dst = lg.trip_dst.long()
    prob = torch.exp(alpha - smax.index_select(0, dst)) / (sden.index_select(0, dst) + 1e-16)
    return out, prob


# ---------------------------------------------------------------------------------- dense layers
ACCUM_WGRAD, DEFER_SLAB_SUM, GATE_DRBF_ACCUM = _C["ACCUM_WGRAD"], _C["DEFER_SLAB_SUM"], _C["GATE_DRBF_ACCUM"]
SlabJob = _lib.STRUCTS["x2g_slab_job"]


class _SlabDeferral:
    """The state of one ``deferred_wgrad()`` context (one backward): the queued slab sums, the
    workspaces they read, the T-layout weight-gradient jobs of the flat launch, and — after the
    context exits — ``flat_launches``: [(rows, cols) per job] of each flat launch it made (bench.py's
    roofline probe replays the largest)."""

    def __init__(self):
        self.jobs = []
        self.keep = []  # workspaces holding the partial slabs until the batched sum is enqueued
        self.tiled = {}  # rows -> [TiledJob]: T-layout weight gradients run as one launch at exit
        self.flat_launches = []


# Open deferrals by HIP stream: autograd runs each backward node on its forward's stream, so a
# backward finds the context its caller opened on that stream, and two models stepping on two
# streams (or threads) never see each other's queue.
_DEFERRALS = {}


def _defer():
    """The deferral open on the current stream, or None."""
    if not _DEFERRALS:
        return None
    return _DEFERRALS.get(torch.cuda.current_stream().cuda_stream)


TILED_MAX_JOBS = _C["TILED_MAX_JOBS"]

# In-step kernel timing for bench.py's roofline line: while a name is a key here, an EAGER (not captured)
# pass appends (start, end) HIP events recorded around that kernel's launch on its stream.  A sleep kernel
# ahead of the start event keeps the device busy while the host enqueues the launch, so the events bracket
# the kernel alone, in the step's own cache state (its operands were just written by the same backward).
KERNEL_TIMERS = {}


@contextlib.contextmanager
def _timed(name):
    evs = KERNEL_TIMERS.get(name)
    if evs is None or torch.cuda.is_current_stream_capturing():
        yield
        return
    st = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    # ~0.1 ms of device time ahead of the start event while the host enqueues the launch.  (The eager
    # launch still runs 3-8 % slower than the same launch in graph-replayed steps, box-dependent; a longer
    # sleep or 0.2 ms of matrix work in its place did not change that: DESIGN.md section 5.)
    torch.cuda._sleep(200_000)
    a.record(st)
    yield
    b.record(st)
    evs.append((a, b))


# FLAT_SPLIT > 0: the queued T-layout weight gradients are launched as soon as that many are queued (the
# last layers' group mid-backward, the rest at exit) — the split an exchange overlap needs, so that the
# first group's gradients exist before the backward ends.  0: one flat launch at exit (the default).  A
# constant like the switches above (set explicitly by an A/B script or a test, never from the environment).
FLAT_SPLIT = 0


def _queue_tiled(d, R, jobs, keep):
    """Queue T-layout weight-gradient jobs (x2g_tiled_job, bucket-backed destinations) on deferral
    ``d`` for its flat launch; ``keep``: tensors the jobs point into."""
    d.tiled.setdefault(int(R), []).extend(jobs)
    d.keep.extend(keep)
    if FLAT_SPLIT > 0 and not d.flat_launches and sum(len(j) for j in d.tiled.values()) >= FLAT_SPLIT:
        _flush_tiled(d)


def _flush_tiled(d):
    """Every queued T-layout weight gradient, whatever its row count (the line-node rows of the trunk,
    the atom rows of the readout MLPs), in as few launches as X2G_TILED_MAX_JOBS allows: one at config 2
    (x2g_tiled_wgrad_flat_rows; one launch per row count before).  ``d.flat_launches`` records each
    launch as [(rows, cols) per job]."""
    lib = _lib.load()
    items = [(int(R), j) for R, jobs in d.tiled.items() for j in jobs]
    for j0 in range(0, len(items), TILED_MAX_JOBS):
        part = items[j0:j0 + TILED_MAX_JOBS]
        n = len(part)
        d.flat_launches.append([(R, int(j.cols) if j.ld > 0 else 128) for R, j in part])
        rows = (ctypes.c_int64 * n)(*[R for R, _ in part])
        ws_bytes = int(lib.x2g_tiled_wgrad_flat_rows_workspace(rows, n, 128))
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=torch.device("cuda", torch.cuda.current_device()))
        out = (SlabJob * n)()
        jobs = (TiledJob * n)(*[j for _, j in part])
        st = stream_ptr()
        with _timed("tiled_wgrad_flat"):  # (nothing but the launch between the timing events)
            call("x2g_tiled_wgrad_flat_rows", jobs, rows, n, 128, ACCUM_WGRAD | DEFER_SLAB_SUM, out, ptr(ws),
                 ws_bytes, st)
        d.jobs.extend(out)
        d.keep.append(ws)
    d.tiled = {}


@contextlib.contextmanager
def deferred_wgrad():
    """Within this context (on the current stream), weight gradients that go straight into a
    gradient bucket (``grad_sink``) leave their per-workgroup partial slabs in place and the
    T-layout ones are queued; on exit ONE flat weight-gradient launch and ONE x2g_slab_sum_batch
    launch finish every layer's (instead of small launches per layer).  Yields the deferral
    (``flat_launches`` is filled on exit)."""
    key = torch.cuda.current_stream().cuda_stream
    prev = _DEFERRALS.get(key)
    d = _DEFERRALS[key] = _SlabDeferral()
    try:
        yield d
        if d.tiled:
            _flush_tiled(d)
        if d.jobs:
            arr = (SlabJob * len(d.jobs))(*d.jobs)
            call("x2g_slab_sum_batch", ctypes.cast(arr, ctypes.c_void_p), len(d.jobs), 1, stream_ptr())
    finally:
        if prev is None:
            _DEFERRALS.pop(key, None)
        else:
            _DEFERRALS[key] = prev


_APPLY_GRAD = [True]  # the caller's grad mode at the innermost Function.apply in flight (_apply)


def _apply(fn, *args):
    """``fn.apply(*args)`` with the caller's grad mode recorded for the forward: autograd runs forward() with
    grad mode off and fills ``ctx.needs_input_grad`` from ``requires_grad`` alone, so under ``torch.no_grad()``
    every parameter still "needs" a gradient and a forward that asked only ``needs_input_grad`` kept its
    backward's operands for nothing (config 5's inference wrote ~0.7 GB of logits and P rows and the chains'
    T-layout inputs per layer)."""
    prev = _APPLY_GRAD[0]
    _APPLY_GRAD[0] = torch.is_grad_enabled()
    try:
        return fn.apply(*args)
    finally:
        _APPLY_GRAD[0] = prev


def _keeps(ctx):
    """Whether this forward keeps the operands of a backward: an input needs a gradient AND the caller's
    grad mode was on (see _apply)."""
    return _APPLY_GRAD[0] and any(ctx.needs_input_grad)


def grad_sink(param):
    """The parameter's gradient buffer when the kernels may accumulate into it directly.

    ``dist.GradBucket`` marks its parameters: their ``.grad`` is a view of one flat zeroed buffer,
    so a weight gradient can be summed straight into it by the slab-sum kernel (X2G_ACCUM_WGRAD)
    and the Function returns None for that input — autograd then launches no add kernel for it.
    Unmarked parameters (tests, plain ``loss.backward()``) get their gradient returned as usual."""
    if param is None or not getattr(param, "_x2g_grad_sink", False):
        return None
    g = param.grad
    if g is None or not g.is_contiguous() or g.dtype != torch.float32:
        return None
    return g


class _WGradDest:
    """Where the weight gradients of ONE launch go, and when their partial slabs are summed.

    ``params``: the launch's parameters, None for an absent bias (``shapes``: their shapes, for a caller
    that may have no parameter objects).  ``bufs`` holds per parameter the gradient-bucket view
    (``grad_sink``) when every present one is bucket-backed — the kernel then sums into the bucket
    (``acc``) and ``grads()``, what the Function returns for them, is all None — and otherwise a fresh
    fp32 buffer each, which ``grads()`` returns.  ``flags(rows)`` is the entry's flag word and
    ``workspace(n)`` its workspace; inside ``deferred_wgrad()`` the flag word leaves the slab sum to the
    context's one batched launch (``deferral`` is then set) and ``queue`` hands it the slabs."""

    def __init__(self, params, dev, shapes=None):
        if shapes is None:
            shapes = [None if p is None else p.shape for p in params]
        sinks = [None if sh is None else grad_sink(p) for p, sh in zip(params, shapes)]
        self.acc = all(s is not None for s, sh in zip(sinks, shapes) if sh is not None)
        self.bufs = sinks if self.acc else [None if sh is None else torch.empty(tuple(sh), dtype=torch.float32,
                                                                               device=dev) for sh in shapes]
        self.dev, self.deferral, self.ws = dev, None, None

    def flags(self, rows):
        """X2G_ACCUM_WGRAD when summing into the bucket, and with it X2G_DEFER_SLAB_SUM when a deferral is
        open on this stream and the launch has rows (the C entries refuse the flag at zero rows)."""
        self.deferral = _defer() if self.acc and rows > 0 else None
        return (ACCUM_WGRAD if self.acc else 0) | (DEFER_SLAB_SUM if self.deferral is not None else 0)

    def workspace(self, n, least=1):
        self.ws = torch.empty(max(int(n), least), dtype=torch.uint8, device=self.dev)
        return self.ws

    def queue(self, *slabs, jobs=()):
        """Queue the slab sums on the deferral, which keeps the workspace alive until they ran: per
        destination (byte offset in the workspace, splits, n_w, n_b, dw, db or None) — ``splits`` slabs of
        n_w weight floats, then ``splits`` of n_b bias floats — or the ``jobs`` (SlabJob array) an entry
        reported itself."""
        d = self.deferral
        for offset, splits, n_w, n_b, dw, db in slabs:
            base = self.ws.data_ptr() + int(offset)
            d.jobs.append(SlabJob(base, None if db is None else base + 4 * splits * n_w, dw.data_ptr(), _dp(db), n_w,
                                  0 if db is None else n_b, splits, 0, 0))
        d.jobs.extend(jobs)
        d.keep.append(self.ws)

    def grads(self):
        return [None] * len(self.bufs) if self.acc else self.bufs


class FanIn:
    """In-place gradient fan-in for a tensor every consumer of which is an x2g op that can add its
    share into a buffer (dx_add, X2G_GATE_DRBF_ACCUM, X2G_CHAIN_RES_ACCUM): the first consumer whose
    backward runs writes the buffer and returns it as its gradient, every later one adds into it
    in place and returns None.  Autograd runs the tensor's producer only after ALL consumers, so the
    producer sees the full sum — without the add kernel autograd would launch per extra consumer.

    Attach with ``t._x2g_fanin = FanIn()`` only when every consumer of ``t`` is fan-aware (a plain
    consumer's gradient could be summed with the buffer out of place, and later in-place adds would
    then be lost).  The trunk attaches one per layer input and one to the radial basis."""

    def __init__(self):
        self.buf = None
        self.registered = 0
        self.used = 0

    def register(self):
        self.registered += 1
        return self

    def take(self, shape, device):
        """(buffer, first) for one consumer's backward."""
        first = self.buf is None
        if first:
            self.buf = torch.empty(shape, dtype=torch.float32, device=device)
        buf = self.buf
        self.used += 1
        if self.used >= self.registered:  # the last consumer: the next backward starts afresh
            self.buf, self.used = None, 0
        return buf, first


def _fan_of(t):
    """The FanIn attached to ``t`` (registered as one more consumer), or None."""
    f = getattr(t, "_x2g_fanin", None) if t is not None else None
    return f.register() if f is not None else None


def linear_wgrad(dy, x, bias=True, w_param=None, b_param=None):
    """(dW [O, I], db [O] or None) with dW = dy^T x, db = column sums of dy, for row-major
    dy [R, O], x [R, I]: row-split MFMA partials + fixed-order slab sum (csrc/linear.hip).  With the
    layer's parameters given and bucket-backed: summed into the bucket, (None, None) (_WGradDest)."""
    _need_cuda(dy, x)
    dy, x = _f32(dy), _f32(x)
    R, O = dy.shape
    I = x.shape[1]
    dest = _WGradDest([w_param, b_param], dy.device, shapes=[(O, I), (O,) if bias else None])
    dw, db = dest.bufs
    ws_bytes = int(_lib.load().x2g_linear_wgrad_workspace(R, O, I))
    call("x2g_linear_wgrad_ex", ptr(dy), ptr(x), R, O, I, ptr(dw), ptr(db), dest.flags(R),
         ptr(dest.workspace(ws_bytes)), ws_bytes, stream_ptr())
    if dest.deferral:
        dest.queue((0, int(_lib.load().x2g_linear_wgrad_splits(R, O, I)), O * I, O, dw, db))
    return dest.grads()


ACT_NONE, ACT_SILU = _C["ACT_NONE"], _C["ACT_SILU"]


def _dense_fwd_raw(x2, w, b, act, r2=None, want_z=True):
    """y (and z = pre-activation, when act != none and want_z) for row-major x2 [R, K]."""
    N, K = w.shape
    R = x2.shape[0]
    y = torch.empty(R, N, dtype=torch.float32, device=x2.device)
    z = torch.empty(R, N, dtype=torch.float32, device=x2.device) if (act != ACT_NONE and want_z) else None
    call("x2g_dense_fwd", ptr(x2), ptr(w), ptr(b), R, K, N, act, ptr(r2), ptr(y), ptr(z), stream_ptr())
    return y, z


def _dense_bwd_raw(gy2, z, act, x2, w, w_param, b_param, has_bias, need_dx, dx_add=None, dx_out=None):
    """Fused backward of one dense layer: returns (dx or None, dw or None, db or None).

    dx = dz W (+ dx_add; dx_out may alias dx_add for an in-place accumulation).  Weight grads go
    straight into the flat gradient bucket when the parameters are bucket-backed (grad_sink; then
    (None, None) is returned for them), with their slab sums deferred inside deferred_wgrad()."""
    N, K = w.shape
    R = gy2.shape[0]
    dev = gy2.device
    dx = None
    if need_dx or dx_add is not None:  # (the kernels form dz = dy * act'(z) themselves when dx is not wanted)
        dx = dx_out if dx_out is not None else torch.empty(R, K, dtype=torch.float32, device=dev)
    dest = _WGradDest([w_param, b_param], dev, shapes=[(N, K), (N,) if has_bias else None])
    dw, db = dest.bufs
    lib = _lib.load()
    ws_bytes = int(lib.x2g_dense_bwd_workspace(R, K, N))
    call("x2g_dense_bwd_ex", ptr(gy2), ptr(z), act, ptr(x2), ptr(w), R, K, N, ptr(dx), ptr(dx_add), ptr(dw), ptr(db),
         dest.flags(R), ptr(dest.workspace(ws_bytes)), ws_bytes, stream_ptr())
    if dest.deferral:  # (the slabs follow the kernel's dz buffer)
        dest.queue((lib.x2g_dense_bwd_slab_offset(R, K, N), int(lib.x2g_dense_bwd_splits(R, K, N)), N * K, N, dw, db))
    return (dx, *dest.grads())


class _DenseFn(torch.autograd.Function):
    """y = act(x W^T + b) (+ res) in one kernel; backward = one fused kernel (activation
    derivative, data gradient, per-workgroup weight-gradient partials) + a fixed-order slab sum."""

    @staticmethod
    def forward(ctx, x, weight, bias, res, act):
        N, K = weight.shape
        lead = x.shape[:-1]
        x2 = _f32(x.reshape(-1, K))
        w = _f32(weight)
        b = _f32(bias) if bias is not None else None
        r2 = _f32(res.reshape(-1, N)) if res is not None else None
        y, z = _dense_fwd_raw(x2, w, b, act, r2)
        ctx.save_for_backward(x2, w, z)
        ctx.act, ctx.has_bias, ctx.has_res, ctx.lead = act, bias is not None, res is not None, lead
        ctx.w_param, ctx.b_param = weight, bias
        return y.view(*lead, N)

    @staticmethod
    def backward(ctx, gy):
        x2, w, z = ctx.saved_tensors
        N, K = w.shape
        need_x = ctx.needs_input_grad[0]
        dx, dw, db = _dense_bwd_raw(_f32(gy.reshape(-1, N)), z, ctx.act, x2, w, ctx.w_param, ctx.b_param,
                                    ctx.has_bias, need_x)
        dres = gy if ctx.has_res else None
        dx = dx.view(*ctx.lead, K) if need_x else None
        return dx, dw, db, dres, None


class _ResidualFn(torch.autograd.Function):
    """ResidualLayer (residual_layer.py:21-27): y = x + SiLU(W1 SiLU(W0 x + b0) + b1), forward as
    two fused dense kernels; the backward's residual term is folded into the second data
    gradient (dx = dz0 W0 + gy via x2g_dense_bwd_ex's dx_add) instead of an autograd add."""

    @staticmethod
    def forward(ctx, x, w0, b0, w1, b1):
        D = x.shape[-1]
        lead = x.shape[:-1]
        x2 = _f32(x.reshape(-1, D))
        W0, W1 = _f32(w0), _f32(w1)
        B0 = _f32(b0) if b0 is not None else None
        B1 = _f32(b1) if b1 is not None else None
        R = x2.shape[0]
        if W0.shape == (D, D) and W1.shape == (D, D) and D % 4 == 0 and 8 < D <= 128:
            f32 = dict(dtype=torch.float32, device=x2.device)
            h, z0, z1, y = (torch.empty(R, D, **f32) for _ in range(4))
            call("x2g_residual_fwd", ptr(x2), ptr(W0), ptr(B0), ptr(W1), ptr(B1), R, D, ptr(h), ptr(z0), ptr(z1),
                 ptr(y), stream_ptr())
        else:
            h, z0 = _dense_fwd_raw(x2, W0, B0, ACT_SILU)
            y, z1 = _dense_fwd_raw(h, W1, B1, ACT_SILU, r2=x2)
        ctx.save_for_backward(x2, h, z0, z1, W0, W1)
        ctx.params = (w0, b0, w1, b1)
        ctx.lead = lead
        return y.view(*lead, W1.shape[0])

    @staticmethod
    def backward(ctx, gy):
        x2, h, z0, z1, W0, W1 = ctx.saved_tensors
        w0, b0, w1, b1 = ctx.params
        gy2 = _f32(gy.reshape(-1, W1.shape[0]))
        dh, dw1, db1 = _dense_bwd_raw(gy2, z1, ACT_SILU, h, W1, w1, b1, b1 is not None, True)
        dx, dw0, db0 = _dense_bwd_raw(dh, z0, ACT_SILU, x2, W0, w0, b0, b0 is not None, True, dx_add=gy2)
        return dx.view(*ctx.lead, W0.shape[1]), dw0, db0, dw1, db1


def residual_layer(x, w0, b0, w1, b1):
    if not x.is_cuda:
        raise RuntimeError("x2gnn device ops need GPU tensors (no CPU fallback by design)")
    return _ResidualFn.apply(x, w0, b0, w1, b1)


# stage flags; RES_ACCUM: backward only; IN0_ROWMAJOR: forward only, stage 0: no T plane 0 (the weight gradient
# reads the input row-major)
CHAIN_SILU, CHAIN_HOLD, CHAIN_RES_HELD, CHAIN_RES_EXT, CHAIN_RES_ACCUM, CHAIN_IN0_ROWMAJOR, CHAIN_MAX_STAGES = (
    _C["CHAIN_" + n] for n in ("SILU", "HOLD", "RES_HELD", "RES_EXT", "RES_ACCUM", "IN0_ROWMAJOR", "MAX_STAGES"))


ChainStage = _lib.STRUCTS["x2g_chain_stage"]
ChainBwdStage = _lib.STRUCTS["x2g_chain_bwd_stage"]


def chain_wgrad(in_t, dz_t, R, weights, biases, x0=None):
    """Weight / bias gradients of every chain stage from the T-layout operands, as tiled jobs of the flat
    launch; bucket-backed parameters are summed into the bucket (Nones returned for them), queued inside
    ``deferred_wgrad()``.  ``x0``: the chain's input, row-major [R, D], when the forward ran with
    CHAIN_IN0_ROWMAJOR (plane 0 of ``in_t`` is then unwritten and stage 0 reads ``x0``)."""
    n = len(weights)
    dest = _WGradDest(list(weights) + list(biases), in_t.device)
    dws, dbs = dest.bufs[:n], dest.bufs[n:]
    tf = in_t.shape[1]
    jobs = [TiledJob(dz_t.data_ptr() + 4 * g * tf, in_t.data_ptr() + 4 * g * tf, _dp(dws[g]), _dp(dbs[g]), 0, 0)
            for g in range(n)]
    if x0 is not None:
        jobs[0] = TiledJob(dz_t.data_ptr(), x0.data_ptr(), _dp(dws[0]), _dp(dbs[0]), 0, 0, TILED_X_ROWMAJOR)
    _run_tiled(R, jobs, [in_t, dz_t] + ([x0] if x0 is not None else []), dest.acc)
    grads = dest.grads()
    return grads[:n], grads[n:]


class _ChainFn(torch.autograd.Function):
    """A chain of D x D Linear stages on the same rows in ONE kernel (x2g_chain_fwd, csrc/chain.hip):
    stage s computes z_s = in_s W_s^T + b_s, out_s = act(z_s) (+ the held ResidualLayer input or
    the external residual), in_{s+1} = out_s.  Backward: one kernel for every stage's data gradient
    (x2g_chain_bwd, residual gradients folded in registers) + the weight gradients over the stage
    inputs and dz that both kernels leave in the tiled-transposed layout: tiled jobs of the flat launch,
    whose stage 0 reads the chain's row-major input (CHAIN_IN0_ROWMAJOR: the forward then writes no T
    plane 0)."""

    @staticmethod
    def forward(ctx, x, res, flags, ln, *params):
        n = len(flags)
        ws, bs = params[0::2], params[1::2]
        x2 = _f32(x)
        R, D = x2.shape
        r2 = _f32(res) if res is not None else None
        f32 = dict(dtype=torch.float32, device=x2.device)
        grad = _keeps(ctx)  # (autograd runs forward() itself with grad mode off: _apply)
        zs = [torch.empty(R, D, **f32) if (flags[i] & CHAIN_SILU) and grad else None for i in range(n)]
        y = torch.empty(R, D, **f32)
        W = [_f32(w) for w in ws]
        B = [_f32(b) if b is not None else None for b in bs]
        tf = int(_lib.load().x2g_chain_t_floats(R, D))
        # for the backward: W^T of every stage, and every stage input in the T layout
        WT = torch.empty(n, D, D, **f32) if grad else None
        in_t = torch.empty(n, tf, **f32) if grad else None
        # The chain's input stays row-major for the backward anyway (xn on the LayerNorm path, else x2), so
        # stage 0's weight gradient reads it there and the kernel writes no T plane 0.
        ctx.rm0 = WGRAD_X_ROWMAJOR and grad
        fl = [flags[i] | (CHAIN_IN0_ROWMAJOR if ctx.rm0 and i == 0 else 0) for i in range(n)]
        st = (ChainStage * n)(*[ChainStage(_dp(W[i]), _dp(B[i]), _dp(zs[i]), _dp(y) if i == n - 1 else None,
                                           None if WT is None else WT[i].data_ptr(), fl[i]) for i in range(n)])
        ctx.ln = ln is not None
        if ln is None:
            call("x2g_chain_fwd", ptr(x2), ptr(r2), st, n, R, D, ptr(in_t), stream_ptr())
            ln_saved = ()
        else:  # x is the LayerNorm's input: the chain normalises it while staging
            stats, rowptr, G, eps = ln
            xn = torch.empty(R, D, **f32) if grad else None
            rstd = torch.empty(G, **f32) if grad else None
            call("x2g_chain_fwd_ln", ptr(x2), ptr(stats), ptr(rowptr), G, float(eps), ptr(xn), None, ptr(rstd),
                 ptr(r2), st, n, R, D, ptr(in_t), stream_ptr())
            ln_saved = (xn, rstd, rowptr)
            ctx.ln_segments = G
        if grad:
            ctx.save_for_backward(*W, *[z if z is not None else x2 for z in zs], WT, in_t, *ln_saved,
                                  *((x2,) if ctx.rm0 and ln is None else ()))
        ctx.flags, ctx.params, ctx.has_res = tuple(flags), params, res is not None
        ctx.fan_res = _fan_of(res)
        return y

    @staticmethod
    def backward(ctx, gy):
        flags = ctx.flags
        n = len(flags)
        saved = ctx.saved_tensors
        W, zs, WT, in_t = saved[:n], saved[n:2 * n], saved[2 * n], saved[2 * n + 1]
        gy2 = _f32(gy)
        R, D = gy2.shape
        f32 = dict(dtype=torch.float32, device=gy2.device)
        dz_t = torch.empty_like(in_t)
        dx = torch.empty(R, D, **f32)
        dres, first = None, True
        if ctx.has_res and ctx.needs_input_grad[1]:
            if ctx.fan_res is not None:  # add into the layer input's fan-in buffer
                dres, first = ctx.fan_res.take((R, D), gy2.device)
            else:
                dres = torch.empty(R, D, **f32)
        bflags = [f | (CHAIN_RES_ACCUM if (f & CHAIN_RES_EXT) and not first else 0) for f in flags]
        st = (ChainBwdStage * n)(*[ChainBwdStage(_dp(W[i]), WT[i].data_ptr(),
                                                 _dp(zs[i]) if flags[i] & CHAIN_SILU else None, None, bflags[i])
                                   for i in range(n)])
        if not ctx.ln:
            call("x2g_chain_bwd", ptr(gy2), None, st, n, R, D, ptr(dx), ptr(dres), ptr(dz_t), stream_ptr())
        elif _LN_BWD_ROWS:  # dx is the LayerNorm output's gradient: through its backward to the chain's input,
            # the per-row sums it needs left by the chain's last store
            xn, rstd, rowptr = saved[2 * n + 2:2 * n + 5]
            gst = torch.empty(R, 2, **f32)
            call("x2g_chain_bwd_ln", ptr(gy2), None, st, n, R, D, ptr(dx), ptr(dres), ptr(dz_t), ptr(xn), ptr(gst),
                 stream_ptr())
            dxp = torch.empty(R, D, **f32)
            call("x2g_graph_layernorm_bwd_rows", ptr(xn), ptr(dx), ptr(rstd), ptr(rowptr), ctx.ln_segments, D, ptr(gst),
                 ptr(dxp), stream_ptr())
            dx = dxp
        else:
            call("x2g_chain_bwd", ptr(gy2), None, st, n, R, D, ptr(dx), ptr(dres), ptr(dz_t), stream_ptr())
            xn, rstd, rowptr = saved[2 * n + 2:2 * n + 5]
            G = ctx.ln_segments
            dxp = torch.empty(R, D, **f32)
            wsb = int(_lib.load().x2g_graph_layernorm_bwd_workspace(G))
            lws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=gy2.device)
            call("x2g_graph_layernorm_bwd_ex", ptr(xn), ptr(dx), ptr(rstd), ptr(rowptr), G, D, ptr(dxp), ptr(lws), wsb,
                 stream_ptr())
            dx = dxp
        ws, bs = ctx.params[0::2], ctx.params[1::2]
        # (rm0: stage 0's input is the saved row-major one, xn or x2, both right after in_t in `saved`)
        dws, dbs = chain_wgrad(in_t, dz_t, R, ws, bs, x0=saved[2 * n + 2] if ctx.rm0 else None)
        grads = []
        for i in range(n):
            grads += [dws[i], dbs[i]]
        return (dx, dres if first else None, None, None, *grads)


def chain_supported(x, linears):
    """True when _ChainFn's kernels cover these layers (D = 128 rows of 16-byte aligned fp32)."""
    if not x.is_cuda or x.dim() != 2 or x.shape[1] != 128 or not rows_fit(x.shape[0], 128):
        return False
    if len(linears) < 1 or len(linears) > CHAIN_MAX_STAGES:
        return False
    for m in linears:
        if tuple(m.weight.shape) != (128, 128) or m.weight.dtype != torch.float32 or m.weight.data_ptr() % 16:
            return False
        if m.bias is not None and m.bias.data_ptr() % 16:
            return False
    return True


_CHAIN = True  # False: layer-by-layer dense kernels (tests/test_gpu_kernels.py flips it)


def row_chain(x, res, linears, flags, ln=None):
    """Apply the chain of ``linears`` (nn.Linear modules, D x D) with per-stage X2G_CHAIN_* flags.

    ``ln`` = (row_stats [R, 2], segment rowptr [G + 1] int32, G, eps): the chain's input is the
    graph LayerNorm of x (model.py:46), computed while staging from the per-row (mean, M2) the
    attention forward left (``x._x2g_rowstats``); the backward runs the LayerNorm's too."""
    params = []
    for m in linears:
        params += [m.weight, m.bias]
    if ln is not None:
        stats, rowptr, G, eps = ln
        ln = (_f32(stats), _i32(rowptr), int(G), float(eps))
    return _apply(_ChainFn, x, res, tuple(flags), ln, *params)


# ------------------------------------------------------------------------------ small-table chains
TABLE_MAX_STAGES = _C["TABLE_MAX_STAGES"]
_FAN_IN = True  # False: autograd's own fan-in adds (test_fan_in_gradients_match_autograd_adds)


TableStage = _lib.STRUCTS["x2g_table_stage"]
TableBwdStage = _lib.STRUCTS["x2g_table_bwd_stage"]


def table_chain_supported(x, linears):
    """True when x2g_table_chain_* cover these layers: D = 128, <= 16 rows, aligned fp32 weights."""
    if not x.is_cuda or x.dim() != 2 or x.shape[1] != 128 or x.shape[0] > 16:
        return False
    if not 1 <= len(linears) <= TABLE_MAX_STAGES:
        return False
    for m in linears:
        if tuple(m.weight.shape) != (128, 128) or m.weight.dtype != torch.float32 or m.weight.data_ptr() % 16:
            return False
        if m.bias is not None and (m.bias.dtype != torch.float32 or m.bias.data_ptr() % 16):
            return False
    return True


class _TableChainFn(torch.autograd.Function):
    """A tree of D x D Linear stages on a <= 16-row table (x2g_table_chain_fwd/bwd): stage s reads
    x (parent -1) or an earlier stage's output; one launch per direction for the whole tree."""

    @staticmethod
    def forward(ctx, x, spec, pending, *params):
        n = len(spec)
        x2 = _f32(x).contiguous()
        R, D = x2.shape
        dev = x2.device
        ws = [_f32(p).contiguous() for p in params[0::2]]
        bs = [_f32(p).contiguous() if p is not None else None for p in params[1::2]]
        f32 = dict(dtype=torch.float32, device=dev)
        ys = [torch.empty(R, D, **f32) for _ in range(n)]
        zs = [torch.empty(R, D, **f32) if spec[s][1] == ACT_SILU else None for s in range(n)]
        st = (TableStage * n)(*[TableStage(_dp(ws[s]), _dp(bs[s]), spec[s][0], spec[s][1], _dp(zs[s]), _dp(ys[s]))
                                for s in range(n)])
        call("x2g_table_chain_fwd", ptr(x2), R, D, st, n, stream_ptr())
        ctx.save_for_backward(x2, *ws, *ys, *zs)
        ctx.spec, ctx.params, ctx.pending = spec, params, pending
        ctx.set_materialize_grads(False)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *gys):
        flush_keyed(ctx.pending)  # the conv layers' deferred edge-table gradients (keyed_row_sum_deferred)
        spec, n = ctx.spec, len(ctx.spec)
        saved = ctx.saved_tensors
        x2, ws, ys, zs = saved[0], saved[1:1 + n], saved[1 + n:1 + 2 * n], saved[1 + 2 * n:1 + 3 * n]
        R, D = x2.shape
        dev = x2.device
        dys = [_f32(g).contiguous() if g is not None else None for g in gys]
        # the kernel sums or stores per stage (x2g_table_bwd_stage.accum): one destination per stage's pair
        dests = [_WGradDest(ctx.params[2 * s:2 * s + 2], dev) for s in range(n)]
        stages = []
        for s in range(n):
            dw, db = dests[s].bufs
            par, act = spec[s]
            src = x2 if par < 0 else ys[par]
            stages.append(TableBwdStage(_dp(ws[s]), _dp(src), _dp(zs[s]), _dp(dys[s]), _dp(dw), _dp(db), par, act,
                                        1 if dests[s].acc else 0))
        dx = torch.empty(R, D, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        # several leaves (the four lin_edge): leaf stages side by side, then the inner ones
        wsb = int(_lib.load().x2g_table_chain_bwd_workspace(n))
        call("x2g_table_chain_bwd_ex", (TableBwdStage * n)(*stages), n, R, D, ptr(dx),
             ptr(dests[0].workspace(wsb, least=16)), wsb, stream_ptr())
        return (dx, None, None, *(g for d in dests for g in d.grads()))


def table_chain(x, stages):
    """Outputs of every stage of ``stages`` = [(Linear, act, parent), ...] applied to the table x."""
    params, spec = [], []
    for m, act, parent in stages:
        params += [m.weight, m.bias]
        spec.append((int(parent), int(act)))
    pending = []  # keyed row sums consumers queue for this chain's backward (keyed_row_sum_deferred)
    outs = _TableChainFn.apply(x, tuple(spec), pending, *params)
    for o in outs:
        o._x2g_keyed_pending = pending
    return outs


# --------------------------------------------------------------------------- line-node featurisation
def featurize_supported(x, env, lin1, lin2):
    """True when x2g_feat_fwd/bwd cover SiLU(lin2(SiLU(lin1(x * env)))): x [R, K] fp32 with
    256 < K <= 384 even and no gradient wanted for x / env, lin1 K -> 256, lin2 256 -> 128."""
    if not x.is_cuda or x.dim() != 2 or x.dtype != torch.float32 or x.requires_grad:
        return False
    R, K = x.shape
    if not (256 < K <= 384 and K % 2 == 0) or not rows_fit(R, 384):
        return False
    if env is not None and (env.numel() != R or env.requires_grad):
        return False
    if tuple(lin1.weight.shape) != (256, K) or tuple(lin2.weight.shape) != (128, 256):
        return False
    for p in (lin1.weight, lin1.bias, lin2.weight, lin2.bias):
        if p is not None and (p.dtype != torch.float32 or p.data_ptr() % 16):
            return False
    return True


class _FeaturizeFn(torch.autograd.Function):
    """neo_x = SiLU(W2 SiLU(W1 (x * env) + b1) + b2) (xgnn.py:64-67): one forward kernel, one
    backward data kernel and one 8-job T-layout weight-gradient launch (csrc/feature.hip)."""

    @staticmethod
    def forward(ctx, x, env, w1, b1, w2, b2):
        x2 = _f32(x)
        R, K = x2.shape
        dev = x2.device
        tf = int(_lib.load().x2g_chain_t_floats(R, 128))
        f32 = dict(dtype=torch.float32, device=dev)
        y = torch.empty(R, 128, **f32)
        # the backward's T-layout operands (8 planes, ~4 KB per row) only when a gradient is wanted
        grad = _keeps(ctx)
        xs_t, z1_t, y1_t, z2_t = ((torch.empty(max(n * tf, 1), **f32) for n in (3, 2, 2, 1)) if grad
                                  else (None, None, None, None))
        e = _f32(env.reshape(-1)) if env is not None else None
        W1, W2 = _f32(w1), _f32(w2)
        B1 = _f32(b1) if b1 is not None else None
        B2 = _f32(b2) if b2 is not None else None
        call("x2g_feat_fwd", ptr(x2), ptr(e), R, K, ptr(W1), ptr(B1), ptr(W2), ptr(B2), ptr(y), ptr(xs_t), ptr(z1_t),
             ptr(y1_t), ptr(z2_t), stream_ptr())
        if grad:
            ctx.save_for_backward(xs_t, z1_t, y1_t, z2_t, W2)
        ctx.R, ctx.K, ctx.tf = R, K, tf
        ctx.params = (w1, b1, w2, b2)
        return y

    @staticmethod
    def backward(ctx, gy):
        xs_t, z1_t, y1_t, z2_t, W2 = ctx.saved_tensors
        R, K, tf = ctx.R, ctx.K, ctx.tf
        dev = gy.device
        f32 = dict(dtype=torch.float32, device=dev)
        dz2_t, dz1_t = torch.empty(max(tf, 1), **f32), torch.empty(max(2 * tf, 1), **f32)
        call("x2g_feat_bwd", ptr(_f32(gy)), ptr(z2_t), ptr(z1_t), ptr(W2), R, ptr(dz2_t), ptr(dz1_t), stream_ptr())
        dest = _WGradDest(ctx.params, dev)
        dw1, db1, dw2, db2 = dest.bufs
        fb = 4  # bytes per float
        specs = []  # (dy_t, x_t, dw pointer, db pointer, ld, cols)
        for o in range(2):
            for i in range(3):
                specs.append((dz1_t.data_ptr() + fb * o * tf, xs_t.data_ptr() + fb * i * tf,
                              dw1.data_ptr() + fb * (o * 128 * K + i * 128),
                              db1.data_ptr() + fb * o * 128 if (db1 is not None and i == 0) else None, K,
                              min(128, K - 128 * i)))
        for i in range(2):
            specs.append((dz2_t.data_ptr(), y1_t.data_ptr() + fb * i * tf, dw2.data_ptr() + fb * i * 128,
                          db2.data_ptr() if (db2 is not None and i == 0) else None, 256, 128))
        _run_tiled(R, [TiledJob(*sp) for sp in specs], [dz1_t, dz2_t, xs_t, y1_t], dest.acc)
        return (None, None, *dest.grads())


def featurize(x, env, lin1, lin2):
    """SiLU(lin2(SiLU(lin1(x * env[:, None])))) through the fused featurisation kernels."""
    return _apply(_FeaturizeFn, x, env, lin1.weight, lin1.bias, lin2.weight, lin2.bias)


TiledJob = _lib.STRUCTS["x2g_tiled_job"]  # layout: TILED_DY_ROWMAJOR | TILED_X_ROWMAJOR (0: both in the T layout)
TILED_DY_ROWMAJOR, TILED_X_ROWMAJOR = _C["TILED_DY_ROWMAJOR"], _C["TILED_X_ROWMAJOR"]

# The weight gradients' x operands that exist row-major anyway (the projections' x, the chains' input) are
# read there, and no T-layout copy of them is written.  False: the forwards write those copies (x_t, T
# plane 0) as before.  A constant like the switches above (an A/B script or a test sets it).
WGRAD_X_ROWMAJOR = True


def _tiled_now(R, jobs, acc, dev):
    """The given x2g_tiled_jobs in one flat launch of their own, slab sums included."""
    lib = _lib.load()
    n = len(jobs)
    ws_bytes = int(lib.x2g_tiled_wgrad_flat_workspace(R, 128, n))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    call("x2g_tiled_wgrad_flat", (TiledJob * n)(*jobs), n, R, 128, ACCUM_WGRAD if acc else 0, None, ptr(ws), ws_bytes,
         stream_ptr())


def _run_tiled(R, jobs, keep, acc):
    """Run x2g_tiled_jobs over ``R`` rows: queued on the open deferral for its flat launch when their
    destinations are bucket-backed (``acc``) and one is open, else launched now.  ``keep``: the tensors the
    jobs point into (a queued job runs after the backward that made it returned)."""
    d = _defer() if acc else None
    if d is not None:
        _queue_tiled(d, R, jobs, keep)
    else:
        _tiled_now(R, jobs, acc, keep[0].device)


Proj = _lib.STRUCTS["x2g_proj"]
ProjGrad = _lib.STRUCTS["x2g_proj_grad"]


def tiled_wgrad(dy_ts, x_ts, R, weights, biases, layouts=None):
    """Weight / bias gradients of D x D Linear layers, one job of the flat launch per layer; bucket-backed
    parameters are summed into the bucket (Nones returned), queued inside ``deferred_wgrad()``.
    ``layouts``: per job TILED_*_ROWMAJOR bits for operands given as row-major [R, D] tensors (default:
    all in the T layout)."""
    n = len(weights)
    dest = _WGradDest(list(weights) + list(biases), dy_ts[0].device)
    dws, dbs = dest.bufs[:n], dest.bufs[n:]
    lay = layouts if layouts is not None else [0] * n
    jobs = [TiledJob(_dp(dy_ts[g]), _dp(x_ts[g]), _dp(dws[g]), _dp(dbs[g]), 0, 0, lay[g]) for g in range(n)]
    _run_tiled(R, jobs, list(dy_ts) + list(x_ts), dest.acc)
    grads = dest.grads()
    return grads[:n], grads[n:]


def conv_proj_fused_supported(x, rbf, weights, biases):
    """True when the row-chain style projection kernels (x2g_conv_proj_fwd / _bwd) cover the layer."""
    if not _CHAIN or not x.is_cuda or x.dim() != 2 or x.shape[1] != 128 or not rows_fit(x.shape[0], 128):
        return False
    if rbf.dim() != 2 or not 1 <= rbf.shape[1] <= 8 or rbf.shape[0] != x.shape[0]:
        return False
    for w in weights:
        if tuple(w.shape) != (128, 128) or w.dtype != torch.float32 or w.data_ptr() % 16:
            return False
    return all(b is None or b.data_ptr() % 16 == 0 for b in biases)


def _conv_proj_bwd_gate(grads, x2, rbf2, Wr, wr, dx, first_x, need_rbf, drbf_out, first_r):
    """x2g_conv_proj_bwd_gate: dx (in place, += when not first_x), drbf, dW_rbf of the projections'
    backward in one launch; returns (dx, drbf, dW_rbf) with None where the gradient went into a
    caller's buffer (fan-in, gradient bucket)."""
    E, D = x2.shape
    RR = rbf2.shape[1]
    dev = x2.device
    drbf = drbf_out if drbf_out is not None else (
        torch.empty(E, RR, dtype=torch.float32, device=dev) if need_rbf else None)
    dest = _WGradDest([wr], dev, shapes=[(D, RR)])
    (dw,) = dest.bufs
    lib = _lib.load()
    ws_bytes = int(lib.x2g_conv_proj_bwd_gate_workspace(E, RR))
    flags = dest.flags(E) | (GATE_DRBF_ACCUM if (need_rbf and not first_r) else 0)
    call("x2g_conv_proj_bwd_gate", grads, E, D, ptr(x2), ptr(rbf2), RR, ptr(Wr), ptr(dx),
         None if first_x else ptr(dx), ptr(drbf), ptr(dw), flags, ptr(dest.workspace(ws_bytes)), ws_bytes,
         stream_ptr())
    if dest.deferral:
        dest.queue((0, int(lib.x2g_conv_proj_bwd_gate_splits(E)), D * RR, 0, dw, None))
    return (dx, drbf, *dest.grads())


class _ConvProjFusedFn(torch.autograd.Function):
    """SBFTransformerConv's projections (sbftransformer_conv.py:99-107,127) in one kernel each way:
    x2g_conv_proj_fwd (x and x_src = x * lin_rbf(rbf) in LDS, q/k/v/skip per wave slice) and
    x2g_conv_proj_bwd (dx = dq Wq + dskip Ws, dx_src = dk Wk + dv Wv) + the gate backward
    (x2g_rbf_gate_bwd: dx += dx_src * f, drbf, dW_rbf) + one T-layout weight-gradient launch."""

    @staticmethod
    def forward(ctx, x, rbf, wr, wq, bq, wk, bk, wv, bv, ws, bs):
        E, D = x.shape
        x2, rbf2, Wr = _f32(x), _f32(rbf), _f32(wr)
        W = [_f32(t) for t in (wq, wk, wv, ws)]
        B = [_f32(t) if t is not None else None for t in (bq, bk, bv, bs)]
        f32 = dict(dtype=torch.float32, device=x2.device)
        outs = [torch.empty(E, D, **f32) for _ in range(4)]
        grad = _keeps(ctx)
        lib = _lib.load()
        tf = int(lib.x2g_chain_t_floats(E, D))
        WT = torch.empty(4, D, D, **f32) if grad else None
        # x_src exists only inside the kernel, so its T-layout copy is kept for dW_k / dW_v; x is saved
        # row-major anyway and the weight gradient reads it there (no x_t)
        xs_t = torch.empty(tf, **f32) if grad else None
        x_t = torch.empty(tf, **f32) if grad and not WGRAD_X_ROWMAJOR else None
        proj = (Proj * 4)(*[Proj(_dp(W[i]), _dp(B[i]), _dp(outs[i]), None if WT is None else WT[i].data_ptr())
                            for i in range(4)])
        call("x2g_conv_proj_fwd", ptr(x2), ptr(rbf2), rbf2.shape[1], ptr(Wr), proj, E, D, ptr(x_t), ptr(xs_t),
             stream_ptr())
        if grad:
            ctx.save_for_backward(x2, rbf2, Wr, *W, WT, xs_t, x_t)
        ctx.params = (wr, wq, bq, wk, bk, wv, bv, ws, bs)
        ctx.fan_x, ctx.fan_r = _fan_of(x), _fan_of(rbf)
        return tuple(outs)

    @staticmethod
    def backward(ctx, gq, gk, gv, gskip):
        x2, rbf2, Wr, Wq, Wk, Wv, Ws, WT, xs_t, x_t = ctx.saved_tensors
        wr, wq, bq, wk, bk, wv, bv, ws, bs = ctx.params
        E, D = x2.shape
        f32 = dict(dtype=torch.float32, device=x2.device)
        g = [_f32(t) if t is not None else torch.zeros(E, D, **f32) for t in (gq, gk, gv, gskip)]
        W = (Wq, Wk, Wv, Ws)
        # no T-layout copies of the four gradients (g_t NULL): the weight gradient reads g itself
        grads = (ProjGrad * 4)(*[ProjGrad(_dp(g[i]), _dp(W[i]), WT[i].data_ptr(), None) for i in range(4)])
        first_x = first_r = True
        if ctx.fan_x is not None:  # dx goes into (or adds onto) the layer input's fan-in buffer
            dx, first_x = ctx.fan_x.take((E, D), x2.device)
        else:
            dx = torch.empty(E, D, **f32)
        need_rbf = ctx.needs_input_grad[1]
        drbf_out = None
        if need_rbf and ctx.fan_r is not None:
            drbf_out, first_r = ctx.fan_r.take(rbf2.shape, x2.device)
        # the gate's backward inside the projection kernel: dxs stays in registers
        gx, grbf, dwr = _conv_proj_bwd_gate(grads, x2, rbf2, Wr, wr, dx, first_x, need_rbf, drbf_out, first_r)
        gx = gx if first_x else None
        grbf = grbf if first_r else None
        # dy = g (row-major) for all four; x = x2 (row-major) for q and skip, the T-layout x_src for k and v.
        # g and x2 go on the deferral's keep list: the flat launch reads them after this backward returned.
        xo = x2 if x_t is None else x_t
        lx = TILED_DY_ROWMAJOR | (TILED_X_ROWMAJOR if x_t is None else 0)
        dws, dbs = tiled_wgrad(g, [xo, xs_t, xs_t, xo], E, [wq, wk, wv, ws], [bq, bk, bv, bs],
                               layouts=[lx, TILED_DY_ROWMAJOR, TILED_DY_ROWMAJOR, lx])
        return (gx, (grbf if need_rbf else None), dwr, dws[0], dbs[0], dws[1], dbs[1], dws[2], dbs[2], dws[3],
                dbs[3])


class _ConvProjFn(torch.autograd.Function):
    """The dense projections of SBFTransformerConv.forward (sbftransformer_conv.py:99-107,127):
    rf = lin_rbf(rbf), x_src = x * rf, q = lin_query(x), k = lin_key(x_src), v = lin_value(x_src),
    skip = lin_skip(x).  The backward chains the four data gradients into one buffer per input
    (x2g_dense_bwd_ex dx_add, in place) instead of summing them with autograd adds."""

    @staticmethod
    def forward(ctx, x, rbf, wr, wq, bq, wk, bk, wv, bv, ws, bs):
        E, D = x.shape
        x2, rbf2 = _f32(x), _f32(rbf)
        Wr, Wq, Wk, Wv, Ws = (_f32(t) for t in (wr, wq, wk, wv, ws))
        Bq, Bk, Bv, Bs = (_f32(t) if t is not None else None for t in (bq, bk, bv, bs))
        if gate_supported(D, rbf2.shape[1]):  # x_src = x * lin_rbf(rbf), filter not materialised
            rf = None
            xs = torch.empty_like(x2)
            call("x2g_rbf_gate_fwd", ptr(x2), ptr(rbf2), ptr(Wr), None, E, D, rbf2.shape[1], ptr(xs), stream_ptr())
        else:
            rf, _ = _dense_fwd_raw(rbf2, Wr, None, ACT_NONE)
            xs = x2 * rf
        q, k, v, skip = _projections4(x2, xs, (Wq, Bq), (Wk, Bk), (Wv, Bv), (Ws, Bs))
        ctx.save_for_backward(x2, rbf2, rf, xs, Wr, Wq, Wk, Wv, Ws)  # rf None on the gate path
        ctx.params = (wr, wq, bq, wk, bk, wv, bv, ws, bs)
        return q, k, v, skip

    @staticmethod
    def backward(ctx, gq, gk, gv, gskip):
        x2, rbf2, rf, xs, Wr, Wq, Wk, Wv, Ws = ctx.saved_tensors
        wr, wq, bq, wk, bk, wv, bv, ws, bs = ctx.params
        g = [_f32(t) if t is not None else torch.zeros_like(x2) for t in (gq, gk, gv, gskip)]
        gxs, dwk, dbk = _dense_bwd_raw(g[1], None, ACT_NONE, xs, Wk, wk, bk, bk is not None, True)
        gxs, dwv, dbv = _dense_bwd_raw(g[2], None, ACT_NONE, xs, Wv, wv, bv, bv is not None, True, dx_add=gxs,
                                       dx_out=gxs)
        need_rbf = ctx.needs_input_grad[1]
        if rf is None:  # one pass: gx = gxs * f, grbf, dWr
            gx, grbf, dwr, _ = _gate_bwd(gxs, None, x2, rbf2, Wr, None, wr, None, True, need_rbf)
        else:
            grf = gxs * x2  # d rf
            gx = gxs * rf   # x_src = x * rf
        gx, dwq, dbq = _dense_bwd_raw(g[0], None, ACT_NONE, x2, Wq, wq, bq, bq is not None, True, dx_add=gx,
                                      dx_out=gx)
        gx, dws, dbs = _dense_bwd_raw(g[3], None, ACT_NONE, x2, Ws, ws, bs, bs is not None, True, dx_add=gx,
                                      dx_out=gx)
        if rf is not None:
            grbf, dwr, _ = _dense_bwd_raw(grf, None, ACT_NONE, rbf2, Wr, wr, None, False, need_rbf)
        return gx, (grbf if need_rbf else None), dwr, dwq, dbq, dwk, dbk, dwv, dbv, dws, dbs


def _projections4(x2, xs, pq, pk, pv, ps):
    """q = lin_query(x), k = lin_key(x_src), v = lin_value(x_src), skip = lin_skip(x) as ONE
    batched launch (x2g_dense_fwd_batched, 4 groups) when the shapes allow, else four."""
    R, K = x2.shape
    N = pq[0].shape[0]
    outs = [torch.empty(R, N, dtype=torch.float32, device=x2.device) for _ in range(4)]
    ok = (K % 4 == 0 and N % 4 == 0 and 8 < K <= 128 and N <= 128 and rows_fit(R, 128)
          and all(p[0].shape == pq[0].shape for p in (pk, pv, ps)))
    if ok and R > 0:
        srcs = (x2, xs, xs, x2)
        grp = (DenseFwdGroup * 4)(*[DenseFwdGroup(_dp(srcs[g]), _dp(p[0]), _dp(p[1]), None, _dp(outs[g]), None)
                                    for g, p in enumerate((pq, pk, pv, ps))])
        call("x2g_dense_fwd_batched", grp, 4, R, K, N, ACT_NONE, stream_ptr())
        return outs
    return [_dense_fwd_raw(src, p[0], p[1], ACT_NONE)[0] for src, p in zip((x2, xs, xs, x2), (pq, pk, pv, ps))]


def gate_supported(D, R):
    """Shapes the rbf-gate kernels are compiled for (csrc/rbf_gate.hip)."""
    return D in (64, 128, 256) and 1 <= R <= 8


def _gate_bwd(g, owner, x, rbf, w, b, w_param, b_param, need_dx, need_rbf, dx_add=None, dx_out=None, drbf_out=None,
              drbf_acc=False):
    """x2g_rbf_gate_bwd: (dx, drbf, dw, db); dw / db are None when summed into the gradient bucket.
    dx_out / drbf_out: caller buffers (dx_out may alias dx_add); drbf_acc: drbf_out += the gradient."""
    rows, D = x.shape
    R = rbf.shape[1]
    dev = x.device
    dx = dx_out if dx_out is not None else (torch.empty(rows, D, dtype=torch.float32, device=dev) if need_dx else None)
    drbf = drbf_out if drbf_out is not None else (
        torch.empty(rows, R, dtype=torch.float32, device=dev) if need_rbf else None)
    dest = _WGradDest([w_param, b_param], dev, shapes=[(D, R), None if b is None else (D,)])
    dw, db = dest.bufs
    lib = _lib.load()
    ws_bytes = int(lib.x2g_rbf_gate_bwd_workspace(rows, D, R))
    flags = dest.flags(rows) | (GATE_DRBF_ACCUM if drbf_acc else 0)
    call("x2g_rbf_gate_bwd", ptr(g), ptr(owner), ptr(x), ptr(rbf), ptr(w), ptr(b), rows, D, R, ptr(dx), ptr(dx_add),
         ptr(drbf), ptr(dw), ptr(db), flags, ptr(dest.workspace(ws_bytes)), ws_bytes, stream_ptr())
    if dest.deferral:
        dest.queue((0, int(lib.x2g_rbf_gate_bwd_splits(rows)), D * R, D, dw, db))
    return (dx, drbf, *dest.grads())


class _RbfPoolFn(torch.autograd.Function):
    """out[n] = sum over rows e of segment n of x[e] * (W rbf[e] + b) (readout.py:39-41,66-67:
    lin_rbf(rbf) * x pooled edges -> atoms) without the [E, D] filter tensor."""

    @staticmethod
    def forward(ctx, x, rbf, w, b, owner, rowptr, n_seg):
        x2, rbf2, W = _f32(x), _f32(rbf), _f32(w)
        B = _f32(b) if b is not None else None
        D, R = x2.shape[1], rbf2.shape[1]
        out = torch.empty(n_seg, D, dtype=torch.float32, device=x2.device)
        call("x2g_rbf_pool_fwd", ptr(x2), ptr(rbf2), ptr(W), ptr(B), ptr(rowptr), n_seg, D, R, ptr(out), stream_ptr())
        ctx.save_for_backward(x2, rbf2, W, B)
        ctx.owner, ctx.params = owner, (w, b)
        ctx.fan_x, ctx.fan_r = _fan_of(x), _fan_of(rbf)
        return out

    @staticmethod
    def backward(ctx, gp):
        x2, rbf2, W, B = ctx.saved_tensors
        w, b = ctx.params
        need_x, need_r = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dev = x2.device
        dx_out = drbf_out = None
        first_x = first_r = True
        if need_x and ctx.fan_x is not None:
            dx_out, first_x = ctx.fan_x.take(x2.shape, dev)
        if need_r and ctx.fan_r is not None:
            drbf_out, first_r = ctx.fan_r.take(rbf2.shape, dev)
        dx, drbf, dw, db = _gate_bwd(_f32(gp), ctx.owner, x2, rbf2, W, B, w, b, need_x, need_r,
                                     dx_add=None if first_x else dx_out, dx_out=dx_out, drbf_out=drbf_out,
                                     drbf_acc=not first_r)
        return (dx if first_x else None), (drbf if first_r else None), dw, db, None, None, None


def _addr(t):
    """Raw device address of a tensor for a ctypes struct field (None -> NULL)."""
    return None if t is None else t.data_ptr()


GateJob = _lib.STRUCTS["x2g_gate_job"]
GATE_MAX_JOBS = _C["GATE_MAX_JOBS"]
# the readouts' edge -> atom pools as one launch each way (x2g_rbf_pool_fwd_batch / _gate_bwd_batch)
_POOL_BATCH = True


class _RbfPoolBatchFn(torch.autograd.Function):
    """Several rbf pools over the same rows / atoms / basis (_RbfPoolFn's math per job), one launch
    each way; the basis gradient is the jobs' sum (one fan-in consumer for the whole batch)."""

    @staticmethod
    def forward(ctx, n, rbf, owner, rowptr, n_seg, *tensors):
        xs, ws, bs = tensors[:n], tensors[n:2 * n], tensors[2 * n:]
        rbf2 = _f32(rbf)
        x2 = [_f32(x) for x in xs]
        W = [_f32(w) for w in ws]
        B = [_f32(b) if b is not None else None for b in bs]
        D, R = x2[0].shape[1], rbf2.shape[1]
        outs = [torch.empty(n_seg, D, dtype=torch.float32, device=rbf2.device) for _ in range(n)]
        jobs = (GateJob * n)(*[GateJob(x2[j].data_ptr(), W[j].data_ptr(), _addr(B[j]), outs[j].data_ptr(), None, None,
                                       None, None, None) for j in range(n)])
        call("x2g_rbf_pool_fwd_batch", jobs, n, ptr(rbf2), ptr(rowptr), n_seg, D, R, stream_ptr())
        ctx.save_for_backward(rbf2, *x2, *W)
        ctx.n, ctx.n_seg, ctx.B, ctx.owner, ctx.params = n, n_seg, B, owner, (ws, bs)
        ctx.fan_x = [_fan_of(x) for x in xs]
        ctx.fan_r = _fan_of(rbf)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gps):
        n = ctx.n
        saved = ctx.saved_tensors
        rbf2, x2, W = saved[0], saved[1:1 + n], saved[1 + n:1 + 2 * n]
        ws, bs = ctx.params
        rows, D = x2[0].shape
        R = rbf2.shape[1]
        dev = rbf2.device
        need_r = ctx.needs_input_grad[1]
        drbf, first_r = None, True
        if need_r:
            if ctx.fan_r is not None:
                drbf, first_r = ctx.fan_r.take(rbf2.shape, dev)
            else:
                drbf = torch.empty(rows, R, dtype=torch.float32, device=dev)
        dest = _WGradDest(list(ws) + list(bs), dev)  # one launch, one flag word: all jobs sum into the bucket or none
        dws, dbs = dest.bufs[:n], dest.bufs[n:]
        dx_ret, jobs, keep = [], [], []
        for j in range(n):
            need_x = ctx.needs_input_grad[5 + j]
            dx, first = None, True
            if need_x:
                if ctx.fan_x[j] is not None:
                    dx, first = ctx.fan_x[j].take(x2[j].shape, dev)
                else:
                    dx = torch.empty(rows, D, dtype=torch.float32, device=dev)
            dx_ret.append(dx if (need_x and first) else None)
            g = _f32(gps[j]) if gps[j] is not None else torch.zeros(ctx.n_seg, D, dtype=torch.float32, device=dev)
            keep.append(g)
            jobs.append(GateJob(x2[j].data_ptr(), W[j].data_ptr(), _addr(ctx.B[j]), None, g.data_ptr(), _addr(dx),
                                None if first else _addr(dx), dws[j].data_ptr(), _addr(dbs[j])))
        lib = _lib.load()
        ws_bytes = int(lib.x2g_rbf_gate_bwd_batch_workspace(rows, D, R, n))
        flags = dest.flags(rows) | (0 if first_r else GATE_DRBF_ACCUM)
        out = (SlabJob * n)()  # the entry reports its slabs itself
        call("x2g_rbf_gate_bwd_batch", (GateJob * n)(*jobs), n, ptr(ctx.owner), ptr(rbf2), rows, D, R, ptr(drbf), flags,
             out, ptr(dest.workspace(ws_bytes)), ws_bytes, stream_ptr())
        if dest.deferral:
            dest.queue(jobs=out)
        return (None, drbf if (need_r and first_r) else None, None, None, None, *dx_ret, *dest.grads())


def rbf_pool_batch(xs, rbf, weights, biases, owner, rowptr, n_seg: int):
    """[rbf_pool(x_j, rbf, W_j, b_j, owner, rowptr, n_seg) for j] in one launch each way."""
    _need_cuda(rbf, *xs)
    n = len(xs)
    return list(_RbfPoolBatchFn.apply(n, rbf, _i32(owner), _i32(rowptr), int(n_seg), *xs, *weights, *biases))


def rbf_pool_batch_supported(xs, rbf, weights):
    return (_POOL_BATCH and 1 < len(xs) <= GATE_MAX_JOBS and all(x.is_cuda and x.dim() == 2 for x in xs)
            and len({tuple(x.shape) for x in xs}) == 1 and gate_supported(xs[0].shape[1], rbf.shape[1])
            and all(tuple(w.shape) == (xs[0].shape[1], rbf.shape[1]) for w in weights))


def rbf_pool(x, rbf, weight, bias, owner, rowptr, n_seg: int):
    """Segment sums of x * lin_rbf(rbf) over rows sorted by ``owner`` (CSR ``rowptr``)."""
    _need_cuda(x, rbf)
    return _RbfPoolFn.apply(x, rbf, weight, bias, _i32(owner), _i32(rowptr), int(n_seg))


def conv_combine_supported(heads, channels):
    """Shapes the combine pass is compiled for (csrc/conv_combine.hip)."""
    return heads >= 1 and channels in (4, 8, 16, 32) and heads * channels in (32, 64, 128, 256)


class _ConvCombineFn(torch.autograd.Function):
    """SBFTransformerConv's concat=False / beta=True (reference sbftransformer_conv.py:115-127) after the
    attention: m = attn or its mean over heads, y = beta x_r + (1 - beta) m with beta = sigmoid(w_beta .
    [m, x_r, m - x_r]), or m + x_r (include/x2g_conv.h).  Keeps attn, x_r and beta [rows] for the backward."""

    @staticmethod
    def forward(ctx, attn, x_r, w_beta, heads, channels, concat, want_stats):
        a = _f32(attn)
        x = None if x_r is None else _f32(x_r)
        w = None if w_beta is None else _f32(w_beta).reshape(-1)
        rows = a.shape[0]
        f32 = dict(dtype=torch.float32, device=a.device)
        y = torch.empty(rows, heads * channels if concat else channels, **f32)
        keeps = _keeps(ctx)
        beta = torch.empty(rows, **f32) if w is not None and keeps else None
        stats = torch.empty(rows, 2, **f32) if want_stats else None
        call("x2g_conv_combine_fwd", ptr(a), ptr(x), ptr(w), rows, heads, channels, int(concat), ptr(y), ptr(beta),
             ptr(stats), stream_ptr())
        if keeps:
            ctx.save_for_backward(a, x, w, beta)
        ctx.cfg, ctx.w_param = (heads, channels, int(concat)), w_beta
        if stats is not None:
            ctx.mark_non_differentiable(stats)
        return y, stats

    @staticmethod
    def backward(ctx, dy, _dstats=None):
        a, x, w, beta = ctx.saved_tensors
        heads, channels, concat = ctx.cfg
        dy = _f32(dy)
        rows, dev = a.shape[0], a.device
        need_a, need_x = ctx.needs_input_grad[0], x is not None and ctx.needs_input_grad[1]
        lib = _lib.load()
        if w is None:  # no gate: d_xr = dy, d_attn = dy (/ H, broadcast over the heads)
            d_attn = None
            if need_a and concat:
                d_attn = dy
            elif need_a:
                d_attn = torch.empty_like(a)
                call("x2g_conv_combine_bwd", ptr(dy), None, None, None, None, rows, heads, channels, concat,
                     ptr(d_attn), None, None, 0, None, None, 0, stream_ptr())
            return d_attn, (dy if need_x else None), None, None, None, None, None
        d_attn = torch.empty_like(a) if need_a else None
        d_xr = torch.empty_like(x) if need_x else None
        dest = _WGradDest([ctx.w_param], dev, shapes=[tuple(ctx.w_param.shape)])
        (dw,) = dest.bufs
        ws_bytes = int(lib.x2g_conv_combine_bwd_workspace(rows, heads, channels, concat))
        flags = dest.flags(rows)
        job = SlabJob()
        call("x2g_conv_combine_bwd", ptr(dy), ptr(a), ptr(x), ptr(w), ptr(beta), rows, heads, channels, concat,
             ptr(d_attn), ptr(d_xr), ptr(dw), flags,
             ctypes.cast(ctypes.pointer(job), ctypes.c_void_p) if dest.deferral else None,
             ptr(dest.workspace(ws_bytes)), ws_bytes, stream_ptr())
        if dest.deferral:  # (the deferral keeps the workspace until its one batched sum ran)
            dest.queue(jobs=[job])
        return d_attn, d_xr, dest.grads()[0], None, None, None, None


def conv_combine(attn, x_r, w_beta, heads: int, channels: int, concat: bool = True):
    """The conv's output from the attention's ``attn`` [E, heads * channels] (computed with a zero skip row),
    ``x_r = lin_skip(x)`` [E, Dout] or None (root_weight=False) and ``w_beta`` = lin_beta.weight [1, 3 Dout] or
    None: see _ConvCombineFn.  Dout = heads * channels (concat) or channels (mean over heads).  At Dout = 128
    the output carries its per-row (mean, M2) as ``_x2g_rowstats``, like the attention's own output, so the graph
    LayerNorm that follows stays fused into the next row chain."""
    _need_cuda(attn, x_r, w_beta)
    heads, channels = int(heads), int(channels)
    if not conv_combine_supported(heads, channels):
        raise NotImplementedError(f"conv combine: heads * channels in 32 / 64 / 128 / 256 and channels in 4 / 8 / 16 "
                                  f"/ 32 are compiled, not heads = {heads}, channels = {channels}")
    if w_beta is not None and x_r is None:
        raise ValueError("conv combine: the gate needs x_r (beta is off without root_weight)")
    dout = heads * channels if concat else channels
    y, stats = _apply(_ConvCombineFn, attn, x_r, w_beta, heads, channels, bool(concat), _LN_FUSE and dout == 128)
    if stats is not None:
        y._x2g_rowstats = stats
    return y


def conv_projections(x, rbf, wr, wq, bq, wk, bk, wv, bv, ws, bs):
    if not x.is_cuda:
        raise RuntimeError("x2gnn device ops need GPU tensors (no CPU fallback by design)")
    if conv_proj_fused_supported(x, rbf, (wq, wk, wv, ws), (bq, bk, bv, bs)):
        return _apply(_ConvProjFusedFn, x, rbf, wr, wq, bq, wk, bk, wv, bv, ws, bs)
    return _apply(_ConvProjFn, x, rbf, wr, wq, bq, wk, bk, wv, bv, ws, bs)


def dense(x, weight, bias=None, act=ACT_NONE, res=None):
    """Fused row-wise Linear (+ SiLU) (+ residual) on the GPU (csrc/dense.hip)."""
    if not x.is_cuda:
        raise RuntimeError("x2gnn device ops need GPU tensors (no CPU fallback by design)")
    return _DenseFn.apply(x, weight, bias, res, act)


def linear(x, weight, bias=None):
    return dense(x, weight, bias)


# ---------------------------------------------------------------------------------- segments
def _seg_sum_raw(x, mul, rowptr, n_seg):
    D = x.shape[1]
    out = torch.empty(n_seg, D, dtype=torch.float32, device=x.device)
    call("x2g_segment_sum", ptr(x), ptr(mul), ptr(rowptr), n_seg, D, ptr(out), stream_ptr())
    return out


def _seg_bcast_raw(g, mul, rowptr, n_rows):
    D = g.shape[1]
    out = torch.empty(n_rows, D, dtype=torch.float32, device=g.device)
    call("x2g_segment_broadcast", ptr(g), ptr(mul), ptr(rowptr), g.shape[0], D, ptr(out), stream_ptr())
    return out


class _SegmentSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mul, rowptr, n_seg):
        x = _f32(x)
        mul = _f32(mul) if mul is not None else None
        ctx.save_for_backward(x, mul, rowptr)
        return _seg_sum_raw(x, mul, rowptr, n_seg)

    @staticmethod
    def backward(ctx, g):
        x, mul, rowptr = ctx.saved_tensors
        g = _f32(g)
        dx = _seg_bcast_raw(g, mul, rowptr, x.shape[0]) if ctx.needs_input_grad[0] else None
        dmul = None
        if mul is not None and ctx.needs_input_grad[1]:
            dmul = _seg_bcast_raw(g, x, rowptr, x.shape[0])
        return dx, dmul, None, None


def segment_sum(x, rowptr, num_segments: int, mul=None):
    """out[g] = sum_{r in segment g} x[r] (* mul[r]); rows of a segment are contiguous."""
    _need_cuda(x, rowptr)
    squeeze = x.dim() == 1
    if squeeze:
        x = x.unsqueeze(1)
        mul = mul.unsqueeze(1) if mul is not None else None
    out = _SegmentSum.apply(x, mul, _i32(rowptr), int(num_segments))
    return out.squeeze(1) if squeeze else out


# ------------------------------------------------------------------- atom context (SBFTransformerV2's edge term)
# False: the composition segment_sum -> row_chain (3 stages) and their adjoints instead of the fused kernels
# (tests/test_gpu_model_v2.py flips it); the composition also serves shapes the kernels are not compiled for.
_ATOM_CTX = True


def atom_context_supported(x, linears):
    """True when x2g_atom_context_fwd / _bwd cover these layers (D = 128 rows of 16-byte aligned fp32)."""
    if not x.is_cuda or x.dim() != 2 or x.shape[1] != 128 or not rows_fit(x.shape[0], 128):
        return False
    for m in linears:
        if tuple(m.weight.shape) != (128, 128) or m.weight.dtype != torch.float32 or m.weight.data_ptr() % 16:
            return False
    return linears[2].bias is None


class _AtomContextFn(torch.autograd.Function):
    """tab [N, D] = lin_edge(edgenn(A)), A[a] = the sum of atom a's out-edge rows of x, in ONE kernel each way
    (x2g_atom_context_fwd / _bwd, csrc/atom_context.hip).  The forward keeps A, z0, h and g: A, h and g are the
    row-major x operands of the three weight gradients, z0 is where SiLU' is taken.  The backward leaves d_g and
    d_z0 row-major; the five weight / bias gradients are row-major jobs of the flat launch (tiled_wgrad).  The
    layer input's gradient joins its fan-in buffer through the kernel's accumulate flag."""

    @staticmethod
    def forward(ctx, x, rowptr, n_atoms, w0, b0, w1, b1, we):
        x2 = _f32(x)
        E, D = x2.shape
        N = int(n_atoms)
        f32 = dict(dtype=torch.float32, device=x2.device)
        grad = _keeps(ctx)
        W0, W1, We = _f32(w0), _f32(w1), _f32(we)
        B0 = _f32(b0) if b0 is not None else None
        B1 = _f32(b1) if b1 is not None else None
        tab = torch.empty(N, D, **f32)
        kept = [torch.empty(N, D, **f32) if grad else None for _ in range(4)]  # A, z0, h, g
        call("x2g_atom_context_fwd", ptr(x2), ptr(rowptr), N, E, D, ptr(W0), ptr(B0), ptr(W1), ptr(B1), ptr(We),
             ptr(tab), *[ptr(t) for t in kept], stream_ptr())
        if grad:
            ctx.save_for_backward(*kept, W0, W1, We, rowptr)
        ctx.rows = E
        ctx.params = (w0, b0, w1, b1, we)
        ctx.fan = _fan_of(x)
        return tab

    @staticmethod
    def backward(ctx, d_tab):
        A, z0, h, g, W0, W1, We, rowptr = ctx.saved_tensors
        d_tab = _f32(d_tab)
        N, D = d_tab.shape
        E = ctx.rows
        f32 = dict(dtype=torch.float32, device=d_tab.device)
        d_g, d_z0 = torch.empty(N, D, **f32), torch.empty(N, D, **f32)
        dx, first = None, True
        if ctx.needs_input_grad[0]:
            if ctx.fan is not None:  # add into the layer input's fan-in buffer
                dx, first = ctx.fan.take((E, D), d_tab.device)
            else:
                dx = torch.empty(E, D, **f32)
        call("x2g_atom_context_bwd", ptr(d_tab), ptr(z0), ptr(rowptr), N, E, D, ptr(W0), ptr(W1), ptr(We), ptr(d_g),
             ptr(d_z0), ptr(dx), 0 if first else 1, stream_ptr())
        w0, b0, w1, b1, we = ctx.params
        rm = TILED_DY_ROWMAJOR | TILED_X_ROWMAJOR
        (dwe, dw1, dw0), (_, db1, db0) = tiled_wgrad([d_tab, d_g, d_z0], [g, h, A], N, [we, w1, w0], [None, b1, b0],
                                                     layouts=[rm, rm, rm])
        return dx if first else None, None, None, dw0, db0, dw1, db1, dwe


def atom_context(x, atom_rowptr, edge_src, edgenn_lin0, edgenn_lin1, lin_edge):
    """SBFTransformerV2's per-layer edge table [N, D] = lin_edge(edgenn_lin1(SiLU(edgenn_lin0(A)))) with
    A = scatter_add(x, edge_src) over the N = len(atom_rowptr) - 1 atoms (reference model.py:138-141 with
    sbftransformer_conv.py:144, per atom instead of per triplet).  ``atom_rowptr``: each atom's out-edge line
    nodes are the contiguous rows [atom_rowptr[a], atom_rowptr[a + 1]) of x; ``edge_src``: the same as an index
    per row (read by the host-tensor form only)."""
    N = int(atom_rowptr.shape[0]) - 1
    lins = [edgenn_lin0, edgenn_lin1, lin_edge]
    if not x.is_cuda:  # modules built and run on a host (Linear.fused's plain nn.Linear math)
        A = torch.zeros(N, x.shape[1], dtype=x.dtype).index_add_(0, edge_src.long(), x)
        return lin_edge(edgenn_lin1(torch.nn.functional.silu(edgenn_lin0(A))))
    if _ATOM_CTX and atom_context_supported(x, lins):
        return _apply(_AtomContextFn, x, _i32(atom_rowptr), N, edgenn_lin0.weight, edgenn_lin0.bias,
                      edgenn_lin1.weight, edgenn_lin1.bias, lin_edge.weight)
    A = segment_sum(x, atom_rowptr, N)
    if _CHAIN and chain_supported(A, lins):
        return row_chain(A, None, lins, [CHAIN_SILU, 0, 0])
    return lin_edge.fused(edgenn_lin1.fused(edgenn_lin0.fused(A, act=ACT_SILU)))


class IndexPlan:
    """A scatter index in any order, prepared on the device without a host read: ``perm`` is the
    stable sort of the keys (sorted position -> source row; equal keys keep the caller's order) and
    ``rowptr`` the CSR row pointer of the sorted keys.  Rows whose key lies outside [0, dim_size)
    belong to no segment (torch_scatter raises for them).  Build once, reuse for every operator
    over the same index (as MessagePassing reuses edge_index[1])."""

    def __init__(self, index, dim_size: int):
        _need_cuda(index)
        idx = _i32(index.reshape(-1))
        self.n, self.dim_size = int(idx.numel()), int(dim_size)
        keys, perm = torch.sort(idx, stable=True)
        self.perm = _i32(perm)
        self.rowptr, _ = csr_rowptr_checked(keys, self.dim_size)


REDUCE_SUM, REDUCE_MEAN = _C["REDUCE_SUM"], _C["REDUCE_MEAN"]


class _ScatterReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, plan, mode):
        x = _f32(src)
        out = torch.empty(plan.dim_size, x.shape[1], dtype=torch.float32, device=x.device)
        call("x2g_segment_reduce_perm", ptr(x), ptr(plan.perm), ptr(plan.rowptr), plan.dim_size, x.shape[1], mode,
             ptr(out), stream_ptr())
        ctx.plan, ctx.mode, ctx.rows = plan, mode, x.shape[0]
        return out

    @staticmethod
    def backward(ctx, g):
        g = _f32(g)
        plan = ctx.plan
        dx = torch.zeros(ctx.rows, g.shape[1], dtype=torch.float32, device=g.device)
        call("x2g_segment_reduce_perm_bwd", ptr(g), ptr(plan.perm), ptr(plan.rowptr), plan.dim_size, g.shape[1],
             ctx.mode, ptr(dx), stream_ptr())
        return dx, None, None


def _plan_rows(src, plan):
    """A prebuilt IndexPlan's row count must be src's: its permutation addresses src's rows."""
    _need_cuda(src)
    if src.shape[0] != plan.n:
        raise ValueError(f"IndexPlan was built for {plan.n} rows, src has {src.shape[0]}")


def _scatter(src, index, dim_size, mode):
    if isinstance(index, IndexPlan):
        _plan_rows(src, index)
        if dim_size is not None and int(dim_size) != index.dim_size:
            raise ValueError(f"dim_size {dim_size} differs from the IndexPlan's {index.dim_size}")
        plan = index
    else:
        _need_cuda(src, index)
        if src.shape[0] != index.numel():
            raise ValueError("scatter: index must hold one key per row of src (dim=0)")
        if dim_size is None:  # torch_scatter's default: index.max() + 1 (a host read)
            dim_size = int(index.max()) + 1 if index.numel() else 0
        plan = IndexPlan(index, int(dim_size))
    squeeze = src.dim() == 1
    x = src.unsqueeze(1) if squeeze else src.reshape(src.shape[0], -1)
    out = _ScatterReduce.apply(x, plan, mode)
    return out.squeeze(1) if squeeze else out.view(plan.dim_size, *src.shape[1:])


def scatter_add(src, index, dim_size: int = None):
    """torch_scatter.scatter_add(src, index, dim=0, dim_size=dim_size) (readout.py:37, model.py:53)
    for ANY index order (or a prebuilt ``IndexPlan``), with no host read (HIP-graph capturable):
    the keys are stably sorted on the device and the segment sum reads src's rows through the
    permutation (x2g_segment_reduce_perm), so each segment is summed in the caller's row order —
    deterministic, no float atomics."""
    return _scatter(src, index, dim_size, REDUCE_SUM)


def scatter_mean(src, index, dim_size: int = None):
    """torch_scatter.scatter_mean(src, index, dim=0, dim_size=dim_size) (readout.py:69, MolWise's
    pool_option='mean'): the segment sum divided by max(count, 1), empty segments 0; any index order,
    no host read."""
    return _scatter(src, index, dim_size, REDUCE_MEAN)


class _SegmentSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, rowptr, n_seg):
        src = _f32(src)
        out = torch.empty_like(src)
        call("x2g_segment_softmax_fwd", ptr(src), ptr(rowptr), n_seg, src.shape[1], ptr(out), stream_ptr())
        ctx.save_for_backward(out, rowptr)
        ctx.n_seg = n_seg
        return out

    @staticmethod
    def backward(ctx, g):
        out, rowptr = ctx.saved_tensors
        g = _f32(g)
        ds = torch.empty_like(out)
        call("x2g_segment_softmax_bwd", ptr(out), ptr(g), ptr(rowptr), ctx.n_seg, out.shape[1], ptr(ds), stream_ptr())
        return ds, None, None


def segment_softmax(src, rowptr, num_segments: int):
    """PyG utils.softmax for a sorted index, [R] or [R, H]."""
    _need_cuda(src, rowptr)
    squeeze = src.dim() == 1
    s = src.unsqueeze(1) if squeeze else src
    out = _SegmentSoftmax.apply(s, _i32(rowptr), int(num_segments))
    return out.squeeze(1) if squeeze else out


class _SoftmaxPerm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, plan):
        x = _f32(src)
        out = torch.empty_like(x)
        call("x2g_segment_softmax_perm_fwd", ptr(x), ptr(plan.perm), ptr(plan.rowptr), plan.dim_size, x.shape[1],
             ptr(out), stream_ptr())
        ctx.save_for_backward(out)
        ctx.plan = plan
        return out

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        plan = ctx.plan
        ds = torch.zeros_like(out)
        call("x2g_segment_softmax_perm_bwd", ptr(out), ptr(_f32(g)), ptr(plan.perm), ptr(plan.rowptr), plan.dim_size,
             out.shape[1], ptr(ds), stream_ptr())
        return ds, None


def softmax(src, index=None, ptr=None, num_nodes=None):
    """torch_geometric.utils.softmax(src, index, ptr, num_nodes) along dim 0
    (sbftransformer_conv.py:151): exp(src - max) / (sum + 1e-16) per group of rows sharing a key.
    ``index`` in any order (or an ``IndexPlan``), or a CSR ``ptr`` of contiguous groups.  With
    neither ``num_nodes`` nor an IndexPlan the group count is ``int(index.max()) + 1`` (a host read,
    as PyG's maybe_num_nodes makes); otherwise nothing is read back."""
    if ptr is not None:
        return segment_softmax(src, ptr, int(ptr.numel()) - 1)
    if index is None:
        raise ValueError("softmax needs index or ptr")
    if isinstance(index, IndexPlan):
        _plan_rows(src, index)
    else:
        _need_cuda(src, index)
        if src.shape[0] != index.numel():
            raise ValueError("softmax: index must hold one key per row of src (dim=0)")
        n = int(num_nodes) if num_nodes is not None else (int(index.max()) + 1 if index.numel() else 0)
        index = IndexPlan(index, n)
    squeeze = src.dim() == 1
    s = src.unsqueeze(1) if squeeze else src
    out = _SoftmaxPerm.apply(s, index)
    return out.squeeze(1) if squeeze else out


class _GraphLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rowptr, n_seg, eps):
        x = _f32(x)
        D = x.shape[1]
        out = torch.empty_like(x)
        mean = torch.empty(n_seg, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        call("x2g_graph_layernorm_fwd", ptr(x), ptr(rowptr), n_seg, D, float(eps), ptr(out), ptr(mean), ptr(rstd),
             stream_ptr())
        ctx.save_for_backward(out, rstd, rowptr)
        ctx.n_seg = n_seg
        return out

    @staticmethod
    def backward(ctx, g):
        out, rstd, rowptr = ctx.saved_tensors
        g = _f32(g)
        dx = torch.empty_like(out)
        wsb = int(_lib.load().x2g_graph_layernorm_bwd_workspace(ctx.n_seg))
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=out.device)
        call("x2g_graph_layernorm_bwd_ex", ptr(out), ptr(g), ptr(rstd), ptr(rowptr), ctx.n_seg, out.shape[1], ptr(dx),
             ptr(ws), wsb, stream_ptr())
        return dx, None, None, None


def graph_layer_norm(x, rowptr, num_segments: int, eps: float = 1e-5):
    """PyG LayerNorm(mode='graph', affine=False) over contiguous row segments."""
    _need_cuda(x, rowptr)
    return _GraphLayerNorm.apply(x, _i32(rowptr), int(num_segments), float(eps))


# ------------------------------------------------------------------------------ loss
class _SmoothL1MeanFn(torch.autograd.Function):
    """F.smooth_l1_loss(pred, target) with reduction='mean' (trainer.py:41) as one launch each way
    (x2g_smooth_l1_mean_fwd / _bwd) instead of torch's elementwise + mean and fill + fill +
    elementwise; the target takes no gradient (the reference's labels)."""

    @staticmethod
    def forward(ctx, pred, target, beta, unit_seed):
        p, t = _f32(pred).reshape(-1), _f32(target).reshape(-1)
        out = torch.empty((), dtype=torch.float32, device=p.device)
        ctx.unit_seed, ctx.dp_unit = unit_seed, None
        if unit_seed is not None:  # the gradient for a backward seeded with `unit_seed` (== 1) in the same pass
            ctx.dp_unit = torch.empty_like(p)
            call("x2g_smooth_l1_mean_fwd_grad", ptr(p), ptr(t), p.numel(), float(beta), ptr(out), ptr(ctx.dp_unit),
                 stream_ptr())
        else:
            call("x2g_smooth_l1_mean_fwd", ptr(p), ptr(t), p.numel(), float(beta), ptr(out), stream_ptr())
        ctx.save_for_backward(p, t)
        ctx.beta, ctx.shape = float(beta), pred.shape
        return out

    @staticmethod
    def backward(ctx, g):
        if ctx.dp_unit is not None and g is ctx.unit_seed:  # autograd hands the caller's seed object through
            return ctx.dp_unit.view(ctx.shape), None, None, None
        p, t = ctx.saved_tensors
        dp = torch.empty_like(p)
        call("x2g_smooth_l1_mean_bwd", ptr(p), ptr(t), p.numel(), ctx.beta, ptr(_f32(g).reshape(1)), ptr(dp),
             stream_ptr())
        return dp.view(ctx.shape), None, None, None


def smooth_l1_loss(pred, target, beta: float = 1.0, unit_seed=None):
    """torch.nn.functional.smooth_l1_loss(pred, target, beta=beta) (mean) on the device path.

    ``unit_seed``: a persistent ones scalar the caller will pass to ``torch.autograd.backward(loss,
    unit_seed)`` (x2gnn.train.Trainer's ``seed``): the forward launch then also writes the gradient for
    that seed, and the backward, handed that very object, returns it without a launch (any other
    gradient takes the backward kernel, so the result is the same either way, bit for bit)."""
    if (not pred.is_cuda or pred.shape != target.shape or pred.numel() == 0 or target.requires_grad
            or beta <= 0):  # beta <= 0 is torch's L1 branch, not compiled
        return torch.nn.functional.smooth_l1_loss(pred, target, beta=beta)
    return _SmoothL1MeanFn.apply(pred, target, beta, unit_seed)


# ------------------------------------------------------------------------------ evaluation metrics
def _acc_ok(acc, least):
    if acc.dtype != torch.float64 or not acc.is_contiguous() or acc.numel() < least:
        raise ValueError(f"the accumulator must be a contiguous float64 tensor of at least {least} elements")


def error_accum(pred, target, acc):
    """Add one batch's error statistics to ``acc`` (float64, >= 4 elements, zeroed by the caller):
    acc[0] += sum |d|, acc[1] += sum d^2, acc[2] = max(acc[2], max |d|), acc[3] += n with d = pred - target
    formed in fp32 and summed in fp64 (trainer.py:57 without its per-batch ``.item()``).  ``pred`` /
    ``target``: contiguous fp32 of equal element count, [B] or [B, 1] alike.  One launch (x2g_error_accum),
    no allocation, nothing read back."""
    _need_cuda(pred, target, acc)
    _acc_ok(acc, 4)
    for t in (pred, target):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("error_accum takes contiguous fp32 predictions and targets")
    if pred.numel() != target.numel():
        raise ValueError(f"{pred.numel()} predictions against {target.numel()} targets")
    call("x2g_error_accum", ptr(pred), ptr(target), pred.numel(), ptr(acc), stream_ptr())


def error_accum_cols(pred, target, acc):
    """``error_accum`` per target: ``pred`` / ``target`` contiguous fp32 [B, K], ``acc`` float64 [K, 4] (zeroed
    by the caller); row k of ``acc`` takes column k's sum |d|, sum d^2, max |d| and count.  One launch
    (x2g_error_accum_cols), no allocation, nothing read back."""
    _need_cuda(pred, target, acc)
    if pred.dim() != 2 or pred.shape != target.shape:
        raise ValueError(f"error_accum_cols takes [B, K] predictions and targets, got {tuple(pred.shape)} and "
                         f"{tuple(target.shape)}")
    K = pred.shape[1]
    _acc_ok(acc, 4 * K)
    for t in (pred, target):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("error_accum_cols takes contiguous fp32 predictions and targets")
    call("x2g_error_accum_cols", ptr(pred), ptr(target), pred.shape[0], K, ptr(acc), stream_ptr())


def weighted_accum(value, weight, acc):
    """acc[0] += weight * value, acc[1] += weight (trainer.py:45: ``loss.item() * num_graphs``, kept on the
    device): ``value`` an fp32 device scalar, ``weight`` a host number, ``acc`` float64 of >= 2 elements.
    One launch (x2g_weighted_accum), no allocation, nothing read back."""
    _need_cuda(value, acc)
    _acc_ok(acc, 2)
    if value.dtype != torch.float32 or value.numel() != 1:
        raise ValueError("weighted_accum takes one fp32 value")
    call("x2g_weighted_accum", ptr(value), float(weight), ptr(acc), stream_ptr())
