/* The graph the model's input sits on: the radius graph of atom_graph.py:32-45 (calculate_Dij, gen_bonds_mini) for any
 * number of molecules, built on the device (csrc/radius_graph.hip).  Compiled into libx2g.so and bound by x2gnn._lib
 * into tables of its own (GRAPH_SIGNATURES / GRAPH_RESTYPES); like x2g_features.h and the other headers beside x2g.h
 * it is outside the recorded ABI (x2g_abi_version() and tests/golden/abi18.json describe x2g.h alone).  Functions only.
 *
 * pos float32 [N, 3].  atom_start int64 [M + 1] on the device: molecule m owns the atoms atom_start[m] ..
 * atom_start[m + 1] - 1; empty molecules are allowed.  For an ordered pair of distinct local atoms (i, j) of one
 * molecule, all in float32, every operation rounded once (to nearest even) and nothing reassociated:
 *   g(i, j) = fmaf(z_i, z_j, fmaf(y_i, y_j, x_i * x_j))
 *   d2      = (g(i, i) + g(j, j)) - 2 * g(i, j)
 *   edge    iff  d2 > 0  and  sqrt_rn(d2) < cutoff
 * This is the reference's float32 Gram form, not a difference of coordinates, with its strict "<"; d2 > 0 drops the
 * diagonal, coincident atoms and a d2 that cancellation left negative (NaN in the reference, no edge there either).  A
 * non-finite coordinate gives d2 = inf or NaN for every pair of its atom: no edge.  g(i, j) = g(j, i) bit for bit (a
 * product commutes, the sum order is fixed) and so is g(i, i) + g(j, j): every edge has its reverse.
 *
 * Order: edges sorted by (molecule, i, j), i.e. each molecule's argwhere (row-major) order, the molecules end to end.
 *
 * x2g_radius_graph_count writes
 *   degree         int32 [N]      edges leaving each atom
 *   row_start      int64 [N + 1]  the exclusive scan of degree; row_start[N] = E
 *   mol_edges      int64 [M]      sum of degree over the molecule
 *   mol_triplets   int64 [M]      sum of d (d - 1): the line graph's edges (the graph is symmetric)
 *   mol_max_degree int64 [M]
 *   mol_last_bonded int32 [M]     the highest local atom id with an edge, -1 when the molecule has none
 * with workspace of x2g_radius_graph_count_workspace(N) bytes, 8-byte aligned (the scan's per-tile sums).
 * x2g_radius_graph_fill takes that row_start and the E the host read from row_start[N] and writes edge_local int64
 * [2, E] (molecule-local ids: what a collated dataset stores) and, when edge_global is not NULL, edge_global [2, E]
 * = edge_local + atom_start[m] (what x2g_ao_edge_features takes).
 *
 * Checked on the host before any launch, with nothing written then: a NULL pointer other than edge_global and stream
 * or a negative count is X2G_EINVAL; N >= 2^31 or M >= 2^31 is X2G_EUNSUPPORTED; a workspace smaller than the query's
 * answer is X2G_EWORKSPACE; N == 0 or M == 0 (and, for the fill, E == 0) is X2G_OK without a launch.
 *
 * Checked by the kernels: atom_start is not trusted.  An atom's molecule is found by bisection over atom_start; an
 * atom that the molecule found does not contain within [0, N) has degree 0 and no edge, a molecule whose range is
 * reversed or outside [0, N] has zero counts and -1, and pos is read at atoms of [0, N) only.  The fill writes slot
 * p only when 0 <= p < E, whatever row_start holds.
 *
 * One wave64 per atom row, lanes over j: the count is the popcount of the lanes' ballot, the fill writes at
 * row_start[i] + the popcount of the lower lanes, so a row's edges come out in ascending j without a sort.  No LDS
 * image of a molecule: any molecule size up to N runs.  No atomics at all: the per-molecule outputs are a reduction
 * of degree by one wave per molecule.  Two runs give the same bits, and a molecule's edges do not depend on what else
 * shares the launch. */
#ifndef X2G_GRAPH_H
#define X2G_GRAPH_H

#include "x2g.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t x2g_radius_graph_count_workspace(int64_t num_atoms);

int x2g_radius_graph_count(const float* pos, const int64_t* atom_start, int64_t num_atoms, int64_t num_mols,
                           float cutoff, int32_t* degree, int64_t* row_start, int64_t* mol_edges,
                           int64_t* mol_triplets, int64_t* mol_max_degree, int32_t* mol_last_bonded, void* workspace,
                           size_t workspace_bytes, void* stream);

int x2g_radius_graph_fill(const float* pos, const int64_t* atom_start, const int64_t* row_start, int64_t num_atoms,
                          int64_t num_mols, float cutoff, int64_t num_edges, int64_t* edge_local,
                          int64_t* edge_global, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* X2G_GRAPH_H */
