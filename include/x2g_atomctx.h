/* SBFTransformerV2's per-layer atom context (csrc/atom_context.hip; reference model.py:138-141 with
 * sbftransformer_conv.py:144): the edge term of layer i is lin_edge_i(edgenn_i(atoms_rep[atom])) with atoms_rep the
 * sum of each atom's out-edge line nodes.  The index the featurisation yields is the triplet's middle atom, and the
 * MLP and lin_edge act row by row, so the whole chain runs on the N atom rows and the attention reads one table row
 * per center atom.  Compiled into libx2g.so and bound by x2gnn._lib into tables of their own (ATOMCTX_SIGNATURES /
 * ATOMCTX_RESTYPES); like x2g_staged.h, x2g_multi.h and x2g_conv.h they are outside the recorded ABI
 * (x2g_abi_version() and tests/golden/abi18.json describe x2g.h alone).  Functions only.
 *
 * For atoms a in [0, N), atom_rowptr [N + 1] (int32, ascending, atom_rowptr[0] = 0, atom_rowptr[N] = E: each atom's
 * out-edge line nodes are contiguous rows of x [E, 128]):
 *   A[a]   = sum_{e in [atom_rowptr[a], atom_rowptr[a+1])} x[e]        (ascending e; no out-edges: 0)
 *   z0     = A W0^T + b0,   h = SiLU(z0)                               (edgenn[0], SiLU)
 *   g      = h W1^T + b1                                               (edgenn[2])
 *   tab[a] = g We^T                                                    (lin_edge: no bias)
 * W0, W1, We are [128, 128] row-major (torch Linear.weight), b0, b1 [128] or NULL (no bias).
 *
 * Shapes: dim = 128 only, and N * 512 < 2^31, E * 512 < 2^31 (32-bit row offsets): X2G_EUNSUPPORTED otherwise.  A
 * NULL required pointer, negative N or E, or a row tensor / weight not 16-byte aligned (atom_rowptr, b0, b1: 4-byte):
 * X2G_EINVAL.  All of it is checked on the host before any launch; nothing is written then.  A row range of
 * atom_rowptr is clamped to [0, E) before it is used, so no index leaves x / dx whatever the array holds.  One launch
 * each, 16 atoms per workgroup, the three products on v_mfma_f32_16x16x4_f32.  No host sync, no global state, no
 * atomics: two runs give the same bits. */
#ifndef X2G_ATOMCTX_H
#define X2G_ATOMCTX_H

#include "x2g.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tab [N, 128].  a_out, z0, h, g [N, 128] each (optional, for a backward: A, h and g are the row-major x operands of
 * the three weight gradients dW0 = d_z0^T A, dW1 = d_g^T h, dWe = d_tab^T g, and z0 is what SiLU' is taken at; any of
 * them may be NULL).  N == 0: X2G_OK, nothing written.  E == 0 with N > 0: every A row is zero, so tab holds the
 * bias-only row (x may then be NULL). */
int x2g_atom_context_fwd(const float* x, const int32_t* atom_rowptr, int64_t num_atoms, int64_t num_edges, int32_t dim,
                         const float* w0, const float* b0, const float* w1, const float* b1, const float* we,
                         float* tab, float* a_out, float* z0, float* h, float* g, void* stream);

/* From d_tab [N, 128] and the forward's z0:
 *   d_g = d_tab We,   d_h = d_g W1,   d_z0 = d_h * SiLU'(z0),   d_A = d_z0 W0
 *   dx[e] = d_A[a]  (accumulate == 0)   or   dx[e] += d_A[a]  (accumulate != 0)   for e in atom a's row range
 * d_g and d_z0 [N, 128] are left row-major for the weight gradients (dWe = d_tab^T g, dW1 = d_g^T h, db1 = colsum d_g,
 * dW0 = d_z0^T A, db0 = colsum d_z0: jobs of x2g_tiled_wgrad_flat_rows, not formed here).  dx [E, 128] may be NULL
 * (not wanted); rows outside every atom's range are not written.  N == 0: X2G_OK,
 * nothing written.  E == 0 with N > 0: d_g and d_z0 only. */
int x2g_atom_context_bwd(const float* d_tab, const float* z0, const int32_t* atom_rowptr, int64_t num_atoms,
                         int64_t num_edges, int32_t dim, const float* w0, const float* w1, const float* we,
                         float* d_g, float* d_z0, float* dx, int32_t accumulate, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* X2G_ATOMCTX_H */
