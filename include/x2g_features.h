/* The model's input: the [E, 338] edge features of scf.py:50-119 (bi_gen_edge_feature_6) from the overlap and
 * core-Hamiltonian matrices of any integral code (csrc/ao_features.hip).  Compiled into libx2g.so and bound by
 * x2gnn._lib into tables of its own (FEATURES_SIGNATURES / FEATURES_RESTYPES); like x2g_staged.h, x2g_multi.h,
 * x2g_conv.h, x2g_atomctx.h and x2g_train.h it is outside the recorded ABI (x2g_abi_version() and
 * tests/golden/abi18.json describe x2g.h alone).  Functions only.
 *
 * For the edge e = (i, j) of a molecule m and each matrix M of (ovlp, hcore / hcore_div[m]):
 *   B = M[ao_begin[i]:ao_end[i], ao_begin[j]:ao_end[j]]      (r x c, each element rounded to float32 after the
 *                                                             float64 division)
 *   P = zeros(39, 39) with B placed at (0, 2) when (r, c) = (39, 9), at (2, 2) when (r, c) = (9, 9) and at (0, 0)
 *       for every other shape, (9, 39) included: the reference's branch for it is never taken, and the published
 *       weights were trained on what that gives
 *   13 index groups of 0..38, the same for rows and columns:
 *       [0] [1] [2] [3] [4] [5,8) [8,11) [11,14) [14,17) [17,22) [22,27) [27,32) [32,39)
 *   f[a, b] = P[a, b] when a < 5 and b < 5 (both groups one index), otherwise the Frobenius norm of
 *       P[rows(a), cols(b)]: the squares of the float32 values summed in float64, row-major inside the sub-block,
 *       a float64 square root, one rounding to float32
 *   edge_attr[e] = concat(f_ovlp.reshape(169), f_hcore.reshape(169))
 *
 * ovlp and hcore are flat float64: molecule m's [nao, nao] row-major matrix (nao = mol_nao[m]) starts at element
 * mat_start[m] of both.  hcore_div [M] or NULL: every hcore element is divided by hcore_div[m] in float64 (a
 * division, not a product with a reciprocal), as geom_scf_6 divides by the electron count.  ao_begin / ao_end [N]:
 * each atom's AO range, local to its molecule's matrix.  atom_mol [N]: the molecule of each atom (the PyG batch
 * vector).  edge_index [2, E] int64: batch-global atom indices, in any order.
 *
 * Checked on the host before the launch, with nothing written then: a NULL pointer other than hcore_div and stream
 * or a negative count is X2G_EINVAL; E * 338 * 4 >= 2^31 (the 32-bit offsets into edge_attr) is X2G_EUNSUPPORTED;
 * E == 0 is X2G_OK without a launch.
 *
 * Checked by the kernel, which cannot trust the indices it reads.  An edge is invalid when one of its atoms is
 * outside [0, N), the atoms' molecules differ or are outside [0, M), or an atom's AO range is empty, reversed, wider
 * than 39 or outside [0, nao].  No read is made through an invalid edge's indices, and its whole 338-float row is
 * NaN; every other row of the launch is what it would be alone.  mat_start and mol_nao are taken as describing the
 * two flat arrays.
 *
 * One launch: one wave per (edge, matrix), the block staged as float32 in LDS, up to three of the 169 cells per
 * lane.  No host sync, no global state, no atomics: two runs give the same bits, and an edge's row does not depend on
 * what else shares the launch. */
#ifndef X2G_FEATURES_H
#define X2G_FEATURES_H

#include "x2g.h"

#ifdef __cplusplus
extern "C" {
#endif

int x2g_ao_edge_features(const double* ovlp, const double* hcore, const int64_t* mat_start, const int32_t* mol_nao,
                         const double* hcore_div, const int32_t* ao_begin, const int32_t* ao_end,
                         const int32_t* atom_mol, const int64_t* edge_index, int64_t num_mols, int64_t num_atoms,
                         int64_t num_edges, float* edge_attr, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* X2G_FEATURES_H */
