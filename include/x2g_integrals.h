/* The overlap matrix S and the core Hamiltonian H of scf.py:27-48 (geom_scf_6: pyscf's get_ovlp() and get_hcore(), no
 * SCF) from geometry and a basis set, on the device (csrc/integrals.hip).  Compiled into libx2g.so and bound by
 * x2gnn._lib into tables of its own (INTEGRALS_SIGNATURES / INTEGRALS_RESTYPES); like x2g_features.h and x2g_graph.h it
 * is outside the recorded ABI (x2g_abi_version() and tests/golden/abi18.json describe x2g.h alone).  Functions only.
 *
 * For a molecule with nuclei at R_C (bohr) and charges Z_C and atom-centred contracted real-spherical Gaussians a, b:
 *   S[a, b] = <a|b>
 *   H[a, b] = <a| -1/2 nabla^2 |b> - sum_C Z_C <a| 1/|r - R_C| |b>      (C: every atom of the same molecule, in order)
 * Everything is float64: inputs, arithmetic and outputs.
 *
 * Conventions (pyscf's, and the layout x2g_features.h assumes).  An atom's shells are ordered by l, stably in file order
 * within one l; a shell holds 2l + 1 real solid harmonics, normalised over the sphere: p as (x, y, z), d and f as
 * m = -l ... l.  A function is  sum_k coef[k] * Y_lm(r - A) * exp(-exp[k] |r - A|^2)  over the shell's primitives, where
 * coef[k] already carries the primitive's radial normalisation, its contraction coefficient and the rescaling that
 * makes S[a, a] = 1 (x2gnn.integrals.Basis prepares it so).  l <= 3.
 *
 * Basis tables.  basis_tab is one int32 array of n_elem + 1 + 3 n_shells + 1 words:
 *   elem_shell [n_elem + 1]   shells of element e: elem_shell[e] .. elem_shell[e + 1]
 *   shell_l    [n_shells]
 *   shell_prim [n_shells + 1] primitives of shell s: shell_prim[s] .. shell_prim[s + 1], indices into prim_exp / prim_coef
 *   shell_ao   [n_shells]     the shell's first function, counted from the atom's first
 * It is given twice with the same contents: basis_tab on the device, which the kernel reads, and basis_tab_host, which
 * the entry point reads for its checks (it makes no host sync, so it cannot read the device's copy).
 * prim_exp / prim_coef [n_prims] float64 on the device.
 *
 * Atoms: atom_pos [N, 3] float64 in bohr; atom_charge [N] int32 (Z_C); atom_elem [N] int32, the element-table index;
 * atom_mol [N] int32; ao_begin [N] int32, the atom's first function inside its molecule's matrix.
 * Molecules: atom_start [M + 1] int64 (the molecule's atoms: the nuclei of its H); mat_start [M] int64 and mol_nao [M]
 * int32: molecule m's [nao, nao] row-major matrix starts at element mat_start[m] of ovlp and of hcore (AOMatrices'
 * flat layout); mat_elems: the length of each of the two arrays.
 * pairs [2, P] int64: batch-global atom indices.
 *
 * For each listed pair (i, j) the nao_i x nao_j blocks of S and H are computed once, for (min, max), and written to
 * (i, j) and, transposed, to (j, i); of a diagonal block (i == j) the upper triangle is computed and mirrored.  The
 * matrices are therefore bitwise symmetric, and a pair listed twice or in both directions writes the same bits.
 * Elements of unlisted blocks are not touched.  hcore is NOT divided by the electron count.
 *
 * Checked on the host before the launch, with nothing written then: a NULL pointer other than stream or a negative
 * count is X2G_EINVAL, and so is a basis table that is not monotone or points outside its arrays; a shell with l > 3,
 * an element with more than 39 functions, or N, n_shells, n_prims or 4 P at or above 2^31 is X2G_EUNSUPPORTED;
 * P == 0 is X2G_OK without a launch.
 *
 * Checked by the kernel, which cannot trust the indices it reads: a pair is skipped, with no read made through its
 * indices, when an atom is outside [0, N), the atoms' molecules differ or are outside [0, M), an element index is
 * outside the table, the molecule's atom range is not inside [0, N], or an atom's AO range or the molecule's matrix
 * lies outside [0, nao] / [0, mat_elems].
 *
 * One launch, four single-wave workgroups per pair (each takes every fourth shell pair).  No host sync, no global
 * state, no atomics: two runs give the same bits, and a block's bits do not depend on what else shares the launch. */
#ifndef X2G_INTEGRALS_H
#define X2G_INTEGRALS_H

#include "x2g.h"

#ifdef __cplusplus
extern "C" {
#endif

int x2g_one_electron_blocks(const int32_t* basis_tab, const int32_t* basis_tab_host, const double* prim_exp,
                            const double* prim_coef, int64_t n_elem, int64_t n_shells, int64_t n_prims,
                            const double* atom_pos, const int32_t* atom_charge, const int32_t* atom_elem,
                            const int32_t* atom_mol, const int32_t* ao_begin, const int64_t* atom_start,
                            const int64_t* mat_start, const int32_t* mol_nao, int64_t num_mols, int64_t num_atoms,
                            int64_t mat_elems, const int64_t* pairs, int64_t num_pairs, double* ovlp, double* hcore,
                            void* stream);

#ifdef __cplusplus
}
#endif

#endif /* X2G_INTEGRALS_H */
