/* Multi-target entry points of libx2g.so: the readouts' last Linear(D, K) for K targets on one trunk, and the
 * per-target error statistics.  Compiled into the library and bound by x2gnn._lib into tables of their own
 * (MULTI_SIGNATURES / MULTI_RESTYPES); like x2g_staged.h they are outside the recorded ABI (x2g_abi_version()
 * and tests/golden/abi18.json describe x2g.h alone).  Same C subset as x2g_staged.h: functions only, scalar
 * and pointer parameters, no struct, no constant.
 *
 * G readouts ("groups"), K targets, D the head width.  h[g] is [rows, D], w[g] is nn.Linear's [K, D] row-major
 * weight, b[g] is [K] or NULL.  h, w, b, dh, dw, db are HOST arrays of G device pointers, read at the call (as
 * x2g_sbf_project_batch's).  D in 4, 8, 16, .., 256, 1 <= G <= X2G_MAX_GROUPS, 1 <= K <=
 * x2g_readout_heads_k_max_targets(), h / w / dh 16-byte aligned: X2G_EUNSUPPORTED otherwise.  A NULL array, a
 * NULL h[g] / w[g] (dw[g] in the backward), a NULL out or a negative size: X2G_EINVAL.  All of it is checked on
 * the host before any launch, at 0 rows too.  Outputs and workspaces are the caller's; no host sync, no global
 * state, no atomics: every sum has a fixed order, two runs give the same bits. */
#ifndef X2G_MULTI_H
#define X2G_MULTI_H

#include "x2g.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the largest K (16) */
int32_t x2g_readout_heads_k_max_targets(void);

/* seg_rowptr == NULL:  out[r, k] = sum_g (h_g[r, :] . w_g[k, :] + b_g[k]),  out [rows, K]; 0 rows write nothing.
 * seg_rowptr [num_segments + 1] given: the same summed over the rows seg_rowptr[m] .. seg_rowptr[m + 1] of each
 * segment m -> out [num_segments, K] (AtomWise's per-atom outputs under the global add pool, model.py:53, in
 * one launch); an empty segment gives zeros, 0 segments write nothing. */
int x2g_readout_heads_k_fwd(const float* const* h, const float* const* w, const float* const* b,
                            int32_t num_groups, int64_t rows, int32_t dim, int32_t num_targets,
                            const int32_t* seg_rowptr, int64_t num_segments, float* out, void* stream);

size_t x2g_readout_heads_k_bwd_workspace(int64_t rows, int32_t dim, int32_t num_targets, int32_t num_groups);
int32_t x2g_readout_heads_k_bwd_splits(int64_t rows);

/* dout is [rows, K], or [num_segments, K] with seg_rowptr given (row r then takes its segment's row: the
 * segments must cover every row).
 *   dh_g[r, :] = sum_k dout[., k] w_g[k, :]          (dh == NULL or dh[g] == NULL: not wanted)
 *   dw_g[k, :] (+)= sum_r dout[., k] h_g[r, :]       db_g[k] (+)= sum_r dout[., k]   (db or db[g] NULL: no bias)
 * flags: X2G_ACCUM_WGRAD, X2G_DEFER_SLAB_SUM as x2g_readout_head_bwd.  Group g's partials start at
 * g * splits * (K*D + K) floats into the workspace: splits slabs of [K*D], then splits slabs of [K]; they are
 * summed by x2g_slab_sum_batch (n_w = K*D, n_b = K), here or, deferred, by the caller.  0 rows: dw / db are
 * zeroed (X2G_ACCUM_WGRAD: left alone), X2G_DEFER_SLAB_SUM is then X2G_EINVAL. */
int x2g_readout_heads_k_bwd(const float* dout, const int32_t* seg_rowptr, int64_t num_segments,
                            const float* const* h, const float* const* w, float* const* dh, float* const* dw,
                            float* const* db, int32_t num_groups, int64_t rows, int32_t dim, int32_t num_targets,
                            int flags, void* workspace, size_t workspace_bytes, void* stream);

/* x2g_error_accum per target: pred, target [n, K] row-major, acc [K, 4] doubles (8-byte aligned, owned and
 * zeroed by the caller).  With d = pred[i, k] - target[i, k] formed in fp32 and everything after in fp64:
 *   acc[4k] += sum_i |d|   acc[4k + 1] += sum_i d^2   acc[4k + 2] = max(., max_i |d|)   acc[4k + 3] += n
 * One launch, one 256-thread workgroup per target, x2g_error_accum's summation order over i (K = 1 gives its
 * bits).  n <= 0, a NULL pointer or a misaligned acc: X2G_EINVAL; K outside 1 .. 16: X2G_EUNSUPPORTED. */
int x2g_error_accum_cols(const float* pred, const float* target, int64_t n, int32_t num_targets, double* acc,
                         void* stream);

#ifdef __cplusplus
}
#endif

#endif /* X2G_MULTI_H */
