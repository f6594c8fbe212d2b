/* SBFTransformerConv's output combine (csrc/conv_combine.hip): the conv's concat=False and beta=True options
 * (reference sbftransformer_conv.py:58-70 for the parameters, :115-127 for the maths).  Compiled into libx2g.so
 * and bound by x2gnn._lib into tables of their own (CONV_SIGNATURES / CONV_RESTYPES); like x2g_staged.h and
 * x2g_multi.h they are outside the recorded ABI (x2g_abi_version() and tests/golden/abi18.json describe x2g.h
 * alone).  Functions only; the one struct they name, x2g_slab_job, is x2g.h's.
 *
 * The attention kernels run with a zero skip row and leave attn [rows, H*C]; per line-node row e, with
 * Dout = H*C (concat) or C (mean over heads):
 *   m    = attn[e]                            (concat != 0)
 *        = mean over h of attn[e].view(H, C)  (concat == 0)                  sbftransformer_conv.py:115-118
 *   s    = w[0:D] . m + w[D:2D] . x_r + w[2D:3D] . (m - x_r)     (D = Dout; lin_beta: Linear(3 Dout, 1, bias=False)
 *   beta = 1 / (1 + exp(-s))                                      over cat([out, x_r, out - x_r]), :122-123)
 *   y    = beta x_r + (1 - beta) m            (w_beta given, :124)
 *        = m + x_r                            (w_beta NULL, :126;  x_r NULL too: y = m, root_weight=False)
 * exp overflowing (s = -100) gives beta = 0, s = 100 gives beta = 1: finite, no NaN.
 *
 * Shapes: H*C in 32 / 64 / 128 / 256 and C in 4 / 8 / 16 / 32 (the destination-major attention kernels' set),
 * rows * H*C * 4 < 2^31 (32-bit row offsets): X2G_EUNSUPPORTED otherwise.  A NULL required pointer, w_beta with a
 * NULL x_r, negative rows, or attn / x_r / y / dy / d_attn / d_xr not 16-byte (row_stats not 8-byte) aligned:
 * X2G_EINVAL.  All of it is checked on the host before any launch; nothing is written then.  w_beta may sit at
 * any 4-byte alignment.  No host sync, no global state, no atomics: two runs give the same bits. */
#ifndef X2G_CONV_H
#define X2G_CONV_H

#include "x2g.h"

#ifdef __cplusplus
extern "C" {
#endif

/* y [rows, Dout].  beta [rows] (optional, only with w_beta): the gate, kept for the backward.  row_stats
 * [rows, 2] (optional) = (mean over c of y[e, c], sum over c of (y[e, c] - that mean)^2), the format
 * x2g_sbf_attention_fwd_stats writes, so that the graph LayerNorm that follows the conv (model.py:46) stays
 * fused into the next row chain (x2g_chain_fwd_ln).  rows == 0: X2G_OK, nothing written. */
int x2g_conv_combine_fwd(const float* attn, const float* x_r, const float* w_beta, int64_t rows, int32_t heads,
                         int32_t channels, int32_t concat, float* y, float* beta, float* row_stats, void* stream);

/* Partial slabs of dw_beta the backward writes at (rows, width = H*C): 256 / (width / 4) rows per workgroup
 * pass, at most 128 workgroups; 0 for rows <= 0 or an uncompiled width. */
int32_t x2g_conv_combine_splits(int64_t rows, int32_t width);
size_t x2g_conv_combine_bwd_workspace(int64_t rows, int32_t heads, int32_t channels, int32_t concat);

/* From dy [rows, Dout], attn, x_r, w_beta and the forward's beta:
 *   dbeta = sum_c dy_c (x_r - m)_c          ds = dbeta beta (1 - beta)
 *   dm    = dy (1 - beta) + ds (w[0:D] + w[2D:3D])
 *   d_xr  = dy beta + ds (w[D:2D] - w[2D:3D])                                   [rows, Dout]
 *   d_attn = dm (concat) or dm / H broadcast over the heads                     [rows, H*C]
 *   dw_beta[3 Dout] (+)= sum_e ds_e [m, x_r, m - x_r]
 * w_beta NULL (no gate): d_attn = dy (/ H, broadcast), d_xr = dy; attn, x_r, beta, dw_beta, the workspace are
 * then not used.  d_attn / d_xr may be NULL (not wanted).  dw_beta: one partial slab [3 Dout] per workgroup at
 * the start of the workspace (x2g_conv_combine_splits of them), summed in a fixed order; flags X2G_ACCUM_WGRAD
 * and X2G_DEFER_SLAB_SUM as x2g_rbf_gate_bwd's, the deferred form filling *slab_job (non-NULL then) for
 * x2g_slab_sum_batch instead of summing.  rows == 0: dw_beta is zeroed (X2G_ACCUM_WGRAD: left as it is) and
 * nothing else is written; X2G_DEFER_SLAB_SUM is then X2G_EINVAL.  A workspace that is NULL or too small:
 * X2G_EWORKSPACE. */
int x2g_conv_combine_bwd(const float* dy, const float* attn, const float* x_r, const float* w_beta,
                         const float* beta, int64_t rows, int32_t heads, int32_t channels, int32_t concat,
                         float* d_attn, float* d_xr, float* dw_beta, int flags, x2g_slab_job* slab_job,
                         void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* X2G_CONV_H */
