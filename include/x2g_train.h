/* The guarded parameter update of libx2g.so (csrc/optim.hip): x2g_clip_adam_ema_ex that decides ON THE DEVICE to
 * skip a step whose gradient norm is not finite, so one bad batch in a long run cannot poison the parameters, both
 * Adam moments and the average for good, and the decision also holds inside a captured HIP graph, where the host
 * cannot look and branch.  Compiled into the library and bound by x2gnn._lib into a table of its own
 * (TRAIN_SIGNATURES / TRAIN_RESTYPES); like x2g_staged.h, x2g_multi.h, x2g_conv.h and x2g_atomctx.h it is outside the
 * recorded ABI (x2g_abi_version() and tests/golden/abi18.json describe x2g.h alone).  Functions only: the scalar
 * block's slots (X2G_OPT_*) and the flag X2G_OPT_ZERO_GRADS are x2g.h's.
 *
 * The gradient norm is formed exactly as x2g_clip_adam_ema_ex forms it: the same 256 partial sums of g^2 in the same
 * order, summed by every workgroup of the second launch in the same order, norm = sqrtf(sum).  Then
 *
 *   norm finite      every output is bit for bit x2g_clip_adam_ema_ex's from the same inputs (params, exp_avg,
 *                    exp_avg_sq, ema, all 16 scalars, and grads under X2G_OPT_ZERO_GRADS); guard[1] = 0.
 *   norm not finite  (inf or NaN: an inf or NaN gradient element, or FINITE gradients whose sum of squares overflows
 *                    fp32, i.e. a norm above about 1.8e19: such a step is skipped too, where the unguarded entry would
 *                    apply a clip coefficient of 0)
 *                    params, exp_avg, exp_avg_sq and ema are not written.  X2G_OPT_STEP, X2G_OPT_LR,
 *                    X2G_OPT_STEP_SIZE and X2G_OPT_BC2_SQRT keep their values: the step is not counted, the
 *                    learning-rate schedule does not advance, and a skipped first step leaves the average's
 *                    first-update copy to the next one.  X2G_OPT_NORM = the norm as computed, X2G_OPT_CLIP = 0.
 *                    grads are still zeroed under X2G_OPT_ZERO_GRADS.  guard[0] += 1, guard[1] = 1.
 *
 * guard: int64 [2] in device memory, owned and zeroed by the caller: [0] the steps skipped so far, [1] whether the
 * last call skipped.  Two launches, as the unguarded entry: the first leaves the tentative step count, learning rate,
 * step size and bias correction in the workspace behind the partials instead of in the scalar block; every workgroup
 * of the second reaches the same verdict from the same partials and reads the tentative values from the workspace,
 * and its workgroup 0 commits them to the scalar block on a finite norm only (no workgroup of that launch reads those
 * slots).  No host read, no fence, no atomics: the call may be captured, and two runs give the same bits.
 *
 * Statuses as x2g_clip_adam_ema_ex (flags other than X2G_OPT_ZERO_GRADS, n < 0, a NULL scalars / params / grads /
 * exp_avg / exp_avg_sq, grads not 16-byte aligned: X2G_EINVAL; a NULL or short workspace: X2G_EWORKSPACE; ema may be
 * NULL); in addition a NULL guard or one not 8-byte aligned is X2G_EINVAL.  All checked on the host before any
 * launch.  n == 0: X2G_OK, nothing is written, guard included. */
#ifndef X2G_TRAIN_H
#define X2G_TRAIN_H

#include "x2g.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace bytes of x2g_clip_adam_ema_guard: the partials and the tentative scalars behind them (0 for n <= 0). */
size_t x2g_optimizer_guard_workspace(int64_t n);

int x2g_clip_adam_ema_guard(float* params, float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                            float* scalars, int flags, int64_t* guard, void* workspace, size_t workspace_bytes,
                            void* stream);

#ifdef __cplusplus
}
#endif

#endif /* X2G_TRAIN_H */
