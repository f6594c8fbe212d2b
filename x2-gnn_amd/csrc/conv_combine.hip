// SBFTransformerConv's output combine (reference sbftransformer_conv.py:115-127): what follows the attention
// when concat=False or beta=True.  The attention kernels run as they do for root_weight=False (a zero skip row)
// and leave attn [E, H*C]; this row pass does the rest:
//   m    = attn                      (concat)      or   mean over heads of attn.view(H, C)        [Dout]
//   s    = w[0:D].m + w[D:2D].x_r + w[2D:3D].(m - x_r),   beta = 1 / (1 + exp(-s))                (gated)
//   y    = beta x_r + (1 - beta) m   (gated)       or   m + x_r        (x_r NULL: y = m)
// It is memory-bound: a row of W = H*C floats is owned by LPR = W / 4 lanes (one 16-byte load each), the mean
// over heads is a butterfly over the lanes that hold the same channels of different heads, and the gate's dot
// product one sum over the lanes of a head; concat=True is the same code with one "head" of W channels.
// Backward: d_attn, d_xr per row, dw_beta as one partial slab per workgroup (slots summed in order through
// LDS) + the fixed-order slab sum: no atomics.
#include "common.hpp"

#include "../../include/x2g_conv.h"

namespace x2g {

typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int kCombineFwdGrid = 1024;  // forward: workgroups (each strides over tiles of 256 / LPR rows)
constexpr int kCombineSplits = 128;    // backward: workgroups = partial slabs of dw_beta

// Sum over the H = LPR / CL heads of a row: lanes sub, sub + CL, sub + 2 CL, .. hold the same 4 channels of
// different heads; a butterfly over those lane bits (exact xor partners: the lower bits pick the channels and
// must not change) leaves every lane with the total, added in the same order in every lane.
template <int LPR, int CL>
__device__ __forceinline__ f4v head_sum(f4v v) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float a = v[i];
    if constexpr (CL <= 1 && 1 < LPR) a += dpp_mov<0xB1>(a);
    if constexpr (CL <= 2 && 2 < LPR) a += dpp_mov<0x4E>(a);
    if constexpr (CL <= 4 && 4 < LPR) a += __shfl_xor(a, 4, kWave);
    if constexpr (CL <= 8 && 8 < LPR) a += __shfl_xor(a, 8, kWave);
    if constexpr (CL <= 16 && 16 < LPR) a += __shfl_xor(a, 16, kWave);
    if constexpr (CL <= 32 && 32 < LPR) a += __shfl_xor(a, 32, kWave);
    v[i] = a;
  }
  return v;
}

__device__ __forceinline__ float hsum4(f4v v) { return (v[0] + v[1]) + (v[2] + v[3]); }

// the lane's 4 channels of the three blocks of w_beta [3 * Dout] (scalar loads: a parameter may sit at any
// 4-byte offset of a flat buffer); zeros without a gate
template <int CL>
struct BetaW {
  f4v w1, w2, w3;
  __device__ __forceinline__ void load(const float* __restrict__ wb, int cs) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w1[i] = wb ? wb[4 * cs + i] : 0.f;
      w2[i] = wb ? wb[4 * CL + 4 * cs + i] : 0.f;
      w3[i] = wb ? wb[8 * CL + 4 * cs + i] : 0.f;
    }
  }
};

// LPR lanes per attention row (W = 4 LPR), CL lanes per head (C = 4 CL; concat: CL == LPR, one head).  Every
// head's lanes compute the same m, s, beta and y (same operands, same order); the lanes of head 0 store them.
template <int LPR, int CL>
__global__ void __launch_bounds__(256) conv_combine_fwd_kernel(const f4v* __restrict__ attn,
                                                               const f4v* __restrict__ xr,
                                                               const float* __restrict__ wb, int rows,
                                                               f4v* __restrict__ y, float* __restrict__ beta,
                                                               float2* __restrict__ stats) {
  constexpr int RPB = 256 / LPR, H = LPR / CL;
  constexpr float kInvH = 1.0f / H, kInvD = 1.0f / (4 * CL);  // powers of two: exact
  const int sub = threadIdx.x % LPR, slot = threadIdx.x / LPR, cs = sub % CL;
  BetaW<CL> w;
  w.load(wb, cs);
  const int tiles = (rows + RPB - 1) / RPB;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {  // (uniform trip count: the cross-lane sums need every lane)
    const int r = t * RPB + slot;
    const bool ok = r < rows;
    const int rc = ok ? r : rows - 1;
    const f4v a = attn[rc * LPR + sub];
    f4v x = {0.f, 0.f, 0.f, 0.f};
    if (xr) x = xr[rc * CL + cs];
    const f4v m = head_sum<LPR, CL>(a) * kInvH;
    f4v yv;
    if (wb) {
      const f4v d = m - x;
      float p = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) p = fmaf(w.w3[i], d[i], fmaf(w.w2[i], x[i], fmaf(w.w1[i], m[i], p)));
      const float s = group_sum<CL>(p);
      const float b = 1.0f / (1.0f + expf(-s));  // s = -100: exp overflows to inf and b = 0; s = 100: b = 1
      yv = b * x + (1.0f - b) * m;
      if (beta && ok && sub == 0) beta[r] = b;
    } else {
      yv = m + x;
    }
    if (ok && sub < CL) y[r * CL + cs] = yv;
    if (stats) {  // (mean, sum of squared deviations) of the row, x2g_sbf_attention_fwd_stats' format
      const float mu = group_sum<CL>(hsum4(yv)) * kInvD;
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) q = fmaf(yv[i] - mu, yv[i] - mu, q);
      q = group_sum<CL>(q);
      if (ok && sub == 0) stats[r] = make_float2(mu, q);
    }
  }
}

// Backward.  Workgroup b takes the row tiles b, b + splits, ..; its dw_beta partial [3 * Dout] is the sum over
// its tiles per slot, then over the slots in order (LDS), written as slab b of `part`.
template <int LPR, int CL>
__global__ void __launch_bounds__(256) conv_combine_bwd_kernel(const f4v* __restrict__ dy, const f4v* __restrict__ attn,
                                                               const f4v* __restrict__ xr,
                                                               const float* __restrict__ wb,
                                                               const float* __restrict__ beta, int rows,
                                                               f4v* __restrict__ dattn, f4v* __restrict__ dxr,
                                                               float* __restrict__ part) {
  constexpr int RPB = 256 / LPR, H = LPR / CL, DOUT = 4 * CL;
  constexpr float kInvH = 1.0f / H;
  __shared__ float red[RPB * 3 * DOUT];
  const int sub = threadIdx.x % LPR, slot = threadIdx.x / LPR, cs = sub % CL;
  BetaW<CL> w;
  w.load(wb, cs);
  const f4v w13 = w.w1 + w.w3, w23 = w.w2 - w.w3;
  f4v a1 = {0.f, 0.f, 0.f, 0.f}, a2 = a1, a3 = a1;
  const int tiles = (rows + RPB - 1) / RPB;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int r = t * RPB + slot;
    const bool ok = r < rows;
    const int rc = ok ? r : rows - 1;
    const f4v g = dy[rc * CL + cs];
    f4v dm = g, dx = g;
    if (wb) {
      const f4v a = attn[rc * LPR + sub];
      const f4v x = xr[rc * CL + cs];
      const float b = beta[rc];
      const f4v m = head_sum<LPR, CL>(a) * kInvH;
      const f4v d = x - m;
      float p = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) p = fmaf(g[i], d[i], p);
      const float ds = group_sum<CL>(p) * (b * (1.0f - b));
      dm = g * (1.0f - b) + ds * w13;
      dx = g * b + ds * w23;
      const float dsk = ok ? ds : 0.f;
      a1 += dsk * m;
      a2 += dsk * x;
      a3 += dsk * (m - x);
    }
    if (ok && dattn) dattn[r * LPR + sub] = dm * kInvH;
    if (ok && dxr && sub < CL) dxr[r * CL + cs] = dx;
  }
  if (!wb) return;
  if (sub < CL) {
    float* mine = red + slot * 3 * DOUT + 4 * cs;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      mine[i] = a1[i];
      mine[DOUT + i] = a2[i];
      mine[2 * DOUT + i] = a3[i];
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 3 * DOUT; idx += 256) {
    float s = 0.f;
    for (int sl = 0; sl < RPB; ++sl) s += red[sl * 3 * DOUT + idx];
    part[static_cast<int64_t>(blockIdx.x) * 3 * DOUT + idx] = s;
  }
}

// H*C in 32 / 64 / 128 / 256, C in 4 / 8 / 16 / 32 (the destination-major attention kernels' set), H >= 1
inline bool combine_shape_ok(int H, int C) {
  if (H < 1 || !(C == 4 || C == 8 || C == 16 || C == 32)) return false;
  const int64_t W = static_cast<int64_t>(H) * C;
  return W == 32 || W == 64 || W == 128 || W == 256;
}

inline int combine_splits(int64_t rows, int W) {
  const int rpb = 1024 / W;
  const int64_t want = (rows + rpb - 1) / rpb;
  return static_cast<int>(want < kCombineSplits ? (want < 1 ? 1 : want) : kCombineSplits);
}

// kernel(LPR, CL) for W = 4 LPR and a head of 4 CL channels (concat: the whole row)
#define X2G_COMBINE_CL(LPR, cl, LAUNCH)                    \
  switch (cl) {                                            \
    case 1: { constexpr int CL = 1; LAUNCH(LPR, CL); break; } \
    case 2: { constexpr int CL = 2; LAUNCH(LPR, CL); break; } \
    case 4: { constexpr int CL = 4; LAUNCH(LPR, CL); break; } \
    case 8: { constexpr int CL = 8; LAUNCH(LPR, CL); break; } \
    default: { constexpr int CL = LPR; LAUNCH(LPR, CL); break; } \
  }
#define X2G_COMBINE_DISPATCH(lpr, cl, LAUNCH)               \
  switch (lpr) {                                            \
    case 8: X2G_COMBINE_CL(8, cl, LAUNCH) break;            \
    case 16: X2G_COMBINE_CL(16, cl, LAUNCH) break;          \
    case 32: X2G_COMBINE_CL(32, cl, LAUNCH) break;          \
    default: X2G_COMBINE_CL(64, cl, LAUNCH) break;          \
  }

}  // namespace x2g

using namespace x2g;

static inline bool al16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

X2G_API int x2g_conv_combine_fwd(const float* attn, const float* x_r, const float* w_beta, int64_t rows, int32_t heads,
                                 int32_t channels, int32_t concat, float* y, float* beta, float* row_stats,
                                 void* stream) {
  if (rows < 0 || !attn || !y || (w_beta && !x_r)) return X2G_EINVAL;
  if (!combine_shape_ok(heads, channels)) return X2G_EUNSUPPORTED;
  const int W = heads * channels;
  if (!al16(attn) || !al16(y) || !al16(x_r) || reinterpret_cast<uintptr_t>(row_stats) % 8) return X2G_EINVAL;
  if (rows * W * 4 >= (int64_t(1) << 31)) return X2G_EUNSUPPORTED;  // 32-bit row offsets
  if (rows == 0) return X2G_OK;
  const int lpr = W / 4, cl = concat ? lpr : channels / 4, rpb = 256 / lpr;
  const int64_t tiles = (rows + rpb - 1) / rpb;
  const unsigned grid = static_cast<unsigned>(tiles < kCombineFwdGrid ? tiles : kCombineFwdGrid);
  hipStream_t st = as_stream(stream);
#define X2G_LAUNCH(LPR, CL)                                                                                        \
  conv_combine_fwd_kernel<LPR, CL><<<grid, 256, 0, st>>>(reinterpret_cast<const f4v*>(attn),                       \
                                                         reinterpret_cast<const f4v*>(x_r), w_beta,               \
                                                         static_cast<int>(rows), reinterpret_cast<f4v*>(y), beta, \
                                                         reinterpret_cast<float2*>(row_stats))
  X2G_COMBINE_DISPATCH(lpr, cl, X2G_LAUNCH)
#undef X2G_LAUNCH
  return last_launch_status();
}

X2G_API int32_t x2g_conv_combine_splits(int64_t rows, int32_t width) {
  if (rows <= 0 || !(width == 32 || width == 64 || width == 128 || width == 256)) return 0;
  return combine_splits(rows, width);
}

X2G_API size_t x2g_conv_combine_bwd_workspace(int64_t rows, int32_t heads, int32_t channels, int32_t concat) {
  if (rows <= 0 || !combine_shape_ok(heads, channels)) return 0;
  const int W = heads * channels, dout = concat ? W : channels;
  return static_cast<size_t>(combine_splits(rows, W)) * 3 * dout * sizeof(float);
}

X2G_API int x2g_conv_combine_bwd(const float* dy, const float* attn, const float* x_r, const float* w_beta,
                                 const float* beta, int64_t rows, int32_t heads, int32_t channels, int32_t concat,
                                 float* d_attn, float* d_xr, float* dw_beta, int flags, x2g_slab_job* slab_job,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  if (rows < 0 || !dy) return X2G_EINVAL;
  if (w_beta && (!attn || !x_r || !beta || !dw_beta)) return X2G_EINVAL;
  if (flags & ~(X2G_ACCUM_WGRAD | X2G_DEFER_SLAB_SUM)) return X2G_EINVAL;
  if ((flags & X2G_DEFER_SLAB_SUM) && (!slab_job || !w_beta || rows == 0)) return X2G_EINVAL;
  if (!combine_shape_ok(heads, channels)) return X2G_EUNSUPPORTED;
  const int W = heads * channels, dout = concat ? W : channels;
  if (!al16(dy) || !al16(attn) || !al16(x_r) || !al16(d_attn) || !al16(d_xr)) return X2G_EINVAL;
  if (rows * W * 4 >= (int64_t(1) << 31)) return X2G_EUNSUPPORTED;
  hipStream_t st = as_stream(stream);
  const bool accum = flags & X2G_ACCUM_WGRAD;
  if (rows == 0) {
    if (!w_beta || accum) return X2G_OK;
    const hipError_t e = hipMemsetAsync(dw_beta, 0, sizeof(float) * 3 * dout, st);
    return e == hipSuccess ? X2G_OK : static_cast<int>(e);
  }
  if (w_beta && (!workspace || workspace_bytes < x2g_conv_combine_bwd_workspace(rows, heads, channels, concat)))
    return X2G_EWORKSPACE;
  const int lpr = W / 4, cl = concat ? lpr : channels / 4;
  const int splits = combine_splits(rows, W);
  float* part = static_cast<float*>(workspace);
#define X2G_LAUNCH(LPR, CL)                                                                                  \
  conv_combine_bwd_kernel<LPR, CL><<<splits, 256, 0, st>>>(                                                  \
      reinterpret_cast<const f4v*>(dy), reinterpret_cast<const f4v*>(attn), reinterpret_cast<const f4v*>(x_r), \
      w_beta, beta, static_cast<int>(rows), reinterpret_cast<f4v*>(d_attn), reinterpret_cast<f4v*>(d_xr), part)
  X2G_COMBINE_DISPATCH(lpr, cl, X2G_LAUNCH)
#undef X2G_LAUNCH
  if (int rc = last_launch_status()) return rc;
  if (!w_beta) return X2G_OK;
  if (flags & X2G_DEFER_SLAB_SUM) {
    *slab_job = x2g_slab_job{part, nullptr, dw_beta, nullptr, static_cast<int64_t>(3) * dout, 0, splits, 0, 0};
    return X2G_OK;
  }
  return sum_slabs_launch(part, static_cast<int64_t>(3) * dout, nullptr, 0, splits, dw_beta, nullptr, accum, st);
}
