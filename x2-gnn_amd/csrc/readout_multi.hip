// The readouts' final Linear(D, K) for K targets on one trunk, all readouts at once (include/x2g_multi.h):
// readout.hip's head kernels with the target count as a run-time argument.  Each 16-byte chunk of an h row is
// loaded once and held in registers for all K targets; the K weight chunks of a readout (<= 16 KiB, read by
// every wave) come through the cache in the forward and from LDS in the backward.  The target loops are fully
// unrolled to kMaxTargets, so the per-target accumulators stay in registers; per-target loads are unconditional
// (clamped index), only the stores and the LDS folds test `k < K`.
// Every sum has a fixed order.  Forward: per lane the chunk's products summed over the readouts (the pooled form: over
// its rows too), one lane butterfly per result, then the bias sum; weight gradients as readout.hip's: per row slot,
// slots in order, then the fixed-order slab sum.
#include "common.hpp"

#include "../../include/x2g_multi.h"

namespace x2g {
namespace {

constexpr int kMaxTargets = 16;
constexpr int kHeadKSplits = 256;

struct HeadKBatch {
  const float* h[X2G_MAX_GROUPS];
  const float* w[X2G_MAX_GROUPS];
  const float* b[X2G_MAX_GROUPS];
  float* dh[X2G_MAX_GROUPS];
};

typedef float f4k __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float dot4(const f4k a, const f4k b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// bs[k] = sum_g b_g[k] in readout order (a readout without a bias: 0); wave-uniform, formed once per thread
__device__ __forceinline__ void bias_sums(const HeadKBatch& b, int G, int K, float (&bs)[kMaxTargets]) {
#pragma unroll
  for (int k = 0; k < kMaxTargets; ++k) {
    float s = 0.f;
    if (k < K)
      for (int g = 0; g < G; ++g) s += b.b[g] ? b.b[g][k] : 0.f;
    bs[k] = s;
  }
}

// out[r, k] = sum_g h_g[r] . w_g[k] + sum_g b_g[k].  64 / LPR rows per wave, one chunk of each row per lane; U rows
// per lane are in flight together so that one weight chunk serves U rows.  Each lane sums its chunk's products over
// the readouts, then ONE lane butterfly per (row, target) instead of one per readout.
template <int LPR>
__global__ void __launch_bounds__(256) heads_k_fwd_kernel(const HeadKBatch b, int G, int64_t R, int K,
                                                          float* __restrict__ out) {
  constexpr int RPW = 64 / LPR;
  constexpr int U = 2;
  const int lane = threadIdx.x & 63, sub = lane % LPR;
  const int64_t nw = static_cast<int64_t>(gridDim.x) * 4;
  float bs[kMaxTargets];
  bias_sums(b, G, K, bs);
  for (int64_t r0 = (static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6)) * (RPW * U) + lane / LPR; r0 < R;
       r0 += nw * (RPW * U)) {
    float acc[U][kMaxTargets];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < kMaxTargets; ++k) acc[u][k] = 0.f;
    for (int g = 0; g < G; ++g) {
      f4k hv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t r = r0 + u * RPW;
        hv[u] = reinterpret_cast<const f4k*>(b.h[g])[(r < R ? r : r0) * LPR + sub];
      }
      // every target's weight chunk loaded unconditionally (a target past K reads target 0's, its sum is never
      // stored): under a `k < K` branch each load waits for the one before it, one cache latency per target
      f4k wv[kMaxTargets];
#pragma unroll
      for (int k = 0; k < kMaxTargets; ++k) wv[k] = reinterpret_cast<const f4k*>(b.w[g])[(k < K ? k : 0) * LPR + sub];
#pragma unroll
      for (int k = 0; k < kMaxTargets; ++k)
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u][k] += dot4(hv[u], wv[k]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = r0 + u * RPW;
#pragma unroll
      for (int k = 0; k < kMaxTargets; ++k) {
        if (k < K) {
          const float v = group_sum<LPR>(acc[u][k]) + bs[k];
          if (sub == 0 && r < R) out[r * K + k] = v;
        }
      }
    }
  }
}

// The same with the per-segment sum fused: one workgroup per segment of rows; wave w takes the segment's rows
// w * RPW .. in turns.  Each lane sums its chunk's products over its rows and the readouts; one wave sum per target
// per segment, the waves' K sums added in wave order, then the segment's rows x the bias sum.
template <int LPR>
__global__ void __launch_bounds__(256) heads_k_pool_fwd_kernel(const HeadKBatch b, int G, int K,
                                                               const int32_t* __restrict__ seg_rowptr,
                                                               int64_t n_seg, float* __restrict__ out) {
  constexpr int RPW = 64 / LPR;
  __shared__ float red[4][kMaxTargets];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, sub = lane % LPR;
  float bs[kMaxTargets];
  bias_sums(b, G, K, bs);
  for (int64_t m = blockIdx.x; m < n_seg; m += gridDim.x) {
    const int r0 = seg_rowptr[m], r1 = seg_rowptr[m + 1];
    float acc[kMaxTargets];
#pragma unroll
    for (int k = 0; k < kMaxTargets; ++k) acc[k] = 0.f;
    for (int r = r0 + wv * RPW + lane / LPR; r < r1; r += 4 * RPW) {
      for (int g = 0; g < G; ++g) {
        const f4k hv = reinterpret_cast<const f4k*>(b.h[g])[static_cast<int64_t>(r) * LPR + sub];
        f4k wk[kMaxTargets];  // (unconditional loads, as in heads_k_fwd_kernel)
#pragma unroll
        for (int k = 0; k < kMaxTargets; ++k) wk[k] = reinterpret_cast<const f4k*>(b.w[g])[(k < K ? k : 0) * LPR + sub];
#pragma unroll
        for (int k = 0; k < kMaxTargets; ++k) acc[k] += dot4(hv, wk[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < kMaxTargets; ++k) {
      if (k < K) {
        const float s = wave64_sum(acc[k]);
        if (lane == 0) red[wv][k] = s;
      }
    }
    __syncthreads();
    if (threadIdx.x < K) {
      const int k = threadIdx.x;
      // (bs is indexed by a constant in every unrolled copy: no scratch)
      float bias = 0.f;
#pragma unroll
      for (int j = 0; j < kMaxTargets; ++j) bias = j == k ? bs[j] : bias;
      out[m * K + k] = (((red[0][k] + red[1][k]) + red[2][k]) + red[3][k]) + static_cast<float>(r1 - r0) * bias;
    }
    __syncthreads();
  }
}

// the segment of row r: the last s with seg_rowptr[s] <= r (segments cover every row)
__device__ __forceinline__ int64_t seg_of_row_k(const int32_t* __restrict__ seg_rowptr, int64_t n_seg, int64_t r) {
  int64_t lo = 0, hi = n_seg;  // seg_rowptr[lo] <= r < seg_rowptr[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (seg_rowptr[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

// Block x owns rows [x * per, (x + 1) * per) of readout blockIdx.y.  Partial slabs of readout g at
// part + g * splits * (K*D + K): splits x [K*D], then splits x [K].  seg_rowptr (or NULL): dout is per segment.
template <int LPR>
__global__ void __launch_bounds__(256) heads_k_bwd_kernel(const float* __restrict__ dout, const HeadKBatch b, int64_t R,
                                                          int K, float* __restrict__ part,
                                                          const int32_t* __restrict__ seg_rowptr, int64_t n_seg) {
  constexpr int RPB = 256 / LPR;
  constexpr int D = 4 * LPR;
  __shared__ f4k wl[kMaxTargets * LPR];  // this readout's weight, [K, D]
  __shared__ f4k red[RPB * LPR];
  __shared__ float redb[RPB];
  const int sub = threadIdx.x % LPR, slot = threadIdx.x / LPR;
  const int64_t per = (R + gridDim.x - 1) / gridDim.x;
  const int64_t lo = per * blockIdx.x, hi = lo + per < R ? lo + per : R;
  const int splits = gridDim.x;
  const int g = blockIdx.y;
  for (int i = threadIdx.x; i < K * LPR; i += 256) wl[i] = reinterpret_cast<const f4k*>(b.w[g])[i];
  __syncthreads();
  f4k aw[kMaxTargets];
  float ab[kMaxTargets];
#pragma unroll
  for (int k = 0; k < kMaxTargets; ++k) {
    aw[k] = f4k{0.f, 0.f, 0.f, 0.f};
    ab[k] = 0.f;
  }
  float* dh = b.dh[g];
  for (int64_t r = lo + slot; r < hi; r += RPB) {
    const f4k hv = reinterpret_cast<const f4k*>(b.h[g])[r * LPR + sub];
    const float* drow = dout + (seg_rowptr ? seg_of_row_k(seg_rowptr, n_seg, r) : r) * K;
    f4k dhv = {0.f, 0.f, 0.f, 0.f};
    float dv[kMaxTargets];  // (unconditional loads; a target past K reads target 0's and adds nothing)
#pragma unroll
    for (int k = 0; k < kMaxTargets; ++k) dv[k] = drow[k < K ? k : 0];
#pragma unroll
    for (int k = 0; k < kMaxTargets; ++k) {
      const float d = k < K ? dv[k] : 0.f;
      aw[k] += hv * d;
      ab[k] += d;
      dhv += wl[(k < K ? k : 0) * LPR + sub] * d;
    }
    if (dh) reinterpret_cast<f4k*>(dh)[r * LPR + sub] = dhv;
  }
  float* pg = part + static_cast<int64_t>(g) * splits * (static_cast<int64_t>(K) * D + K);
  float* pb = pg + static_cast<int64_t>(splits) * K * D;
#pragma unroll
  for (int k = 0; k < kMaxTargets; ++k) {
    if (k < K) {  // (wave-uniform: every thread takes the same barriers)
      red[slot * LPR + sub] = aw[k];
      if (sub == 0) redb[slot] = ab[k];
      __syncthreads();
      if (threadIdx.x < LPR) {
        f4k s = {0.f, 0.f, 0.f, 0.f};
        for (int sl = 0; sl < RPB; ++sl) s += red[sl * LPR + threadIdx.x];
        reinterpret_cast<f4k*>(pg + (static_cast<int64_t>(blockIdx.x) * K + k) * D)[threadIdx.x] = s;
      }
      if (threadIdx.x == 0) {
        float s = 0.f;
        for (int sl = 0; sl < RPB; ++sl) s += redb[sl];
        pb[static_cast<int64_t>(blockIdx.x) * K + k] = s;
      }
      __syncthreads();
    }
  }
}

inline int heads_k_splits(int64_t R) {
  const int64_t want = (R + 31) / 32;
  return static_cast<int>(want < kHeadKSplits ? (want < 1 ? 1 : want) : kHeadKSplits);
}

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// X2G_OK, or the status of the first argument that fails (NULLs before shapes, as the K = 1 entries)
inline int heads_k_check(const float* const* h, const float* const* w, float* const* dh, int G, int D, int K) {
  if (!h || !w) return X2G_EINVAL;
  if (G < 1 || G > X2G_MAX_GROUPS || D % 4 || D < 4 || D > 256 || ((D / 4) & (D / 4 - 1)) || K < 1 ||
      K > kMaxTargets)
    return X2G_EUNSUPPORTED;
  for (int g = 0; g < G; ++g) {
    if (!h[g] || !w[g]) return X2G_EINVAL;
    if (!aligned16(h[g]) || !aligned16(w[g]) || (dh && !aligned16(dh[g]))) return X2G_EUNSUPPORTED;
  }
  return X2G_OK;
}

// per target k (blockIdx.x): error_accum_kernel's sums over the column's n elements, in its order
constexpr int kColThreads = 256;
constexpr int kColWaves = kColThreads / kWave;

__global__ void __launch_bounds__(kColThreads) error_accum_cols_kernel(const float* __restrict__ pred,
                                                                       const float* __restrict__ target, int64_t n,
                                                                       int K, double* __restrict__ acc) {
  __shared__ double red_abs[kColWaves], red_sq[kColWaves];
  __shared__ float red_max[kColWaves];
  const int k = blockIdx.x;
  double s_abs = 0.0, s_sq = 0.0;
  float m = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += kColThreads) {
    const float d = pred[i * K + k] - target[i * K + k];
    const float af = fabsf(d);
    const double a = static_cast<double>(af);
    s_abs += a;
    s_sq += a * a;  // exact in fp64
    m = fmaxf(m, af);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s_abs += __shfl_xor(s_abs, off, kWave);
    s_sq += __shfl_xor(s_sq, off, kWave);
    m = fmaxf(m, __shfl_xor(m, off, kWave));
  }
  if ((threadIdx.x & 63) == 0) {
    red_abs[threadIdx.x >> 6] = s_abs;
    red_sq[threadIdx.x >> 6] = s_sq;
    red_max[threadIdx.x >> 6] = m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t_abs = red_abs[0], t_sq = red_sq[0];
    float t_max = red_max[0];
#pragma unroll
    for (int w = 1; w < kColWaves; ++w) {
      t_abs += red_abs[w];
      t_sq += red_sq[w];
      t_max = fmaxf(t_max, red_max[w]);
    }
    double* a = acc + 4 * k;
    const double prev = a[2], now = static_cast<double>(t_max);
    a[0] += t_abs;
    a[1] += t_sq;
    a[2] = prev > now ? prev : now;
    a[3] += static_cast<double>(n);
  }
}

}  // namespace
}  // namespace x2g

using namespace x2g;

#define X2G_HEADK_DISPATCH(KERNEL, GRID, ...)                                    \
  switch (D / 4) {                                                               \
    case 1: KERNEL<1><<<GRID, 256, 0, st>>>(__VA_ARGS__); break;                 \
    case 2: KERNEL<2><<<GRID, 256, 0, st>>>(__VA_ARGS__); break;                 \
    case 4: KERNEL<4><<<GRID, 256, 0, st>>>(__VA_ARGS__); break;                 \
    case 8: KERNEL<8><<<GRID, 256, 0, st>>>(__VA_ARGS__); break;                 \
    case 16: KERNEL<16><<<GRID, 256, 0, st>>>(__VA_ARGS__); break;               \
    case 32: KERNEL<32><<<GRID, 256, 0, st>>>(__VA_ARGS__); break;               \
    default: KERNEL<64><<<GRID, 256, 0, st>>>(__VA_ARGS__); break;               \
  }

X2G_API int32_t x2g_readout_heads_k_max_targets(void) { return kMaxTargets; }

X2G_API int x2g_readout_heads_k_fwd(const float* const* h, const float* const* w, const float* const* bias,
                                    int32_t G, int64_t R, int32_t D, int32_t K, const int32_t* seg_rowptr,
                                    int64_t n_seg, float* out, void* stream) {
  if (R < 0 || n_seg < 0 || !out) return X2G_EINVAL;
  if (int rc = heads_k_check(h, w, nullptr, G, D, K)) return rc;
  HeadKBatch b{};
  for (int g = 0; g < G; ++g) {
    b.h[g] = h[g];
    b.w[g] = w[g];
    b.b[g] = bias ? bias[g] : nullptr;
  }
  hipStream_t st = as_stream(stream);
  if (seg_rowptr) {
    if (n_seg == 0) return X2G_OK;
    const unsigned grid = static_cast<unsigned>(n_seg < 65535 ? n_seg : 65535);
    X2G_HEADK_DISPATCH(heads_k_pool_fwd_kernel, grid, b, G, K, seg_rowptr, n_seg, out)
    return last_launch_status();
  }
  if (R == 0) return X2G_OK;
  const int64_t waves = (R * (D / 4) + 127) / 128;  // 2 rows per lane group
  const unsigned grid = static_cast<unsigned>((waves + 3) / 4 < 2048 ? (waves + 3) / 4 : 2048);
  X2G_HEADK_DISPATCH(heads_k_fwd_kernel, grid, b, G, R, K, out)
  return last_launch_status();
}

X2G_API int32_t x2g_readout_heads_k_bwd_splits(int64_t R) { return R > 0 ? heads_k_splits(R) : 0; }

X2G_API size_t x2g_readout_heads_k_bwd_workspace(int64_t R, int32_t D, int32_t K, int32_t G) {
  if (R <= 0 || D <= 0 || K <= 0 || G <= 0) return 0;
  return static_cast<size_t>(G) * heads_k_splits(R) * (static_cast<size_t>(K) * D + K) * sizeof(float);
}

X2G_API int x2g_readout_heads_k_bwd(const float* dout, const int32_t* seg_rowptr, int64_t n_seg,
                                    const float* const* h, const float* const* w, float* const* dh,
                                    float* const* dw, float* const* db, int32_t G, int64_t R, int32_t D, int32_t K,
                                    int flags, void* ws, size_t wsb, void* stream) {
  if (R < 0 || n_seg < 0 || !dw) return X2G_EINVAL;
  if (int rc = heads_k_check(h, w, dh, G, D, K)) return rc;
  for (int g = 0; g < G; ++g)
    if (!dw[g]) return X2G_EINVAL;
  if (seg_rowptr && R > 0 && n_seg < 1) return X2G_EINVAL;
  const bool accum = flags & X2G_ACCUM_WGRAD;
  hipStream_t st = as_stream(stream);
  if (R == 0) {
    if (flags & X2G_DEFER_SLAB_SUM) return X2G_EINVAL;
    if (accum) return X2G_OK;
    for (int g = 0; g < G; ++g) {
      hipError_t e = hipMemsetAsync(dw[g], 0, sizeof(float) * K * D, st);
      if (e == hipSuccess && db && db[g]) e = hipMemsetAsync(db[g], 0, sizeof(float) * K, st);
      if (e != hipSuccess) return static_cast<int>(e);
    }
    return X2G_OK;
  }
  if (!dout) return X2G_EINVAL;
  if (!ws || wsb < x2g_readout_heads_k_bwd_workspace(R, D, K, G)) return X2G_EWORKSPACE;
  HeadKBatch b{};
  for (int g = 0; g < G; ++g) {
    b.h[g] = h[g];
    b.w[g] = w[g];
    b.dh[g] = dh ? dh[g] : nullptr;
  }
  const int splits = heads_k_splits(R);
  float* part = static_cast<float*>(ws);
  X2G_HEADK_DISPATCH(heads_k_bwd_kernel, dim3(splits, G), dout, b, R, K, part, seg_rowptr, n_seg)
  if (int rc = last_launch_status()) return rc;
  if (flags & X2G_DEFER_SLAB_SUM) return X2G_OK;
  x2g_slab_job jobs[X2G_MAX_GROUPS];
  const int64_t nw = static_cast<int64_t>(K) * D;
  for (int g = 0; g < G; ++g) {
    float* pg = part + static_cast<int64_t>(g) * splits * (nw + K);
    float* dbg = db ? db[g] : nullptr;
    jobs[g] = x2g_slab_job{pg, dbg ? pg + static_cast<int64_t>(splits) * nw : nullptr, dw[g], dbg, nw, dbg ? K : 0,
                           splits};
  }
  return x2g_slab_sum_batch(jobs, G, accum ? 1 : 0, stream);
}

X2G_API int x2g_error_accum_cols(const float* pred, const float* target, int64_t n, int32_t K, double* acc,
                                 void* stream) {
  if (n <= 0 || !pred || !target || !acc || reinterpret_cast<uintptr_t>(acc) % 8) return X2G_EINVAL;
  if (K < 1 || K > kMaxTargets) return X2G_EUNSUPPORTED;
  error_accum_cols_kernel<<<K, kColThreads, 0, as_stream(stream)>>>(pred, target, n, K, acc);
  return last_launch_status();
}
