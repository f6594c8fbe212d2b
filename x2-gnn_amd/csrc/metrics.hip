// Evaluation metrics kept on the device (trainer.py:45,50 and 52-58 without their per-batch .item()):
// the error statistics of one batch added to a running fp64 accumulator, and a weighted running mean
// of a device scalar.  One launch each, one workgroup, a fixed summation order (deterministic), no
// atomics; the accumulator is read and written by thread 0 alone.
#include "common.hpp"

namespace x2g {
namespace {
constexpr int kMetricThreads = 256;
constexpr int kMetricWaves = kMetricThreads / kWave;

// acc[0] += sum |d|, acc[1] += sum d^2, acc[2] = max(acc[2], max |d|), acc[3] += n; d = pred - target in
// fp32 (as torch forms it), all sums in fp64.  Thread t sums elements t, t + 256, .. in index order, a
// butterfly folds each wave, thread 0 adds the waves in index order.  A thread or wave with no element
// holds 0 for the sums and for the maximum (|d| >= 0, so 0 is its identity here).
__global__ void __launch_bounds__(kMetricThreads) error_accum_kernel(const float* __restrict__ pred,
                                                                     const float* __restrict__ target, int64_t n,
                                                                     double* __restrict__ acc) {
  __shared__ double red_abs[kMetricWaves], red_sq[kMetricWaves];
  __shared__ float red_max[kMetricWaves];
  double s_abs = 0.0, s_sq = 0.0;
  float m = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += kMetricThreads) {
    const float d = pred[i] - target[i];
    const float af = fabsf(d);
    const double a = static_cast<double>(af);
    s_abs += a;
    s_sq += a * a;  // exact in fp64 (24-bit significand squared), so a fused multiply-add rounds the same
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
    for (int w = 1; w < kMetricWaves; ++w) {
      t_abs += red_abs[w];
      t_sq += red_sq[w];
      t_max = fmaxf(t_max, red_max[w]);
    }
    const double prev = acc[2], now = static_cast<double>(t_max);
    acc[0] += t_abs;
    acc[1] += t_sq;
    acc[2] = prev > now ? prev : now;
    acc[3] += static_cast<double>(n);
  }
}

__global__ void __launch_bounds__(kWave) weighted_accum_kernel(const float* __restrict__ value, double weight,
                                                               double* __restrict__ acc) {
  if (threadIdx.x == 0) {
    acc[0] += weight * static_cast<double>(value[0]);
    acc[1] += weight;
  }
}

inline bool acc_ok(const double* acc) { return acc && reinterpret_cast<uintptr_t>(acc) % 8 == 0; }
}  // namespace
}  // namespace x2g

X2G_API int x2g_error_accum(const float* pred, const float* target, int64_t n, double* acc, void* stream) {
  if (n <= 0 || !pred || !target || !x2g::acc_ok(acc)) return X2G_EINVAL;
  x2g::error_accum_kernel<<<1, x2g::kMetricThreads, 0, x2g::as_stream(stream)>>>(pred, target, n, acc);
  return x2g::last_launch_status();
}

X2G_API int x2g_weighted_accum(const float* value, double weight, double* acc, void* stream) {
  if (!value || !x2g::acc_ok(acc)) return X2G_EINVAL;
  x2g::weighted_accum_kernel<<<1, x2g::kWave, 0, x2g::as_stream(stream)>>>(value, weight, acc);
  return x2g::last_launch_status();
}
