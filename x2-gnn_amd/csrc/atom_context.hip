// SBFTransformerV2's atom context (reference model.py:138-141, sbftransformer_conv.py:144): per layer the edge term
// of the attention is lin_edge(edgenn(atoms_rep[middle atom])) with atoms_rep = scatter_add of the line nodes over
// their source atoms.  The chain acts row by row, so it runs on the N atom rows:
//   A[a] = sum of atom a's out-edge rows of x,  z0 = A W0^T + b0,  h = SiLU(z0),  g = h W1^T + b1,  tab = g We^T.
// At N ~ 2.3k rows it is launch- and latency-bound: ONE launch each way, a tile of 16 atoms per workgroup (144
// workgroups at config 2), the tile's rows kept in LDS from product to product, the next product's weight slice in
// flight while the current one runs.  The pool is done while the tile is staged (an atom's out-edges are contiguous
// rows), and the backward's broadcast of d_A over those rows closes its launch.  8 waves: wave w owns the 16 output
// features 16w..16w+15 of every product (the layout of table_chain.hip).  Deterministic: fixed orders throughout.
#include "common.hpp"

#include "../../include/x2g_atomctx.h"

namespace x2g {
namespace {

constexpr int kAD = 128;        // feature width
constexpr int kARows = 16;      // atoms per workgroup tile
constexpr int kAThreads = 512;  // 8 waves
constexpr int kAS = 132;        // LDS row stride (floats): conflict-free 16-byte operand reads

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float silu_(float z) { return z / (1.0f + expf(-z)); }
__device__ __forceinline__ float silu_grad_(float z) {
  const float s = 1.0f / (1.0f + expf(-z));
  return s * (1.0f + z * (1.0f - s));
}

__device__ __forceinline__ f4 mfma4(float a, float b, f4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
}

// v_mfma_f32_16x16x4_f32 sweeps over the 16-row tile: lane l = (i = l & 15, g = l >> 4); the contraction index of
// k-step e in 16-group q is 16q + 4g + e, so one 16-byte LDS read per lane and group feeds four MFMAs.  D lane l
// holds rows 4g + e, column i of the wave's 16-column block.

// the wave's slice of W for out = in W^T: W[c][16q + 4g .. + 3], c = 16w + i
__device__ __forceinline__ void load_w(const float* __restrict__ W, int c, int g, f4 (&wv)[8]) {
  const float* p = W + c * kAD + 4 * g;
#pragma unroll
  for (int q = 0; q < 8; ++q) wv[q] = *reinterpret_cast<const f4*>(p + 16 * q);
}

// the wave's slice of W for out = in W: W[16q + 4g + e][c], c = 16w + i (64-byte runs per 16 lanes)
__device__ __forceinline__ void load_wt(const float* __restrict__ W, int c, int g, f4 (&wv)[8]) {
  const float* p = W + 4 * g * kAD + c;
#pragma unroll
  for (int q = 0; q < 8; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e) wv[q][e] = p[(16 * q + e) * kAD];
}

// acc[e] = sum_k in[4g + e][k] * slice(k) for the lane's column
__device__ __forceinline__ f4 tile_product(const float* __restrict__ in, int i, int g, const f4 (&wv)[8]) {
  const float* a = in + i * kAS + 4 * g;
  f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const f4 av = *reinterpret_cast<const f4*>(a + 16 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = mfma4(av[e], wv[q][e], acc);
  }
  return acc;
}

// atom a's row range, clamped into [0, E) (a broken row pointer reads or writes no row outside x / dx)
__device__ __forceinline__ void atom_range(const int32_t* __restrict__ rowptr, int a, int E, int& e0, int& e1) {
  e0 = rowptr[a];
  e1 = rowptr[a + 1];
  e0 = e0 < 0 ? 0 : e0;
  e1 = e1 > E ? E : e1;
}

struct AtomCtxFwdArgs {
  const float* x;
  const int32_t* rowptr;
  const float *w0, *b0, *w1, *b1, *we;
  float *tab, *a_out, *z0, *h, *g;
  int N, E;
};

__global__ void __launch_bounds__(kAThreads) atom_context_fwd_kernel(const AtomCtxFwdArgs a) {
  __shared__ __attribute__((aligned(16))) float Y[3][kARows * kAS];  // A, h, g of the tile
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i = lane & 15, g = lane >> 4, c = 16 * w + i;
  const int a0 = blockIdx.x * kARows, N = a.N;
  f4 wa[8], wb[8];
  load_w(a.w0, c, g, wa);
  const float b0 = a.b0 ? a.b0[c] : 0.0f, b1 = a.b1 ? a.b1[c] : 0.0f;
  {  // the pool while staging: 32 lanes per atom row, 4 features each, the atom's rows ascending
    const int r = tid >> 5, c4 = 4 * (tid & 31), atom = a0 + r;
    f4 s = {0.f, 0.f, 0.f, 0.f};
    if (atom < N) {
      int e0, e1;
      atom_range(a.rowptr, atom, a.E, e0, e1);
      for (int e = e0; e < e1; ++e) s += *reinterpret_cast<const f4*>(a.x + e * kAD + c4);
      if (a.a_out) *reinterpret_cast<f4*>(a.a_out + atom * kAD + c4) = s;
    }
    *reinterpret_cast<f4*>(&Y[0][r * kAS + c4]) = s;
  }
  load_w(a.w1, c, g, wb);
  __syncthreads();
  f4 acc = tile_product(Y[0], i, g, wa);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int r = 4 * g + e;
    const float z = acc[e] + b0, y = silu_(z);
    Y[1][r * kAS + c] = y;
    if (a0 + r < N) {
      if (a.z0) a.z0[(a0 + r) * kAD + c] = z;
      if (a.h) a.h[(a0 + r) * kAD + c] = y;
    }
  }
  load_w(a.we, c, g, wa);
  __syncthreads();
  acc = tile_product(Y[1], i, g, wb);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int r = 4 * g + e;
    const float y = acc[e] + b1;
    Y[2][r * kAS + c] = y;
    if (a0 + r < N && a.g) a.g[(a0 + r) * kAD + c] = y;
  }
  __syncthreads();
  acc = tile_product(Y[2], i, g, wa);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int r = 4 * g + e;
    if (a0 + r < N) a.tab[(a0 + r) * kAD + c] = acc[e];
  }
}

struct AtomCtxBwdArgs {
  const float *d_tab, *z0;
  const int32_t* rowptr;
  const float *w0, *w1, *we;
  float *d_g, *d_z0, *dx;
  int N, E, accumulate;
};

__global__ void __launch_bounds__(kAThreads) atom_context_bwd_kernel(const AtomCtxBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float Y[3][kARows * kAS];  // d_tab (then d_A), d_g, d_z0 of the tile
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i = lane & 15, g = lane >> 4, c = 16 * w + i;
  const int a0 = blockIdx.x * kARows, N = a.N;
  const int sr = tid >> 5, c4 = 4 * (tid & 31), atom = a0 + sr;  // staging / broadcast: 32 lanes per atom row
  f4 wa[8], wb[8];
  load_wt(a.we, c, g, wa);
  {
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if (atom < N) v = *reinterpret_cast<const f4*>(a.d_tab + atom * kAD + c4);
    *reinterpret_cast<f4*>(&Y[0][sr * kAS + c4]) = v;
  }
  float z[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) z[e] = a0 + 4 * g + e < N ? a.z0[(a0 + 4 * g + e) * kAD + c] : 0.0f;
  load_wt(a.w1, c, g, wb);
  __syncthreads();
  f4 acc = tile_product(Y[0], i, g, wa);  // d_g = d_tab We
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int r = 4 * g + e;
    Y[1][r * kAS + c] = acc[e];
    if (a0 + r < N) a.d_g[(a0 + r) * kAD + c] = acc[e];
  }
  load_wt(a.w0, c, g, wa);
  __syncthreads();
  acc = tile_product(Y[1], i, g, wb);  // d_h = d_g W1
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int r = 4 * g + e;
    const float dz = acc[e] * silu_grad_(z[e]);
    Y[2][r * kAS + c] = dz;
    if (a0 + r < N) a.d_z0[(a0 + r) * kAD + c] = dz;
  }
  __syncthreads();  // (every wave has read Y[0] before the barrier above: it is free for d_A)
  acc = tile_product(Y[2], i, g, wa);  // d_A = d_z0 W0
  if (!a.dx) return;
#pragma unroll
  for (int e = 0; e < 4; ++e) Y[0][(4 * g + e) * kAS + c] = acc[e];
  __syncthreads();
  if (atom < N) {  // the pool's adjoint: d_A[a] to every out-edge row of atom a
    const f4 d = *reinterpret_cast<const f4*>(&Y[0][sr * kAS + c4]);
    int e0, e1;
    atom_range(a.rowptr, atom, a.E, e0, e1);
    if (a.accumulate) {
      for (int e = e0; e < e1; ++e) {
        f4* p = reinterpret_cast<f4*>(a.dx + e * kAD + c4);
        *p = *p + d;
      }
    } else {
      for (int e = e0; e < e1; ++e) *reinterpret_cast<f4*>(a.dx + e * kAD + c4) = d;
    }
  }
}

inline bool al16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }
inline bool al4(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }
inline bool rows_fit32(int64_t rows) { return rows * kAD * 4 < (int64_t(1) << 31); }

}  // namespace
}  // namespace x2g

using namespace x2g;

X2G_API int x2g_atom_context_fwd(const float* x, const int32_t* atom_rowptr, int64_t num_atoms, int64_t num_edges,
                                 int32_t dim, const float* w0, const float* b0, const float* w1, const float* b1,
                                 const float* we, float* tab, float* a_out, float* z0, float* h, float* g,
                                 void* stream) {
  if (num_atoms < 0 || num_edges < 0 || !atom_rowptr || !w0 || !w1 || !we || !tab || (num_edges > 0 && !x))
    return X2G_EINVAL;
  if (dim != kAD) return X2G_EUNSUPPORTED;
  if (!al16(x) || !al16(w0) || !al16(w1) || !al16(we) || !al16(tab) || !al16(a_out) || !al16(z0) || !al16(h) ||
      !al16(g) || !al4(atom_rowptr) || !al4(b0) || !al4(b1))
    return X2G_EINVAL;
  if (!rows_fit32(num_atoms) || !rows_fit32(num_edges)) return X2G_EUNSUPPORTED;
  if (num_atoms == 0) return X2G_OK;
  const AtomCtxFwdArgs a{x, atom_rowptr, w0, b0, w1, b1, we, tab, a_out, z0, h, g, static_cast<int>(num_atoms),
                         static_cast<int>(num_edges)};
  atom_context_fwd_kernel<<<blocks_for(num_atoms, kARows), kAThreads, 0, as_stream(stream)>>>(a);
  return last_launch_status();
}

X2G_API int x2g_atom_context_bwd(const float* d_tab, const float* z0, const int32_t* atom_rowptr, int64_t num_atoms,
                                 int64_t num_edges, int32_t dim, const float* w0, const float* w1, const float* we,
                                 float* d_g, float* d_z0, float* dx, int32_t accumulate, void* stream) {
  if (num_atoms < 0 || num_edges < 0 || !d_tab || !z0 || !atom_rowptr || !w0 || !w1 || !we || !d_g || !d_z0)
    return X2G_EINVAL;
  if (dim != kAD) return X2G_EUNSUPPORTED;
  if (!al16(d_tab) || !al16(z0) || !al16(w0) || !al16(w1) || !al16(we) || !al16(d_g) || !al16(d_z0) || !al16(dx) ||
      !al4(atom_rowptr))
    return X2G_EINVAL;
  if (!rows_fit32(num_atoms) || !rows_fit32(num_edges)) return X2G_EUNSUPPORTED;
  if (num_atoms == 0) return X2G_OK;
  const AtomCtxBwdArgs a{d_tab, z0, atom_rowptr, w0, w1, we, d_g, d_z0, num_edges > 0 ? dx : nullptr,
                         static_cast<int>(num_atoms), static_cast<int>(num_edges), accumulate};
  atom_context_bwd_kernel<<<blocks_for(num_atoms, kARows), kAThreads, 0, as_stream(stream)>>>(a);
  return last_launch_status();
}
