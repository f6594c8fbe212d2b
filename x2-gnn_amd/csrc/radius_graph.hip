// The radius graph on the device (include/x2g_graph.h; reference atom_graph.py:32-45): which ordered pairs of a
// molecule's atoms are closer than the cutoff, in the reference's float32 Gram form, as edge lists in argwhere order
// with the per-atom and per-molecule counts the dataset caches.
//
// One wave per atom row i, its 64 lanes over the molecule's atoms j in steps of 64.  The count kernel adds the
// popcount of each step's ballot; after an exclusive scan of the degrees the fill kernel evaluates the same predicate
// again and writes lane j's edge at row_start[i] + (edges of the steps before) + (set ballot bits below the lane):
// ascending j inside the row, rows in atom order, no sort and no atomics.  Positions are read from global memory (a
// molecule's 12 n bytes stay in L2 across its n rows), so no LDS image bounds the molecule size.
#include "common.hpp"

#include "../../include/x2g_graph.h"

namespace x2g {
namespace {

constexpr int kThreads = 256;
constexpr int kRows = kThreads / kWave;      // atom rows (count, fill) or molecules (stats) per workgroup
constexpr int kScanItems = 8;                // consecutive degrees per thread of the scan
constexpr int kScanTile = kThreads * kScanItems;
constexpr int64_t kMaxCount = int64_t(1) << 31;

struct Vec3 {
  float x, y, z;
};

__device__ __forceinline__ Vec3 load3(const float* pos, int64_t atom) {
  const float* p = pos + atom * 3;
  return {p[0], p[1], p[2]};
}

// g(i, j) of the header: the same bits for (i, j) and (j, i)
__device__ __forceinline__ float gram(const Vec3& a, const Vec3& b) {
  return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x));
}

// The edge test.  The square root goes through float64: the root of a float32 taken in float64 and rounded to
// float32 is the correctly rounded float32 root (53 >= 2 * 24 + 2 bits), whatever the build's fast-math settings
// make of sqrtf.
__device__ __forceinline__ bool bonded(float gii, float gjj, float gij, float cutoff) {
#pragma clang fp contract(off)
  const float d2 = (gii + gjj) - 2.0f * gij;
  return d2 > 0.f && static_cast<float>(sqrt(static_cast<double>(d2))) < cutoff;
}

// The atom range [lo, hi) of the molecule that owns atom a (wave-uniform: scalar loads): bisection for the last m
// with atom_start[m] <= a.  atom_start is not trusted: false unless 0 <= lo <= a < hi <= N.
__device__ __forceinline__ bool molecule_of(const int64_t* atom_start, int64_t M, int64_t N, int64_t a, int64_t& lo,
                                            int64_t& hi) {
  int64_t l = 0, h = M;
  while (h - l > 1) {
    const int64_t mid = l + ((h - l) >> 1);
    if (atom_start[mid] <= a) l = mid; else h = mid;
  }
  lo = atom_start[l];
  hi = atom_start[l + 1];
  return lo >= 0 && lo <= a && a < hi && hi <= N;
}

__device__ __forceinline__ int64_t wave_row(int per_block) {
  return static_cast<int64_t>(blockIdx.x) * per_block + uniform(threadIdx.x >> 6);
}

// ballot of "lane's atom j is bonded to atom a" for the 64 atoms from j0 (lanes beyond hi: 0)
__device__ __forceinline__ unsigned long long row_step(const float* pos, const Vec3& pa, float gaa, int64_t a,
                                                       int64_t j, int64_t hi, float cutoff) {
  const bool in = j < hi;
  const Vec3 pj = load3(pos, in ? j : a);  // (a clamped lane reads the row's own atom: always inside [0, N))
  return __ballot(in && j != a && bonded(gaa, gram(pj, pj), gram(pa, pj), cutoff));
}

__global__ __launch_bounds__(kThreads) void radius_count_kernel(const float* pos, const int64_t* atom_start, int64_t M,
                                                                int64_t N, float cutoff, int32_t* degree) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t a = wave_row(kRows);
  if (a >= N) return;
  int64_t lo, hi;
  int count = 0;
  if (molecule_of(atom_start, M, N, a, lo, hi)) {
    const Vec3 pa = load3(pos, a);
    const float gaa = gram(pa, pa);
    for (int64_t j0 = lo; j0 < hi; j0 += kWave) count += __popcll(row_step(pos, pa, gaa, a, j0 + lane, hi, cutoff));
  }
  if (lane == 0) degree[a] = count;
}

__global__ __launch_bounds__(kThreads) void radius_fill_kernel(const float* pos, const int64_t* atom_start,
                                                               const int64_t* row_start, int64_t M, int64_t N,
                                                               float cutoff, int64_t E, int64_t* edge_local,
                                                               int64_t* edge_global) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t a = wave_row(kRows);
  if (a >= N) return;
  int64_t lo, hi;
  if (!molecule_of(atom_start, M, N, a, lo, hi)) return;
  const Vec3 pa = load3(pos, a);
  const float gaa = gram(pa, pa);
  const unsigned long long below = (1ull << lane) - 1ull;
  int64_t at = row_start[a];
  for (int64_t j0 = lo; j0 < hi; j0 += kWave) {
    const int64_t j = j0 + lane;
    const unsigned long long mask = row_step(pos, pa, gaa, a, j, hi, cutoff);
    const int64_t p = at + __popcll(mask & below);
    if (((mask >> lane) & 1ull) && p >= 0 && p < E) {  // never at or beyond E, whatever row_start holds
      edge_local[p] = a - lo;
      edge_local[E + p] = j - lo;
      if (edge_global) {
        edge_global[p] = a;
        edge_global[E + p] = j;
      }
    }
    at += __popcll(mask);
  }
}

// ------------------------------------------------------------------------------------------------ the scan
__device__ __forceinline__ int64_t wave_inclusive_scan(int64_t v, int lane) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int64_t t = __shfl_up(v, off, kWave);
    if (lane >= off) v += t;
  }
  return v;
}

// exclusive prefix of v over the workgroup's threads, and the workgroup's total; `tot`: kRows words of LDS
__device__ __forceinline__ int64_t block_exclusive_scan(int64_t v, int64_t* tot, int64_t& total) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int64_t inc = wave_inclusive_scan(v, lane);
  __syncthreads();  // (the words may still be read from the call before)
  if (lane == kWave - 1) tot[wave] = inc;
  __syncthreads();
  int64_t before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kRows; ++w) {
    const int64_t t = tot[w];
    if (w < wave) before += t;
    total += t;
  }
  return before + inc - v;
}

// tile_sum[b] = sum of the degrees of tile b (the scan runs over N + 1 slots; slot N holds no degree)
__global__ __launch_bounds__(kThreads) void scan_tile_sums_kernel(const int32_t* degree, int64_t N, int64_t* tile_sum) {
  __shared__ int64_t tot[kRows];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kScanTile;
  int64_t s = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    const int64_t i = base + k * kThreads + threadIdx.x;
    if (i < N) s += degree[i];
  }
  int64_t total;
  block_exclusive_scan(s, tot, total);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// tile_sum -> its exclusive prefix, in place: one workgroup, kThreads tiles per pass with a running carry
__global__ __launch_bounds__(kThreads) void scan_tile_prefix_kernel(int64_t* tile_sum, int64_t tiles) {
  __shared__ int64_t tot[kRows];
  int64_t carry = 0;
  for (int64_t base = 0; base < tiles; base += kThreads) {
    const int64_t i = base + threadIdx.x;
    const int64_t v = i < tiles ? tile_sum[i] : 0;
    int64_t total;
    const int64_t ex = block_exclusive_scan(v, tot, total);
    if (i < tiles) tile_sum[i] = carry + ex;
    carry += total;
  }
}

// row_start[i] for the slots i <= N of tile b: tile_prefix[b] (0 when there is one tile) + the prefix inside it
__global__ __launch_bounds__(kThreads) void scan_write_kernel(const int32_t* degree, int64_t N,
                                                              const int64_t* tile_prefix, int64_t* row_start) {
  __shared__ int64_t tot[kRows];
  const int64_t first = static_cast<int64_t>(blockIdx.x) * kScanTile + threadIdx.x * kScanItems;
  int32_t d[kScanItems];
  int64_t s = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    d[k] = first + k < N ? degree[first + k] : 0;
    s += d[k];
  }
  int64_t total;
  int64_t run = block_exclusive_scan(s, tot, total) + (tile_prefix ? tile_prefix[blockIdx.x] : 0);
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (first + k <= N) row_start[first + k] = run;
    run += d[k];
  }
}

// ------------------------------------------------------------------------------------------------ per molecule
__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, kWave));
  return v;
}

// one wave per molecule over its atoms' degrees (integers: the result does not depend on the order of the sum)
__global__ __launch_bounds__(kThreads) void molecule_counts_kernel(const int32_t* degree, const int64_t* atom_start,
                                                                   int64_t M, int64_t N, int64_t* mol_edges,
                                                                   int64_t* mol_triplets, int64_t* mol_max_degree,
                                                                   int32_t* mol_last_bonded) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t m = wave_row(kRows);
  if (m >= M) return;
  const int64_t lo = atom_start[m], hi = atom_start[m + 1];
  int64_t edges = 0, trips = 0;
  int top = 0, last = -1;
  if (lo >= 0 && lo <= hi && hi <= N) {
    for (int64_t j = lo + lane; j < hi; j += kWave) {
      const int d = degree[j];
      edges += d;
      trips += static_cast<int64_t>(d) * (d - 1);
      top = max(top, d);
      if (d > 0) last = static_cast<int>(j - lo);
    }
  }
  edges = wave_sum(edges);
  trips = wave_sum(trips);
  top = wave_max(top);
  last = wave_max(last);
  if (lane == 0) {
    mol_edges[m] = edges;
    mol_triplets[m] = trips;
    mol_max_degree[m] = top;
    mol_last_bonded[m] = last;
  }
}

inline int64_t scan_tiles(int64_t num_atoms) { return (num_atoms + 1 + kScanTile - 1) / kScanTile; }

}  // namespace
}  // namespace x2g

using namespace x2g;

X2G_API size_t x2g_radius_graph_count_workspace(int64_t num_atoms) {
  if (num_atoms <= 0 || num_atoms >= kMaxCount) return 0;
  return static_cast<size_t>(scan_tiles(num_atoms)) * sizeof(int64_t);
}

X2G_API int x2g_radius_graph_count(const float* pos, const int64_t* atom_start, int64_t num_atoms, int64_t num_mols,
                                   float cutoff, int32_t* degree, int64_t* row_start, int64_t* mol_edges,
                                   int64_t* mol_triplets, int64_t* mol_max_degree, int32_t* mol_last_bonded,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  if (!pos || !atom_start || !degree || !row_start || !mol_edges || !mol_triplets || !mol_max_degree ||
      !mol_last_bonded || !workspace || num_atoms < 0 || num_mols < 0)
    return X2G_EINVAL;
  // one wave per atom and per molecule, four to a workgroup; the atom ids inside the kernels are 64-bit
  if (num_atoms >= kMaxCount || num_mols >= kMaxCount) return X2G_EUNSUPPORTED;
  if (num_atoms == 0 || num_mols == 0) return X2G_OK;
  if (workspace_bytes < x2g_radius_graph_count_workspace(num_atoms)) return X2G_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  radius_count_kernel<<<blocks_for(num_atoms, kRows), kThreads, 0, st>>>(pos, atom_start, num_mols, num_atoms, cutoff,
                                                                         degree);
  const int64_t tiles = scan_tiles(num_atoms);
  int64_t* tile_sum = static_cast<int64_t*>(workspace);
  if (tiles > 1) {
    scan_tile_sums_kernel<<<static_cast<unsigned>(tiles), kThreads, 0, st>>>(degree, num_atoms, tile_sum);
    scan_tile_prefix_kernel<<<1, kThreads, 0, st>>>(tile_sum, tiles);
  }
  scan_write_kernel<<<static_cast<unsigned>(tiles), kThreads, 0, st>>>(degree, num_atoms,
                                                                       tiles > 1 ? tile_sum : nullptr, row_start);
  molecule_counts_kernel<<<blocks_for(num_mols, kRows), kThreads, 0, st>>>(
      degree, atom_start, num_mols, num_atoms, mol_edges, mol_triplets, mol_max_degree, mol_last_bonded);
  return last_launch_status();
}

X2G_API int x2g_radius_graph_fill(const float* pos, const int64_t* atom_start, const int64_t* row_start,
                                  int64_t num_atoms, int64_t num_mols, float cutoff, int64_t num_edges,
                                  int64_t* edge_local, int64_t* edge_global, void* stream) {
  if (!pos || !atom_start || !row_start || !edge_local || num_atoms < 0 || num_mols < 0 || num_edges < 0)
    return X2G_EINVAL;
  if (num_atoms >= kMaxCount || num_mols >= kMaxCount) return X2G_EUNSUPPORTED;
  if (num_atoms == 0 || num_mols == 0 || num_edges == 0) return X2G_OK;
  radius_fill_kernel<<<blocks_for(num_atoms, kRows), kThreads, 0, as_stream(stream)>>>(
      pos, atom_start, row_start, num_mols, num_atoms, cutoff, num_edges, edge_local, edge_global);
  return last_launch_status();
}
