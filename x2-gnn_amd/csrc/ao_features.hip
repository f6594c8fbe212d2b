// The model's edge features from AO matrices (include/x2g_features.h; reference scf.py:50-119).  Per edge (i, j) and
// matrix (overlap, core Hamiltonian): the r x c block of the two atoms' AO ranges, rounded to float32, placed in a
// zero 39 x 39 pad, and 13 x 13 cells of it: the signed element where both index groups are single, a Frobenius norm
// otherwise.  No edge depends on another, the arithmetic is 1521 squares at most, and the cost is the gather of the
// block: one wave per (edge, matrix) reads it with its 64 lanes over the flattened block (a row's doubles in
// consecutive lanes), stages it as float32 in LDS, and each lane then owns up to three of the 169 cells.
//
// The pad is never built.  A cell's rows and columns are clipped to the placed block, so what lies outside it adds
// nothing: the same bits as summing the pad's zeros, and a cell wholly outside is an exact 0.
#include "common.hpp"

#include "../../include/x2g_features.h"

namespace x2g {
namespace {

constexpr int kPad = 39;                    // AOs of a heavy atom in 6-311+G(3df,2p): the pad's side
constexpr int kGroups = 13;                 // 5 s, 4 p, 3 d, 1 f shells
constexpr int kCells = kGroups * kGroups;   // per matrix
constexpr int kRow = 2 * kCells;            // floats per edge
constexpr int kSingles = 5;                 // the s groups: one index each
constexpr int kHyd = 9;                     // AOs of hydrogen (3 s, 2 p): placed at offset 2
constexpr int kHydOffset = 2;
constexpr int kStride = kPad + 2;           // LDS row stride in floats (odd: a column walk changes bank every row)
constexpr int kThreads = 256;               // 4 waves: 2 edges x 2 matrices
constexpr int kEdgesPerBlock = kThreads / kWave / 2;

__constant__ int kGroupStart[kGroups + 1] = {0, 1, 2, 3, 4, 5, 8, 11, 14, 17, 22, 27, 32, 39};

struct AoArgs {
  const double* mat[2];  // ovlp, hcore
  const int64_t* mat_start;
  const int32_t* mol_nao;
  const double* hcore_div;
  const int32_t* ao_begin;
  const int32_t* ao_end;
  const int32_t* atom_mol;
  const int64_t* edge_index;
  float* out;
  int64_t num_mols, num_atoms;
  int num_edges;
};

// an atom's AO range inside a matrix of nao functions
__device__ __forceinline__ bool range_ok(int b, int e, int nao) { return b >= 0 && e > b && e - b <= kPad && e <= nao; }

__global__ __launch_bounds__(kThreads) void ao_edge_features_kernel(const AoArgs a) {
  __shared__ float blk[kThreads / kWave][kPad * kStride];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = uniform(threadIdx.x >> 6);
  const int which = wave & 1;  // 0: ovlp, 1: hcore
  const int e = blockIdx.x * kEdgesPerBlock + (wave >> 1);
  const bool have = e < a.num_edges;
  float* tile = blk[wave];

  // every index is checked before anything is read through it (wave-uniform: scalar loads and branches)
  bool valid = false;
  int r = 0, c = 0;
  if (have) {
    const int64_t ai = a.edge_index[e], aj = a.edge_index[static_cast<int64_t>(a.num_edges) + e];
    if (ai >= 0 && ai < a.num_atoms && aj >= 0 && aj < a.num_atoms) {
      const int m = a.atom_mol[ai];
      if (m == a.atom_mol[aj] && m >= 0 && m < a.num_mols) {
        const int nao = a.mol_nao[m];
        const int bi = a.ao_begin[ai], ei = a.ao_end[ai], bj = a.ao_begin[aj], ej = a.ao_end[aj];
        if (range_ok(bi, ei, nao) && range_ok(bj, ej, nao)) {
          valid = true;
          r = ei - bi;
          c = ej - bj;
          const double* src = a.mat[which] + a.mat_start[m] + static_cast<int64_t>(bi) * nao + bj;
          const bool divide = which == 1 && a.hcore_div != nullptr;
          const double div = divide ? a.hcore_div[m] : 1.0;
          for (int t = lane; t < r * c; t += kWave) {
            const int rr = t / c, cc = t - rr * c;
            double v = src[static_cast<int64_t>(rr) * nao + cc];
            if (divide) v /= div;
            tile[rr * kStride + cc] = static_cast<float>(v);
          }
        }
      }
    }
  }
  __syncthreads();
  if (!have) return;

  float* out = a.out + (static_cast<uint32_t>(e) * kRow + which * kCells);
  if (!valid) {
    for (int k = lane; k < kCells; k += kWave) out[k] = __builtin_nanf("");
    return;
  }
  const int r0 = (r == kHyd && c == kHyd) ? kHydOffset : 0;
  const int c0 = (c == kHyd && (r == kPad || r == kHyd)) ? kHydOffset : 0;
  for (int k = lane; k < kCells; k += kWave) {
    const int ga = k / kGroups, gb = k - ga * kGroups;
    // the cell's rows and columns of the pad, clipped to the block and moved into its coordinates
    const int rlo = max(kGroupStart[ga] - r0, 0), rhi = min(kGroupStart[ga + 1] - r0, r);
    const int clo = max(kGroupStart[gb] - c0, 0), chi = min(kGroupStart[gb + 1] - c0, c);
    float f = 0.f;
    if (ga < kSingles && gb < kSingles) {
      if (rlo < rhi && clo < chi) f = tile[rlo * kStride + clo];
    } else {
      double s = 0.0;
      for (int rr = rlo; rr < rhi; ++rr)
        for (int cc = clo; cc < chi; ++cc) {
          const double v = static_cast<double>(tile[rr * kStride + cc]);
          s += v * v;
        }
      f = static_cast<float>(sqrt(s));
    }
    out[k] = f;
  }
}

}  // namespace
}  // namespace x2g

using namespace x2g;

X2G_API int x2g_ao_edge_features(const double* ovlp, const double* hcore, const int64_t* mat_start,
                                 const int32_t* mol_nao, const double* hcore_div, const int32_t* ao_begin,
                                 const int32_t* ao_end, const int32_t* atom_mol, const int64_t* edge_index,
                                 int64_t num_mols, int64_t num_atoms, int64_t num_edges, float* edge_attr,
                                 void* stream) {
  if (!ovlp || !hcore || !mat_start || !mol_nao || !ao_begin || !ao_end || !atom_mol || !edge_index || !edge_attr ||
      num_mols < 0 || num_atoms < 0 || num_edges < 0)
    return X2G_EINVAL;
  // the kernel's offsets into edge_attr are 32-bit: E * 338 * 4 < 2^31
  if (num_edges > (int64_t(1) << 31) / (kRow * 4)) return X2G_EUNSUPPORTED;
  if (num_edges == 0) return X2G_OK;
  const AoArgs a{{ovlp, hcore}, mat_start, mol_nao, hcore_div, ao_begin, ao_end, atom_mol, edge_index, edge_attr,
                 num_mols, num_atoms, static_cast<int>(num_edges)};
  ao_edge_features_kernel<<<blocks_for(num_edges, kEdgesPerBlock), kThreads, 0, as_stream(stream)>>>(a);
  return last_launch_status();
}
