// x2g_batch_assemble: one training batch built on the device from a dataset that lives there.
//
// The dataset is PyG's InMemoryDataset layout on the GPU: every molecule's tensors concatenated, edge_index
// with molecule-local atom ids.  A batch is a list of molecules (any order, repeats allowed); the host sends
// one small int64 block of per-molecule offsets and this launch writes what data.collate and
// _add_device_indices make on the host, gathered from the resident tensors.
//
// All of the traffic is edge_attr (E x 338 floats: 28 MB read and 28 MB written at 128 S160 molecules, the
// rest is under 1 MB), so the launch is a ragged slab copy plus a tail of index work:
//   blocks [0, n_chunks)  each moves one fixed-size chunk of the DESTINATION edge_attr.  The chunk finds the
//                         molecule its first float lies in by binary search over the B + 1 destination edge
//                         offsets (wave-uniform: scalar loads), then walks the slabs that overlap it: one for
//                         nearly every chunk, several where small molecules meet.  Each piece is copied
//                         16 bytes per lane where source and destination agree mod 16, 8 bytes where they
//                         agree mod 8, else float by float (the head up to the first aligned address and
//                         the tail by single floats).  A 338-float row is 1352 B = 8 * 169, so a molecule with
//                         an odd edge count leaves every later slab 8-byte aligned only, on either side.
//   the blocks after      one thread per edge, per atom and per molecule for the index outputs.
// Source offsets are 64-bit end to end (QM9's edge_attr is ~7e9 floats); destination offsets are too.  Every
// output element has exactly one writer: plain vector stores, no atomics.
#include "common.hpp"

namespace x2g {

constexpr int kAsmThreads = 256;
constexpr int kAsmChunk = 4096;  // floats of the destination per copy block (16 KB: 4 x 16 B per lane)

typedef float asm_f4 __attribute__((ext_vector_type(4)));
typedef float asm_f2 __attribute__((ext_vector_type(2)));

// largest b in [0, n) with off[b] * scale <= v (off ascending, off[0] = 0 <= v)
__device__ __forceinline__ int64_t slab_of(const int64_t* __restrict__ off, int64_t n, int64_t scale, int64_t v) {
  int64_t lo = 0, hi = n;  // off[lo] * scale <= v < off[hi] * scale
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] * scale <= v) lo = mid; else hi = mid;
  }
  return lo;
}

// n vectors of type V from src to dst by the whole block, four loads in flight per lane; the source is read
// once and never again (the dataset is far larger than the last-level cache): non-temporal loads
template <typename V>
__device__ __forceinline__ void copy_vec(V* __restrict__ dst, const V* __restrict__ src, int64_t n) {
  int64_t base = 0;
  for (; base + 4 * kAsmThreads <= n; base += 4 * kAsmThreads) {  // whole rounds: no lane is masked
    V v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = __builtin_nontemporal_load(src + base + k * kAsmThreads + threadIdx.x);
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[base + k * kAsmThreads + threadIdx.x] = v[k];
  }
  for (int64_t i = base + threadIdx.x; i < n; i += kAsmThreads) dst[i] = __builtin_nontemporal_load(src + i);
}

// n floats, dst and src 4-byte aligned and otherwise arbitrary (all arguments block-uniform)
__device__ __forceinline__ void copy_piece(float* __restrict__ dst, const float* __restrict__ src, int64_t n) {
  const uintptr_t d = reinterpret_cast<uintptr_t>(dst), s = reinterpret_cast<uintptr_t>(src);
  const int width = ((d ^ s) & 15) == 0 ? 16 : ((d ^ s) & 7) == 0 ? 8 : 4;
  // floats up to the first destination address aligned to `width` (the source is then aligned too)
  int64_t head = static_cast<int64_t>(((width - (d & (width - 1))) & (width - 1)) >> 2);
  if (head > n) head = n;
  const int per = width >> 2;
  const int64_t body = (n - head) / per, tail0 = head + body * per;
  if (static_cast<int64_t>(threadIdx.x) < head) dst[threadIdx.x] = __builtin_nontemporal_load(src + threadIdx.x);
  if (width == 16)
    copy_vec(reinterpret_cast<asm_f4*>(dst + head), reinterpret_cast<const asm_f4*>(src + head), body);
  else if (width == 8)
    copy_vec(reinterpret_cast<asm_f2*>(dst + head), reinterpret_cast<const asm_f2*>(src + head), body);
  else
    copy_vec(dst + head, src + head, body);
  const int64_t t = tail0 + threadIdx.x;  // fewer than 4 floats
  if (t < n) dst[t] = __builtin_nontemporal_load(src + t);
}

struct AssembleArgs {
  // the resident dataset
  const int64_t* x_all;
  const float* pos_all;
  const int64_t* ei_all;
  int64_t ei_stride;  // elements between edge_index row 0 and row 1 (= E_all)
  const float* attr_all;
  int64_t F;
  const float* y_all;
  const int64_t* trips_all;
  // the batch: off = [src atom start (B) | src edge start (B) | molecule id (B) | dst atom offsets (B + 1) |
  // dst edge offsets (B + 1)]
  const int64_t* off;
  int64_t B, N, E;
  int64_t n_chunks;
  // outputs
  int64_t* x;
  float* pos;
  int64_t* batch;
  int64_t* ptr;
  int64_t* ei;
  float* attr;
  int64_t* edge_num;
  float* y;
  int32_t* edge_src;
  int32_t* edge_dst;
  int32_t* src_type;
  int32_t* dst_type;
  int32_t* atom_type;
  int32_t* mol_ptr;
  int32_t* line_ptr;
  int64_t* mol_trips;
};

__global__ __launch_bounds__(kAsmThreads) void batch_assemble_kernel(const AssembleArgs a) {
  const int64_t B = a.B;
  const int64_t* __restrict__ src_atom = a.off;
  const int64_t* __restrict__ src_edge = a.off + B;
  const int64_t* __restrict__ mol_id = a.off + 2 * B;
  const int64_t* __restrict__ atom_off = a.off + 3 * B;
  const int64_t* __restrict__ edge_off = a.off + 4 * B + 1;
  if (static_cast<int64_t>(blockIdx.x) < a.n_chunks) {
    // ---- one chunk of the destination edge_attr (everything here is block-uniform)
    const int64_t F = a.F, total = a.E * F;
    const int64_t c0 = static_cast<int64_t>(blockIdx.x) * kAsmChunk;
    const int64_t c1 = c0 + kAsmChunk < total ? c0 + kAsmChunk : total;
    int64_t m = slab_of(edge_off, B, F, c0);
    for (int64_t lo = c0; lo < c1 && m < B; ++m) {  // (edge_off[B] * F = total >= c1: m < B only guards the reads)
      const int64_t d0 = edge_off[m] * F, d1 = edge_off[m + 1] * F;  // the slab of molecule m in the destination
      const int64_t hi = d1 < c1 ? d1 : c1;
      if (hi > lo) {
        const int64_t s = src_edge[m] * F + (lo - d0);  // 64-bit: ~7e9 floats into the dataset
        copy_piece(a.attr + lo, a.attr_all + s, hi - lo);
        lo = hi;
      }
    }
    return;
  }
  // ---- the index outputs: thread i takes edge i, atom i and molecule i
  const int64_t i = (static_cast<int64_t>(blockIdx.x) - a.n_chunks) * kAsmThreads + threadIdx.x;
  if (i < a.E) {
    const int64_t m = slab_of(edge_off, B, 1, i);
    const int64_t s = src_edge[m] + (i - edge_off[m]);
    const int64_t la = a.ei_all[s], lb = a.ei_all[a.ei_stride + s];  // molecule-local atom ids
    const int64_t shift = atom_off[m], a0 = src_atom[m];
    a.ei[i] = la + shift;
    a.ei[a.E + i] = lb + shift;
    a.edge_src[i] = static_cast<int32_t>(la + shift);
    a.edge_dst[i] = static_cast<int32_t>(lb + shift);
    a.src_type[i] = static_cast<int32_t>(a.x_all[a0 + la]);
    a.dst_type[i] = static_cast<int32_t>(a.x_all[a0 + lb]);
  }
  if (i < a.N) {
    const int64_t m = slab_of(atom_off, B, 1, i);
    const int64_t s = src_atom[m] + (i - atom_off[m]);
    const int64_t z = a.x_all[s];
    a.x[i] = z;
    a.atom_type[i] = static_cast<int32_t>(z);
    a.batch[i] = m;
#pragma unroll
    for (int c = 0; c < 3; ++c) a.pos[3 * i + c] = a.pos_all[3 * s + c];
  }
  if (i <= B) {
    a.ptr[i] = atom_off[i];
    a.mol_ptr[i] = static_cast<int32_t>(atom_off[i]);
    a.line_ptr[i] = static_cast<int32_t>(edge_off[i]);
  }
  if (i < B) {
    a.edge_num[i] = edge_off[i + 1] - edge_off[i];
    if (a.y) a.y[i] = a.y_all[mol_id[i]];
    if (a.mol_trips) a.mol_trips[i] = a.trips_all[mol_id[i]];
  }
}

}  // namespace x2g

using namespace x2g;

X2G_API int x2g_batch_assemble(const int64_t* x_all, const float* atom_pos_all, const int64_t* edge_index_all,
                               int64_t edge_row_stride, const float* edge_attr_all, int32_t num_features,
                               const float* y_all, const int64_t* trips_all, const int64_t* offsets,
                               int64_t num_mols, int64_t num_nodes, int64_t num_edges, int64_t* x, float* atom_pos,
                               int64_t* batch, int64_t* ptr, int64_t* edge_index, float* edge_attr,
                               int64_t* edge_num, float* y, int32_t* edge_src, int32_t* edge_dst,
                               int32_t* src_type, int32_t* dst_type, int32_t* atom_type, int32_t* mol_ptr,
                               int32_t* line_ptr, int64_t* mol_trips, void* stream) {
  const int64_t B = num_mols, N = num_nodes, E = num_edges;
  if (B < 0 || N < 0 || E < 0 || num_features < 0 || edge_row_stride < 0) return X2G_EINVAL;
  if (B == 0) return (N == 0 && E == 0) ? X2G_OK : X2G_EINVAL;  // nothing to assemble: nothing launched
  if (!offsets || !ptr || !mol_ptr || !line_ptr || !edge_num) return X2G_EINVAL;
  if (N > 0 && (!x_all || !atom_pos_all || !x || !atom_pos || !batch || !atom_type)) return X2G_EINVAL;
  if (E > 0 && (!x_all || !edge_index_all || !edge_index || !edge_src || !edge_dst || !src_type || !dst_type))
    return X2G_EINVAL;
  if (!edge_attr_all != !edge_attr || !y_all != !y || !trips_all != !mol_trips) return X2G_EINVAL;
  if (edge_attr && num_features == 0) return X2G_EINVAL;
  // the int32 index forms hold atom and edge ids
  if (N > 0x7fffffff || E > 0x7fffffff || B > 0x7fffffff) return X2G_EUNSUPPORTED;
  const int64_t n_chunks = edge_attr ? (E * num_features + kAsmChunk - 1) / kAsmChunk : 0;
  const int64_t longest = E > N ? (E > B + 1 ? E : B + 1) : (N > B + 1 ? N : B + 1);
  const int64_t blocks = n_chunks + (longest + kAsmThreads - 1) / kAsmThreads;
  if (blocks > 0x7fffffff) return X2G_EUNSUPPORTED;
  AssembleArgs a;
  a.x_all = x_all; a.pos_all = atom_pos_all; a.ei_all = edge_index_all; a.ei_stride = edge_row_stride;
  a.attr_all = edge_attr_all; a.F = num_features; a.y_all = y_all; a.trips_all = trips_all;
  a.off = offsets; a.B = B; a.N = N; a.E = E; a.n_chunks = n_chunks;
  a.x = x; a.pos = atom_pos; a.batch = batch; a.ptr = ptr; a.ei = edge_index; a.attr = edge_attr;
  a.edge_num = edge_num; a.y = y; a.edge_src = edge_src; a.edge_dst = edge_dst; a.src_type = src_type;
  a.dst_type = dst_type; a.atom_type = atom_type; a.mol_ptr = mol_ptr; a.line_ptr = line_ptr;
  a.mol_trips = mol_trips;
  batch_assemble_kernel<<<static_cast<unsigned>(blocks), kAsmThreads, 0, as_stream(stream)>>>(a);
  return last_launch_status();
}
