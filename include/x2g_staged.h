/* Staged entry points of libx2g.so: compiled into the library and bound by x2gnn._lib like x2g.h's
 * (STAGED_SIGNATURES / STAGED_RESTYPES), but not yet part of the recorded ABI (x2g_abi_version() and
 * tests/golden/abi18.json describe x2g.h alone).  They move into x2g.h at the next ABI version.  Same C subset
 * as x2g.h: scalar and pointer parameters, no struct.
 *
 * Attention dropout (reference sbftransformer_conv.py:153: alpha = F.dropout(softmax(...), p, training)).
 *
 * The mask is counter-based: never stored, regenerated identically by the forward and the backward.  All
 * arithmetic is uint32 and wraps; mix(x) is the 32-bit finaliser
 *     x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 * drop_key: two int64 words in DEVICE memory, drop_key[0] = seed, drop_key[1] = step counter (a captured step
 * advances it on the device, so every replay draws a new mask); their bits are read as uint64 and split into
 * lo / hi 32-bit halves.  salt: the conv layer's index.  For triplet row t and head h of H heads:
 *     k0 = mix(seed_lo ^ mix(step_lo ^ (salt * 0x9E3779B9)))
 *     k1 = mix(seed_hi + mix(step_hi ^ k0))
 *     bits(t, h) = mix(mix((t * H + h) ^ k0) + k1)
 *     thr  = min(floor(p * 2^32 + 0.5), 2^32 - 1)        (formed in double, in the entry point)
 *     keep = bits >= thr
 *     r[t, h] = keep ? (float)(1.0 / (1.0 - (double)p)) : 0.0f
 * (t * H + h < 2^32: T * H < 2^28 wherever the center backward runs.)
 *
 * With a_t the softmax weight (the mask enters neither the max nor the denominator), u_t = v_src + e:
 *     out_d    = sum_t a_t r_t u_t S_t + skip_d
 *     g_t      = r_t sum_c dout_d u_t S_t,   rho_d = sum_t a_t g_t,   dlogit_t = a_t (g_t - rho_d)
 *     dv_s    += a_t r_t dout_d S_t,         G_s[l] += a_t r_t dout_d u_t Y_l(t)
 * dq, dk and d_edge follow from dlogit as without dropout; alpha_raw, seg_max, seg_den and the S / P rows are
 * those of the plain entries, bit for bit (one instance excepted: 32 heads without an edge term at degrees 33
 * to 64 runs smaller batches, and its seg_den rounds differently). */
#ifndef X2G_STAGED_H
#define X2G_STAGED_H

#include "x2g.h"

#ifdef __cplusplus
extern "C" {
#endif

/* r_out [T, H] = r[t, h] above (a plain grid-stride kernel: the device statement of the definition, for
 * tests and for callers who want the dropped weights alpha * r).  drop_p outside [0, 1) or a NULL drop_key:
 * X2G_EINVAL; T * H >= 2^32: X2G_EUNSUPPORTED. */
int x2g_attn_dropout_mask(int64_t T, int H, float drop_p, const int64_t* drop_key, uint32_t salt, float* r_out,
                          void* stream);

/* x2g_sbf_attention_fwd_center_sf / _sf_tiled / x2g_sbf_attention_bwd_center (x2g.h) with attention dropout:
 * the parent's arguments and checks, then drop_p in [0, 1) (else X2G_EINVAL; 0 keeps every triplet), drop_key
 * (NULL: X2G_EINVAL) and salt.  The tiled forward runs its storing instance whatever it is asked to store, and
 * takes max_degree <= 64 (X2G_EUNSUPPORTED above: the 8-destinations-per-owner instance cannot hold the mask
 * arithmetic without register spills).
 * The backward takes the P-row form only (sbf_p given): with S rows (sbfproj) it returns X2G_EUNSUPPORTED;
 * it must be given the forward's drop_p, salt and the key's VALUE at the forward. */
int x2g_sbf_attention_fwd_center_sf_drop(const float* q, const float* k, const float* v, const float* skip,
                                         const float* edge, const int32_t* src_row, int edge_mode,
                                         const float* radial, const float* sph_y, const float* w_sbf,
                                         const float* b_sbf, const int32_t* atom_rowptr, const int32_t* edge_rev,
                                         const int32_t* rev_trip, const int32_t* atom_order,
                                         const int32_t* pack_ptr, const int32_t* atom_info, int64_t unit0,
                                         int64_t n_units, int32_t max_rows, int64_t num_edges, int64_t num_triplets,
                                         int32_t heads, int32_t channels, float* out, float* alpha_raw,
                                         float* seg_max, float* seg_den, float* row_stats, float* sbfproj_out,
                                         float* sbf_p_out, void* stream, float drop_p, const int64_t* drop_key,
                                         uint32_t salt);
int x2g_sbf_attention_fwd_center_sf_tiled_drop(const float* q, const float* k, const float* v, const float* skip,
                                               const float* edge, const int32_t* src_row, int edge_mode,
                                               const float* radial, const float* sph_y, const float* w_sbf,
                                               const float* b_sbf, const int32_t* atom_rowptr,
                                               const int32_t* edge_rev, const int32_t* rev_trip,
                                               const int32_t* atom_order, const int32_t* pack_ptr,
                                               const int32_t* atom_info, int64_t unit0, int64_t n_units,
                                               int32_t max_degree, int32_t skip_rows, int64_t num_edges,
                                               int64_t num_triplets, int32_t heads, int32_t channels, float* out,
                                               float* alpha_raw, float* seg_max, float* seg_den, float* row_stats,
                                               float* sbfproj_out, float* sbf_p_out, void* stream, float drop_p,
                                               const int64_t* drop_key, uint32_t salt);
int x2g_sbf_attention_bwd_center_drop(const float* q, const float* k, const float* v, const float* edge,
                                      const int32_t* src_row, int edge_mode, const float* sbfproj,
                                      const float* sbf_p, const float* b_sbf, const float* sph_y,
                                      const int32_t* atom_rowptr, const int32_t* edge_rev, const int32_t* rev_trip,
                                      const int32_t* atom_order, const float* alpha_raw, const float* seg_max,
                                      const float* seg_den, const float* dout, int64_t num_atoms,
                                      int32_t max_degree, int64_t num_edges, int64_t num_triplets, int32_t heads,
                                      int32_t channels, float* dq, float* dk, float* dv, float* radial_grad,
                                      float* d_edge_atom, float* g_work, void* stream, float drop_p,
                                      const int64_t* drop_key, uint32_t salt);

#ifdef __cplusplus
}
#endif

#endif /* X2G_STAGED_H */
