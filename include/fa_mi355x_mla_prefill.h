/*
 * fa_mi355x_mla_prefill.h -- MLA prefill: attention over token-major Q, K and
 * V with no cache in the non-absorbed form of Multi-head Latent Attention
 * (DeepSeek-V2 / V3 / R1, Kimi K2), the other half of the layer whose decode
 * is fa_mi355x_mla.h.  kv_b_proj has expanded the latent to per-head k_nope
 * (128) and v (128) and the 64 RoPE dims are appended to the keys: the score
 * contracts over 192 dims, the value has 128 and the softmax scale is the
 * caller's (the model's 192**-0.5 * mscale**2).  The conventions and status
 * codes are those of fa_mi355x.h, the calling convention that of its
 * fa_attn_varlen_* entries without head_dim and with softmax_scale.
 *
 *   q   [T_q][Hq ][192]   16-bit, token stride q_stride elements (0 = dense)
 *   k   [T_k][Hkv][192]   k = [k_nope (128) | k_pe (64)], token stride k_stride
 *   v   [T_k][Hkv][128]   token stride v_stride
 *   o   [T_q][Hq ][128]   dense, the same 16-bit type
 *   lse [Hq][T_q] fp32 natural log, or NULL
 *
 *   s[i,j]  = softmax_scale * sum_{d<192} q[i,h,d] * k[j,hkv,d],   hkv = h / (Hq/Hkv)
 *   visible : j < nk_b                       (causal = 0)
 *             j <= nk_b - nq_b + i           (causal != 0, bottom-right; i and j
 *                                             count within sequence b)
 *   O[i,h,:] = sum_j softmax_j(s[i,.]) * v[j,hkv,0:128]
 *   LSE[h,i] = log sum_j exp(s[i,j])
 *   a row that sees no key: O = 0, LSE = -inf; rows of no sequence are neither
 *   read nor written.
 *
 * Modes (batch = the number of sequences):
 *   cu_seqlens_q and cu_seqlens_k (device int32[batch + 1]): cross-attention,
 *       sequence b's rows are [cu_q[b], cu_q[b+1]) and its keys [cu_k[b], cu_k[b+1]);
 *   cu_seqlens_q alone: self-attention, the keys' spans are the queries';
 *   neither: uniform [batch][seqlen][H][D], total_q = batch * seqlen_q and
 *       total_k = batch * seqlen_k, and no array is read.
 * The cu arrays are read and clamped on the device (to [0, total_q] and
 * [0, total_k], each entry no smaller than its predecessor's clamp): any
 * contents are memory-safe.  No sync, no workspace, graph-capturable; the grid
 * is sized from shapes alone.
 *
 * Strides are in elements, multiples of 8 and no shorter than one token's
 * heads (heads * 192 for q and k, heads_kv * 128 for v); the byte range of 128
 * q rows and of 64 k / v rows must fit 31 bits.  Within a token the heads of a
 * tensor are exactly one row apart (192 elements for q and k, 128 for v): there
 * is a token stride and no head stride.  v may so be the second half of a
 * per-token buffer [k_nope (Hkv * 128) | v (Hkv * 128)], i.e. [T][2][Hkv][128],
 * passed as v = buf + Hkv * 128 with v_stride = Hkv * 256 and read in place.
 * The per-head interleaved layout [T][Hkv][k_nope 128 | v 128] (kv_b_proj's
 * output under the usual weight order) has a head stride of 256 and CANNOT be
 * expressed: v = buf + 128 with v_stride = Hkv * 256 passes every check here
 * (the entry sees only a pointer and a stride) and reads other heads' k_nope
 * and v as the values of every head >= 1.  Permute the projection's weight
 * rows once so that it writes the two halves, or copy the slice.  A layout
 * that cannot be read in place is never copied by the library.
 *
 * Scores are scaled by softmax_scale in fp32 after the matrix products for
 * both element types, the row sums are fp32 sums of the fp32 exponentials.
 * heads_q % heads_kv == 0 (DeepSeek: equal; GQA / MQA accepted).
 *
 * Statuses, in order: FA_ERR_BAD_SHAPE (a negative batch, heads or total_k;
 * softmax_scale not finite or not > 0; total_q < 0; a stride that is negative,
 * no multiple of 8 or out of range; cu_seqlens_k without cu_seqlens_q; uniform
 * lengths negative or not multiplying out to the totals), FA_OK on an empty
 * problem (batch, heads_q or total_q zero), FA_ERR_BAD_SHAPE (heads_q %
 * heads_kv; a stride shorter than a token; sizes past 31 bits), total_k == 0
 * (O = 0, LSE = -inf: FA_ERR_NULL_POINTER without o), FA_ERR_NULL_POINTER (q,
 * k, v or o), FA_ERR_HIP / FA_ERR_LAUNCH.
 */
#ifndef FA_MI355X_MLA_PREFILL_H
#define FA_MI355X_MLA_PREFILL_H

#include "fa_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int fa_mla_prefill_varlen_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                              int batch, int heads_q, int heads_kv, int total_q, int total_k,
                              long long q_stride, long long k_stride, long long v_stride,
                              const int* cu_seqlens_q, const int* cu_seqlens_k, int seqlen_q,
                              int seqlen_k, int causal, float softmax_scale, void* hip_stream);
int fa_mla_prefill_varlen_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                               int batch, int heads_q, int heads_kv, int total_q, int total_k,
                               long long q_stride, long long k_stride, long long v_stride,
                               const int* cu_seqlens_q, const int* cu_seqlens_k, int seqlen_q,
                               int seqlen_k, int causal, float softmax_scale, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* FA_MI355X_MLA_PREFILL_H */
