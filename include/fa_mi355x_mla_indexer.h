/*
 * fa_mi355x_mla_indexer.h -- the MLA sparse indexer (DeepSeek-V3.2's DSA): the
 * index logits of every query token over a flat pool of index keys, and the
 * selection of each token's top-k rows, written as the int32 lists of flat pool
 * rows that fa_mi355x_mla_sparse.h reads.  The conventions and the status codes
 * are those of fa_mi355x.h.
 *
 * 1. Index logits: fa_mla_indexer_logits[_k8]_{f16,bf16}
 *
 *   q        [num_tokens][64][128]  16-bit, contiguous: 64 index heads of 128
 *            dims (V3.2's); `heads` must be 64
 *   k        [num_rows][128]  a flat pool of index keys: the same 16-bit type,
 *            or for the _k8 entries E4M3 bytes with k_scale fp32 [num_rows],
 *            one scale per row, read on the device
 *   weights  fp32 [num_tokens][64], any sign (the caller folds the softmax
 *            scale, heads^-1/2 and a q scale into them)
 *   ks, ke   int32 [num_tokens], on the device: token n scores rows
 *            [ks[n], ke[n]) of the pool
 *   logits   fp32 [num_tokens][.], row stride logits_stride elements (64-bit
 *            arithmetic), max_len columns
 *
 *   logits[n][j - ks[n]] = k_scale[j] * sum_h weights[n][h] * max(0, sum_d q[n][h][d] * k[j][d])
 *                                                                     ks[n] <= j < ke[n]
 *
 * The products are exact and the sums fp32.  The dot products are the matrix
 * unit's (v_mfma_f32_16x16x32, fp32 accumulation).  The head sum has a fixed
 * order: for g = 0..3, chain_g = fma(w[h], max(0, s[h]), chain_g) from 0 over
 * the heads h = 16 hb + 4 g + i in ascending (hb, i), then
 * (chain_0 + chain_1) + (chain_2 + chain_3), then the multiplication by
 * k_scale[j] (the _k8 entries only).  Two calls give the same bits.
 *
 * ks and ke are read and clamped on the device: s = min(max(ks, 0), num_rows),
 * e = min(max(ke, s), num_rows), e = min(e, s + max_len); an inverted range is
 * empty and any contents are memory-safe.  Columns at or beyond e - s are not
 * written.  A pool row outside every token's range never changes a result
 * (NaN rows included).  No sync, no workspace; graph-capturable.  num_rows *
 * 256 bytes and num_tokens * logits_stride * 4 bytes may exceed 4 GiB.
 *
 * A prefill over token-major keys is ks = the sequence's first row, ke = the
 * token's position + 1; a decode over a contiguous [B][cap][128] key cache is
 * ks = b * cap, ke = b * cap + len.  A paged key pool (a block table) is not
 * built.
 *
 * 2. Selection: fa_mla_indexer_topk
 *
 *   logits   as above, read only in columns [0, e - s) after the same clamp
 *   indices  int32 [num_tokens][topk]
 *
 * Token n's list holds the flat rows s + c of its min(topk, e - s) largest
 * logits, compared by IEEE value (-0 equals +0); among values equal to the
 * last one kept the lowest columns win.  The list is in ascending row order
 * and padded with -1, the holes fa_mla_sparse_* skips.  It is determined by
 * the logits alone.  NaN logits are outside the contract but memory-safe:
 * every entry is a row of the token's range or -1.  topk is any value >= 0.
 * No sync, no workspace; graph-capturable.
 *
 * Statuses, in order, for both: a negative num_tokens, heads, num_rows,
 * max_len or topk, or logits_stride < max_len, then heads != 64:
 * FA_ERR_BAD_SHAPE; num_tokens == 0: FA_OK; a NULL pointer (k_scale of the
 * _k8 entries included): FA_ERR_NULL_POINTER; max_len == 0 or num_rows == 0:
 * FA_OK, every list is all -1 and no logit is written; topk == 0: FA_OK.
 */
#ifndef FA_MI355X_MLA_INDEXER_H
#define FA_MI355X_MLA_INDEXER_H

#include "fa_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int fa_mla_indexer_logits_f16(const void* q, const void* k, const float* weights, const int* ks, const int* ke,
                              float* logits, int num_tokens, int heads, int num_rows, int max_len,
                              long long logits_stride, void* hip_stream);
int fa_mla_indexer_logits_bf16(const void* q, const void* k, const float* weights, const int* ks, const int* ke,
                               float* logits, int num_tokens, int heads, int num_rows, int max_len,
                               long long logits_stride, void* hip_stream);
int fa_mla_indexer_logits_k8_f16(const void* q, const void* k, const float* weights, const int* ks, const int* ke,
                                 float* logits, int num_tokens, int heads, int num_rows, int max_len,
                                 long long logits_stride, void* hip_stream, const float* k_scale);
int fa_mla_indexer_logits_k8_bf16(const void* q, const void* k, const float* weights, const int* ks, const int* ke,
                                  float* logits, int num_tokens, int heads, int num_rows, int max_len,
                                  long long logits_stride, void* hip_stream, const float* k_scale);
int fa_mla_indexer_topk(const float* logits, const int* ks, const int* ke, int* indices, int num_tokens,
                        int num_rows, int max_len, long long logits_stride, int topk, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* FA_MI355X_MLA_INDEXER_H */
