/*
 * fa_mi355x_mla_sparse_kv8.h -- MLA sparse attention over an FP8 (E4M3) latent
 * pool: fa_mi355x_mla_sparse.h's attention (every query token attends only to
 * the latent rows its index list names, DeepSeek-V3.2's DSA) over the bytes of
 * fa_mi355x_mla_kv8.h's cache.  The conventions and the status codes are those
 * of fa_mi355x.h.
 *
 *   q          [num_tokens][heads_q][576]  fp16 or bf16, contiguous
 *   ckv8       [num_rows][576]  OCP E4M3 bytes, 16-byte aligned: a flat pool of
 *              latent rows [c_kv (512) | k_pe (64)], read as
 *                c[r, d] = ckv_scale * float(E4M3 byte ckv8[r][d])
 *              (a contiguous cache [B][cap][576] is such a pool with row b * cap
 *              + j, a page pool with row page * page_size + off)
 *   indices    int32 [num_tokens][topk], on the device, read on the device
 *   ckv_scale  device float[1], read by the kernel (a captured graph follows a
 *              rewritten scale); NULL: 1.0
 *   o          [num_tokens][heads_q][512]  q's type
 *   lse        fp32 [num_tokens][heads_q], or NULL
 *
 * Entry i is valid iff 0 <= i < num_rows; every other value is a hole: it
 * contributes nothing and no byte of the pool is read on its behalf.  A row
 * listed twice counts twice.  Over the valid entries,
 *
 *   s[n,h,i]  = softmax_scale * sum_{d<576} q[n,h,d] * c[idx_i, d]     (scaled in fp32)
 *   O[n,h,:]  = sum_i softmax_i(s[n,h,.]) * c[idx_i, 0:512]
 *   LSE[n,h]  = log sum_i exp(s[n,h,i])                                 (natural log)
 *   a token with no valid entry (topk = 0 among them): O = 0, LSE = -inf
 *
 * The scale never multiplies a byte: it is folded into the score scale (and so
 * into LSE) and into the final normalisation.  E4M3 -> fp16 / bf16 is exact; q,
 * the probabilities and the matrix products stay 16-bit.  A writer stores
 * E4M3(clamp(x / ckv_scale, -448, 448)), round to nearest even.  One scale per
 * pool, all 576 dims as bytes: this is NOT FlashMLA's 656-byte FP8 row (scales
 * per 128 dims, a 16-bit k_pe).
 *
 * topk is any value >= 0, heads_q any value >= 1, num_tokens * heads_q <=
 * INT_MAX, and num_rows * 576 bytes may exceed 4 GiB.  softmax_scale must be
 * finite and > 0.  No sync, no scratch beyond the workspace; graph-capturable;
 * two calls give the same bits.
 *
 * num_splits, the plan and the workspace are fa_mi355x_mla_sparse.h's: the MLA
 * decode entries' with batch = num_tokens and seqlen_q = 1
 * (fa_mla_decode_num_splits(num_tokens, heads_q, 1, topk),
 * fa_mla_decode_ws_bytes(num_tokens, heads_q, 1, num_splits)).
 *
 * Statuses, in fa_mi355x_mla_sparse.h's order: a negative num_tokens, heads_q,
 * topk, num_rows or num_splits, then a softmax_scale that is not finite and
 * > 0: FA_ERR_BAD_SHAPE; num_tokens == 0 or heads_q == 0: FA_OK; num_tokens *
 * heads_q > INT_MAX: FA_ERR_BAD_SHAPE; topk == 0 or num_rows == 0: `o` is
 * filled (NULL: FA_ERR_NULL_POINTER) and q, ckv8 and indices may be NULL; a
 * NULL q, ckv8, indices or o: FA_ERR_NULL_POINTER; num_splits > 64:
 * FA_ERR_BAD_CONFIG; a split without a workspace that is present, long enough
 * and 16-byte aligned: FA_ERR_WORKSPACE.  ckv_scale is never a status.
 */
#ifndef FA_MI355X_MLA_SPARSE_KV8_H
#define FA_MI355X_MLA_SPARSE_KV8_H

#include "fa_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int fa_mla_sparse_kv8_f16(const void* q, const void* ckv8, const int* indices, const float* ckv_scale, void* o,
                          float* lse, int num_tokens, int heads_q, int topk, int num_rows, float softmax_scale,
                          int num_splits, void* workspace, unsigned long long ws_bytes, void* hip_stream);
int fa_mla_sparse_kv8_bf16(const void* q, const void* ckv8, const int* indices, const float* ckv_scale, void* o,
                           float* lse, int num_tokens, int heads_q, int topk, int num_rows, float softmax_scale,
                           int num_splits, void* workspace, unsigned long long ws_bytes, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* FA_MI355X_MLA_SPARSE_KV8_H */
