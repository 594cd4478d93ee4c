/*
 * fa_mi355x_mla_sparse.h -- MLA sparse attention: the weight-absorbed 576/512
 * attention of fa_mi355x_mla.h where every query token attends only to the
 * latent rows an index list names (DeepSeek-V3.2's sparse attention, DSA),
 * for decode and for prefill alike.  The conventions and the status codes are
 * those of fa_mi355x.h.
 *
 *   q        [num_tokens][heads_q][576]  16-bit, contiguous (a [B][Sq][Hq][576]
 *            tensor taken as it is, num_tokens = B * Sq)
 *   ckv      [num_rows][576]  the same 16-bit type: a flat pool of latent rows
 *            [c_kv (512) | k_pe (64)].  A contiguous cache [B][cap][576] is such
 *            a pool with row b * cap + j, a page pool [num_pages][page_size][576]
 *            with row page * page_size + off: no block table, no page-size rule
 *   indices  int32 [num_tokens][topk], on the device, read on the device
 *   o        [num_tokens][heads_q][512]  the same 16-bit type
 *   lse      fp32 [num_tokens][heads_q], or NULL
 *
 * Token n attends to exactly the rows indices[n][0..topk), the same set for
 * all its heads.  Entry i is valid iff 0 <= i < num_rows; every other value
 * (-1, num_rows, INT_MAX, INT_MIN, ...) is a hole: it contributes nothing and
 * no byte of the pool is read on its behalf, so any contents are memory-safe.
 * A row listed twice counts twice.  There is no causal flag and no kv_lens:
 * what a token sees is its list's business.  Over the valid entries,
 *
 *   s[n,h,i]  = softmax_scale * sum_{d<576} q[n,h,d] * ckv[idx_i, d]   (scaled in fp32)
 *   O[n,h,:]  = sum_i softmax_i(s[n,h,.]) * ckv[idx_i, 0:512]
 *   LSE[n,h]  = log sum_i exp(s[n,h,i])                                 (natural log)
 *   a token with no valid entry (topk = 0 among them): O = 0, LSE = -inf
 *
 * topk is any value >= 0 (not only multiples of 64), heads_q any value >= 1,
 * num_tokens * heads_q <= INT_MAX, and num_rows * 1152 bytes may exceed 4 GiB.
 * softmax_scale must be finite and > 0.  No sync, no scratch beyond the
 * workspace; graph-capturable; two calls give the same bits.
 *
 * num_splits: 0 = the plan's choice, 1 up to 64 forces it: the list's 64-entry
 * tiles are split across workgroups and merged in the same launch through
 * `workspace`.  Geometry, plan and workspace are the MLA decode entries' with
 * batch = num_tokens and seqlen_q = 1: the plan is
 * fa_mla_decode_num_splits(num_tokens, heads_q, 1, topk), the size
 * fa_mla_decode_ws_bytes(num_tokens, heads_q, 1, num_splits) (16-byte aligned,
 * counters zero before the first launch and left zero by each), so the
 * per-stream workspace of fa_mi355x_mla.h serves these entries too.
 *
 * Statuses, in order: a negative num_tokens, heads_q, topk, num_rows or
 * num_splits, then a softmax_scale that is not finite and > 0:
 * FA_ERR_BAD_SHAPE; num_tokens == 0 or heads_q == 0: FA_OK; num_tokens *
 * heads_q > INT_MAX: FA_ERR_BAD_SHAPE; topk == 0 or num_rows == 0 (every entry
 * a hole): `o` is filled (NULL: FA_ERR_NULL_POINTER) and q, ckv and indices may
 * be NULL; a NULL q, ckv, indices or o: FA_ERR_NULL_POINTER; num_splits > 64:
 * FA_ERR_BAD_CONFIG; a split without a workspace that is present, long enough
 * and 16-byte aligned: FA_ERR_WORKSPACE.
 */
#ifndef FA_MI355X_MLA_SPARSE_H
#define FA_MI355X_MLA_SPARSE_H

#include "fa_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int fa_mla_sparse_f16(const void* q, const void* ckv, const int* indices, void* o, float* lse,
                      int num_tokens, int heads_q, int topk, int num_rows, float softmax_scale,
                      int num_splits, void* workspace, unsigned long long ws_bytes, void* hip_stream);
int fa_mla_sparse_bf16(const void* q, const void* ckv, const int* indices, void* o, float* lse,
                       int num_tokens, int heads_q, int topk, int num_rows, float softmax_scale,
                       int num_splits, void* workspace, unsigned long long ws_bytes, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* FA_MI355X_MLA_SPARSE_H */
