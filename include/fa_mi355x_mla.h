/*
 * fa_mi355x_mla.h -- decode attention over a latent K/V cache: Multi-head
 * Latent Attention (DeepSeek-V2 / V3 / R1, Kimi K2) in its weight-absorbed
 * decode form.  The conventions and the status codes are those of
 * fa_mi355x.h; what differs from its fa_decode_* entries is the cache.
 *
 * Every query head attends to ONE shared latent row per token,
 * [c_kv (512) | k_pe (64)]: the score contracts over all 576 dims, the value
 * is the first 512 dims of the same row, and the softmax scale is the
 * caller's (the model's 1/sqrt(192) times its YaRN factor, not 1/sqrt(576)).
 * With c = ckv[b] and len_b = clamp(kv_lens[b], 0, capacity):
 *
 *   s[t, j]    = softmax_scale * sum_{d<576} q[b,h,t,d] * c[j,d]
 *   visible    : j < len_b                      (causal = 0)
 *                j <= len_b - seqlen_q + t      (causal != 0, bottom-right)
 *   O[b,h,t,:] = sum_j softmax_j(s[t,.]) * c[j, 0:512]
 *   LSE[b,h,t] = log sum_j exp(s[t,j])          (natural log)
 *   a row that sees no key: O = 0, LSE = -inf
 *
 *   q    [batch][heads_q][seqlen_q][576]  16-bit (W_UK absorbed into q_nope, q_pe appended)
 *   o    [batch][heads_q][seqlen_q][512]  the same 16-bit type
 *   lse  [batch][heads_q][seqlen_q] fp32, or NULL
 *   ckv  [batch][kv_capacity][576]                         (contiguous)
 *   ckv_pages [num_pages][page_size][576], page_size % 64 == 0, with
 *        block_table int32 [batch][max_pages_per_seq]      (paged: the paged
 *        decode entries' conventions with one K/V head)
 *
 * seqlen_q is 1..16, heads_q any value >= 1.  kv_lens (NULL: the capacity),
 * the block table and the page ids are read and clamped on the device: rows
 * at or past a length and table entries of pages holding no key below it are
 * never read, a page id outside the pool reads as zero rows, any contents are
 * memory-safe.  No sync; graph-capturable.  softmax_scale must be finite and
 * > 0 (FA_ERR_BAD_SHAPE otherwise, where the fa_decode_win_* entries check
 * their window); every other status and its order are the fa_decode_* entries'.
 *
 * num_splits: 0 = the plan's choice (fa_mla_decode_num_splits), 1 up to 64
 * forces it.  The key range is split across workgroups and merged in the same
 * launch through `workspace` (fa_mla_decode_ws_bytes; 16-byte aligned): the
 * fa_decode_* entries' layout with head_dim 512 -- arrival counters in the
 * first 64 KB, which must be zero before the first launch and are left zero by
 * each -- so one per-stream workspace of the larger size serves both families.
 * The paged entries give the contiguous entries' O and LSE on the gathered
 * cache bit for bit at the same num_splits.
 */
#ifndef FA_MI355X_MLA_H
#define FA_MI355X_MLA_H

#include "fa_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int fa_mla_decode_f16(const void* q, const void* ckv, void* o, float* lse, int batch, int heads_q,
                      int seqlen_q, int kv_capacity, const int* kv_lens, int causal,
                      float softmax_scale, int num_splits, void* workspace,
                      unsigned long long ws_bytes, void* hip_stream);
int fa_mla_decode_bf16(const void* q, const void* ckv, void* o, float* lse, int batch, int heads_q,
                       int seqlen_q, int kv_capacity, const int* kv_lens, int causal,
                       float softmax_scale, int num_splits, void* workspace,
                       unsigned long long ws_bytes, void* hip_stream);
int fa_mla_decode_paged_f16(const void* q, const void* ckv_pages, void* o, float* lse, int batch,
                            int heads_q, int seqlen_q, int num_pages, int page_size,
                            const int* block_table, int max_pages_per_seq, const int* kv_lens,
                            int causal, float softmax_scale, int num_splits, void* workspace,
                            unsigned long long ws_bytes, void* hip_stream);
int fa_mla_decode_paged_bf16(const void* q, const void* ckv_pages, void* o, float* lse, int batch,
                             int heads_q, int seqlen_q, int num_pages, int page_size,
                             const int* block_table, int max_pages_per_seq, const int* kv_lens,
                             int causal, float softmax_scale, int num_splits, void* workspace,
                             unsigned long long ws_bytes, void* hip_stream);
int fa_mla_decode_num_splits(int batch, int heads_q, int seqlen_q, int kv_capacity);
unsigned long long fa_mla_decode_ws_bytes(int batch, int heads_q, int seqlen_q, int num_splits);

#ifdef __cplusplus
}
#endif

#endif /* FA_MI355X_MLA_H */
