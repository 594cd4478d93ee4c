/*
 * fa_mi355x_mla_kv8.h -- MLA decode over an FP8 latent cache: the entries of
 * fa_mi355x_mla.h with the cache stored as OCP FP8 E4M3 bytes and one fp32
 * scale.  The contract is that header's with one change,
 *
 *   c[j, d] = ckv_scale * float(E4M3 byte ckv8[b][j][d])        d < 576
 *   s, visible, O, LSE: exactly as fa_mi355x_mla.h states them over this c
 *
 *   ckv8       [batch][kv_capacity][576] bytes                    (contiguous)
 *   ckv8_pages [num_pages][page_size][576] bytes, page_size % 64 == 0, with
 *              the same block_table                               (paged)
 *   ckv_scale  DEVICE float[1], or NULL for 1.0: fa_mi355x.h's k_scale[heads_kv]
 *              with the one latent head.  It is read on the device (a captured
 *              graph follows a rewritten scale) and never multiplied into a
 *              byte: it enters the score scale, and through it the LSE, and
 *              the final normalisation.
 *
 * q and o stay f16 / bf16, Q is not quantised and the products are the 16-bit
 * ones (E4M3 -> f16 / bf16 is exact).  A writer stores E4M3(clamp(x /
 * ckv_scale, -448, 448)), round to nearest even; no entry here writes the
 * cache.  Each function takes the argument list of its fa_mi355x_mla.h
 * namesake followed by ckv_scale, after hip_stream, where the fa_decode_*_kv8
 * entries put their scales.  Everything else is unchanged: seqlen_q 1..16, any
 * heads_q, kv_lens, the table and the page ids read and clamped on the device,
 * rows at or past a length never read, no sync, graph-capturable, the statuses
 * and their order, num_splits 0..64 with the plan and the workspace of
 * fa_mla_decode_num_splits and fa_mla_decode_ws_bytes (neither depends on the
 * cache type), and paged = contiguous on the gathered cache bit for bit.  The
 * contiguous capacity bound is kv_capacity * 576 <= INT_MAX.
 */
#ifndef FA_MI355X_MLA_KV8_H
#define FA_MI355X_MLA_KV8_H

#include "fa_mi355x_mla.h"

#ifdef __cplusplus
extern "C" {
#endif

int fa_mla_decode_kv8_f16(const void* q, const void* ckv8, void* o, float* lse, int batch, int heads_q,
                          int seqlen_q, int kv_capacity, const int* kv_lens, int causal,
                          float softmax_scale, int num_splits, void* workspace,
                          unsigned long long ws_bytes, void* hip_stream, const float* ckv_scale);
int fa_mla_decode_kv8_bf16(const void* q, const void* ckv8, void* o, float* lse, int batch, int heads_q,
                           int seqlen_q, int kv_capacity, const int* kv_lens, int causal,
                           float softmax_scale, int num_splits, void* workspace,
                           unsigned long long ws_bytes, void* hip_stream, const float* ckv_scale);
int fa_mla_decode_paged_kv8_f16(const void* q, const void* ckv8_pages, void* o, float* lse, int batch,
                                int heads_q, int seqlen_q, int num_pages, int page_size,
                                const int* block_table, int max_pages_per_seq, const int* kv_lens,
                                int causal, float softmax_scale, int num_splits, void* workspace,
                                unsigned long long ws_bytes, void* hip_stream, const float* ckv_scale);
int fa_mla_decode_paged_kv8_bf16(const void* q, const void* ckv8_pages, void* o, float* lse, int batch,
                                 int heads_q, int seqlen_q, int num_pages, int page_size,
                                 const int* block_table, int max_pages_per_seq, const int* kv_lens,
                                 int causal, float softmax_scale, int num_splits, void* workspace,
                                 unsigned long long ws_bytes, void* hip_stream, const float* ckv_scale);

#ifdef __cplusplus
}
#endif

#endif /* FA_MI355X_MLA_KV8_H */
