/*
 * fa_mi355x_mla_append.h -- the writers of the MLA caches: the latent append
 * with fused RoPE, into every latent cache form fa_mi355x_mla.h,
 * fa_mi355x_mla_kv8.h, fa_mi355x_mla_sparse.h and fa_mi355x_mla_sparse_kv8.h
 * read, and the quantising writer of the FP8 index-key pool that
 * fa_mla_indexer_logits_k8_* (fa_mi355x_mla_indexer.h) reads.  The conventions
 * and the status codes are those of fa_mi355x.h.  Everything is read on the
 * device: no sync, no workspace, graph-capturable.
 *
 * 1. Latent append: fa_mla_append[_paged][_kv8]_{f16,bf16}
 *
 * The suffix names the 16-bit type of the sources and of q.  All sources are
 * token-major; strides are in elements and addresses use 64-bit arithmetic
 * (pools pass 4 GiB).  Every stride is a multiple of 8 and every base pointer
 * 16-byte aligned: rows move in 16-byte pieces.
 *
 *   ckv_new  [T][512], token stride ckv_stride >= 512
 *   kpe_new  [T][64], token stride kpe_stride >= 64 (the [:, 512:576] slice of
 *            the kv_a projection output is read in place)
 *   q_pe     [T][heads_q][64], token and head strides >= 64 (the [..., 128:192]
 *            slice of a [T][Hq][192] q is read in place)
 *   q_out    rows (token, head) of 576 elements, token and head strides >= 576;
 *            only dims [512, 576) are written, so the caller's q_nope @ W_UK goes
 *            straight into dims [0, 512).  [N][Hq][576] (the sparse entries'
 *            layout) and [B][Hq][1][576] (the decode layout at Sq = 1) are
 *            expressible; the decode layout at Sq > 1 is not.  q_pe may alias
 *            its destination slice: a lane loads its bytes before it stores
 *            them.  heads_q = 0 with NULL q pointers appends only.
 *   cos, sin float32 [rope_len][32], 16-byte aligned; interleaved 0: NeoX pairs
 *            (i, i + 32), 1: GPT-J pairs (2i, 2i + 1).  The rotary dim is 64.
 *            Both NULL (heads_q = 0 only): the plain append, k_pe is a bit copy.
 *   cu_seqlens  device int32 [batch + 1], read and clamped on the device as
 *            fa_cache_append_varlen_* states: s_b = clamp(cu[b], 0, T), e_b =
 *            clamp(cu[b + 1], s_b, T), n_b = e_b - s_b, T = total_new.  NULL:
 *            the batch is uniform, n_b = seqlen_new, token (b, t) is row
 *            b * seqlen_new + t, and batch * seqlen_new must equal total_new.
 *   kv_lens  device int32 [batch], required: the lengths AFTER the append.
 *
 *   for t in [0, n_b):  pos = kv_lens[b] - n_b + t
 *     cache row pos of b   <- [ckv_new row | rope(kpe_new row, pos)]
 *     q_out[(b, t)][h][512:576] <- rope(q_pe[(b, t)][h], pos)      every head h
 *
 * The rotation is fa_rope_append_*'s: a' = a c - b s, b' = b c + a s with c =
 * cos[pos][i], s = sin[pos][i]; every product and sum is an fp32 operation of
 * its own (no fma contraction), the result is rounded once to the 16-bit type
 * and equals (a.float() * c - b.float() * s).to(dtype) on the CPU bit for bit.
 *
 * The cache is [batch][kv_capacity][576], or the pool [num_pages][page_size][576]
 * through block_table int32 [batch][max_pages_per_seq] (page_size % 64 == 0),
 * of the 16-bit type or (_kv8) of E4M3 bytes.  The FP8 byte is the reciprocal
 * contract of fa_cache_append_*_kv8 applied to the rounded 16-bit value y:
 * E4M3(clamp(float(y) * (1.0f / s), -448, 448)), s = ckv_scale[0], a device
 * float[1] read on the device (NULL: 1.0); +-inf saturates, a NaN stores a NaN
 * code.
 *
 * A cache row is written iff 0 <= pos < capacity (paged: max_pages_per_seq *
 * page_size, and the page id is in [0, num_pages)) and, when the tables are
 * given, pos < rope_len.  A q_out row is written iff t < n_b and 0 <= pos <
 * rope_len.  Nothing else is stored to, and no table row outside [0, rope_len)
 * is read.
 *
 * Statuses, in order, all before any launch:
 *   heads_q < 0 or rope_len < 0; batch < 0 or kv_capacity < 0; total_new < 0 or
 *   > INT_MAX - 64: FA_ERR_BAD_SHAPE
 *   paged: page_size not a positive multiple of 64, num_pages <= 0,
 *   max_pages_per_seq < 0, page_size * 1152 or max_pages_per_seq * page_size
 *   past their 32-bit bounds (the MLA readers' checks): FA_ERR_BAD_SHAPE
 *   batch == 0 or total_new == 0: FA_OK
 *   cu_seqlens NULL and batch * seqlen_new != total_new (or seqlen_new < 0);
 *   contiguous: kv_capacity * 1152 (kv8: * 576) > INT_MAX (the MLA readers'
 *   bound); total_new / 16 + batch > INT_MAX: FA_ERR_BAD_SHAPE
 *   capacity == 0 and heads_q == 0: FA_OK (capacity == 0 alone: the cache
 *   arguments are not looked at, q is still rotated)
 *   a stride below its row or no multiple of 8: FA_ERR_BAD_SHAPE
 *   ckv_new, kpe_new, ckv_cache, block_table or kv_lens NULL; one table NULL
 *   and not the other; heads_q > 0 with a NULL table, q_pe or q_out:
 *   FA_ERR_NULL_POINTER
 *   tables given with rope_len < 1; a table or a base pointer not 16-byte
 *   aligned: FA_ERR_BAD_SHAPE
 *
 * 2. Indexer key-pool writer: fa_mla_indexer_append_k8[_paged]_{f16,bf16}
 *
 *   k_new    [T][128] 16-bit, token stride k_stride >= 128, a multiple of 8
 *   k_pool   E4M3 bytes [num_rows][128];  k_scale  fp32 [num_rows]
 *
 * The sequences (cu_seqlens / kv_lens / uniform), pos and the rows are entry
 * 1's, so the indexer's flat rows are the latent pool's flat rows: contiguous
 * row b * kv_capacity + pos, paged row page * page_size + off; a row is written
 * iff it exists (0 <= pos < capacity, the page id inside the pool).  Per row
 * (DeepSeek-V3.2's act_quant):
 *
 *   a = max(max_d |float(x_d)|, 1e-4f);  s = a / 448.0f (an IEEE fp32 division)
 *   scale_pow2 != 0: s <- the smallest power of two >= s (exact, on the bits)
 *   byte = E4M3(clamp(float(x) * (1.0f / s), -448, 448));  k_scale[row] = s
 *
 * The index key's RoPE stays the caller's: V3.2 applies a Hadamard transform
 * between the RoPE and the quantisation, so there is nothing to fuse here.
 *
 * Statuses, in order: entry 1's sizes, page geometry, empties and sequence
 * checks (the block is 64 tokens); capacity == 0: FA_OK; k_stride < 128 or no
 * multiple of 8: FA_ERR_BAD_SHAPE; a NULL k_new, k_pool, k_scale, kv_lens or
 * block_table: FA_ERR_NULL_POINTER; k_new or k_pool not 16-byte aligned:
 * FA_ERR_BAD_SHAPE.
 */
#ifndef FA_MI355X_MLA_APPEND_H
#define FA_MI355X_MLA_APPEND_H

#include "fa_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int fa_mla_append_f16(const void* ckv_new, const void* kpe_new, void* ckv_cache, long long ckv_stride, long long
                      kpe_stride, int batch, int total_new, int seqlen_new, int kv_capacity, const int*
                      cu_seqlens, const int* kv_lens, const void* q_pe, void* q_out, int heads_q, long long
                      q_pe_token_stride, long long q_pe_head_stride, long long q_out_token_stride, long long
                      q_out_head_stride, const float* cos, const float* sin, int rope_len, int interleaved,
                      void* hip_stream);
int fa_mla_append_bf16(const void* ckv_new, const void* kpe_new, void* ckv_cache, long long ckv_stride, long
                       long kpe_stride, int batch, int total_new, int seqlen_new, int kv_capacity, const int*
                       cu_seqlens, const int* kv_lens, const void* q_pe, void* q_out, int heads_q, long long
                       q_pe_token_stride, long long q_pe_head_stride, long long q_out_token_stride, long long
                       q_out_head_stride, const float* cos, const float* sin, int rope_len, int interleaved,
                       void* hip_stream);
int fa_mla_append_kv8_f16(const void* ckv_new, const void* kpe_new, void* ckv_cache, long long ckv_stride, long
                          long kpe_stride, int batch, int total_new, int seqlen_new, int kv_capacity, const int*
                          cu_seqlens, const int* kv_lens, const void* q_pe, void* q_out, int heads_q, long long
                          q_pe_token_stride, long long q_pe_head_stride, long long q_out_token_stride, long long
                          q_out_head_stride, const float* cos, const float* sin, int rope_len, int interleaved,
                          void* hip_stream, const float* ckv_scale);
int fa_mla_append_kv8_bf16(const void* ckv_new, const void* kpe_new, void* ckv_cache, long long ckv_stride, long
                           long kpe_stride, int batch, int total_new, int seqlen_new, int kv_capacity, const
                           int* cu_seqlens, const int* kv_lens, const void* q_pe, void* q_out, int heads_q, long
                           long q_pe_token_stride, long long q_pe_head_stride, long long q_out_token_stride,
                           long long q_out_head_stride, const float* cos, const float* sin, int rope_len, int
                           interleaved, void* hip_stream, const float* ckv_scale);
int fa_mla_append_paged_f16(const void* ckv_new, const void* kpe_new, void* ckv_cache, long long ckv_stride,
                            long long kpe_stride, int batch, int total_new, int seqlen_new, int num_pages, int
                            page_size, const int* block_table, int max_pages_per_seq, const int* cu_seqlens,
                            const int* kv_lens, const void* q_pe, void* q_out, int heads_q, long long
                            q_pe_token_stride, long long q_pe_head_stride, long long q_out_token_stride, long
                            long q_out_head_stride, const float* cos, const float* sin, int rope_len, int
                            interleaved, void* hip_stream);
int fa_mla_append_paged_bf16(const void* ckv_new, const void* kpe_new, void* ckv_cache, long long ckv_stride,
                             long long kpe_stride, int batch, int total_new, int seqlen_new, int num_pages, int
                             page_size, const int* block_table, int max_pages_per_seq, const int* cu_seqlens,
                             const int* kv_lens, const void* q_pe, void* q_out, int heads_q, long long
                             q_pe_token_stride, long long q_pe_head_stride, long long q_out_token_stride, long
                             long q_out_head_stride, const float* cos, const float* sin, int rope_len, int
                             interleaved, void* hip_stream);
int fa_mla_append_paged_kv8_f16(const void* ckv_new, const void* kpe_new, void* ckv_cache, long long ckv_stride,
                                long long kpe_stride, int batch, int total_new, int seqlen_new, int num_pages,
                                int page_size, const int* block_table, int max_pages_per_seq, const int*
                                cu_seqlens, const int* kv_lens, const void* q_pe, void* q_out, int heads_q, long
                                long q_pe_token_stride, long long q_pe_head_stride, long long
                                q_out_token_stride, long long q_out_head_stride, const float* cos, const float*
                                sin, int rope_len, int interleaved, void* hip_stream, const float* ckv_scale);
int fa_mla_append_paged_kv8_bf16(const void* ckv_new, const void* kpe_new, void* ckv_cache, long long
                                 ckv_stride, long long kpe_stride, int batch, int total_new, int seqlen_new, int
                                 num_pages, int page_size, const int* block_table, int max_pages_per_seq, const
                                 int* cu_seqlens, const int* kv_lens, const void* q_pe, void* q_out, int
                                 heads_q, long long q_pe_token_stride, long long q_pe_head_stride, long long
                                 q_out_token_stride, long long q_out_head_stride, const float* cos, const float*
                                 sin, int rope_len, int interleaved, void* hip_stream, const float* ckv_scale);

int fa_mla_indexer_append_k8_f16(const void* k_new, void* k_pool, float* k_scale, long long k_stride, int batch,
                                 int total_new, int seqlen_new, int kv_capacity, const int* cu_seqlens, const
                                 int* kv_lens, int scale_pow2, void* hip_stream);
int fa_mla_indexer_append_k8_bf16(const void* k_new, void* k_pool, float* k_scale, long long k_stride, int
                                  batch, int total_new, int seqlen_new, int kv_capacity, const int* cu_seqlens,
                                  const int* kv_lens, int scale_pow2, void* hip_stream);
int fa_mla_indexer_append_k8_paged_f16(const void* k_new, void* k_pool, float* k_scale, long long k_stride, int
                                       batch, int total_new, int seqlen_new, int num_pages, int page_size, const
                                       int* block_table, int max_pages_per_seq, const int* cu_seqlens, const
                                       int* kv_lens, int scale_pow2, void* hip_stream);
int fa_mla_indexer_append_k8_paged_bf16(const void* k_new, void* k_pool, float* k_scale, long long k_stride, int
                                        batch, int total_new, int seqlen_new, int num_pages, int page_size,
                                        const int* block_table, int max_pages_per_seq, const int* cu_seqlens,
                                        const int* kv_lens, int scale_pow2, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* FA_MI355X_MLA_APPEND_H */
