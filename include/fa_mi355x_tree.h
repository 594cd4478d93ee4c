/*
 * fa_mi355x_tree.h -- tree-masked decode attention for speculative decoding
 * (EAGLE / Medusa style tree verification) over the four K/V cache forms of
 * fa_mi355x.h: the eight `fa_decode_sink_*` entries with
 * `const int* tree_mask` inserted directly after `sinks` (`_tree` in `_sink`'s
 * place).  The conventions, the status codes and every argument but
 * `tree_mask` are those of fa_mi355x.h.
 *
 * The seqlen_q (1..16) query tokens of a call are draft tokens that form a
 * tree behind the cached prefix; their K/V rows are the LAST seqlen_q rows of
 * the cache (appended with the fa_cache_append_* or fa_rope_append_* entries
 * before the call, kv_lens counted after the append).  Each draft token sees
 * the prefix and, among the drafts, only the tokens its mask word names: its
 * ancestors and itself.
 *
 * tree_mask: a device array int32 [batch][seqlen_q], read on the device (no
 * sync; a captured graph follows a mask rewritten between replays), shared by
 * all heads of a batch element, or NULL for the chain.  With
 *   len = clamp(kv_lens[b], 0, capacity),  base = len - seqlen_q,
 *   m_t = tree_mask[b][t] & ((1 << seqlen_q) - 1)      (higher bits ignored):
 *  - draft key i (0 <= i < seqlen_q), cache row base + i: seen by row t iff bit
 *    i of m_t is set and base + i >= 0;
 *  - prefix key j < base: seen by every row, subject to the window;
 *  - window = W >= 1: depth_t = max(popcount(m_t) - 1, 0), pos_t = base +
 *    depth_t, and a prefix key j is seen iff j > pos_t - W.  W = 0: no window.
 *    0 < W < seqlen_q is FA_ERR_BAD_SHAPE: with W >= seqlen_q every ancestor
 *    lies inside the window, so draft keys take no window test;
 *  - the first key any row can see is max(0, len - seqlen_q + 1 - W) as for
 *    the `_win` entries: cache rows below it are never read, and in the paged
 *    form neither are the block-table entries of pages lying wholly below it;
 *  - sinks: exactly the `_sink` entries' rule (den = exp(sinks[h]) + sum_j
 *    exp(s_j), LSE = log(den), the sink counted once, split or not);
 *  - a row that sees no key gives O = 0 and LSE = -inf (with sinks: sinks[h]);
 *  - causal must be non-zero (FA_ERR_BAD_SHAPE otherwise): the mask replaces
 *    the causal rule.
 * tree_mask == NULL, or the chain m_t = (2 << t) - 1, gives the `_sink` twin's
 * O and LSE bit for bit at the same window, sinks and num_splits (W = 0 and no
 * sinks: the plain entry's).  Any mask contents are memory-safe: the words only
 * deselect keys inside [0, len), they need not describe a tree.  The two new
 * refusals arrive where the twin refuses a window without causal; every other
 * status and its order, fa_decode_num_splits() / fa_decode_ws_bytes() at the
 * window's capacity, and the workspace are the `_sink` twin's; paged equals
 * contiguous on the gathered cache and an FP8 cache with unit scales equals
 * the 16-bit one, bit for bit.
 */
#ifndef FA_MI355X_TREE_H
#define FA_MI355X_TREE_H

#include "fa_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int fa_decode_tree_f16(const void* q, const void* k, const void* v, void* o, float* lse, int batch,
                       int heads_q, int heads_kv, int seqlen_q, int kv_capacity, int head_dim,
                       const int* kv_lens, int causal, int window, const float* sinks,
                       const int* tree_mask, int num_splits, void* workspace,
                       unsigned long long ws_bytes, void* hip_stream);
int fa_decode_tree_bf16(const void* q, const void* k, const void* v, void* o, float* lse, int batch,
                        int heads_q, int heads_kv, int seqlen_q, int kv_capacity, int head_dim,
                        const int* kv_lens, int causal, int window, const float* sinks,
                        const int* tree_mask, int num_splits, void* workspace,
                        unsigned long long ws_bytes, void* hip_stream);
int fa_decode_tree_kv8_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                           int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                           int head_dim, const int* kv_lens, int causal, int window,
                           const float* sinks, const int* tree_mask, int num_splits,
                           void* workspace, unsigned long long ws_bytes, void* hip_stream,
                           const float* k_scale, const float* v_scale);
int fa_decode_tree_kv8_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                            int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                            int head_dim, const int* kv_lens, int causal, int window,
                            const float* sinks, const int* tree_mask, int num_splits,
                            void* workspace, unsigned long long ws_bytes, void* hip_stream,
                            const float* k_scale, const float* v_scale);
int fa_decode_tree_paged_f16(const void* q, const void* k_pages, const void* v_pages, void* o,
                             float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                             int head_dim, int num_pages, int page_size, const int* block_table,
                             int max_pages_per_seq, const int* kv_lens, int causal, int window,
                             const float* sinks, const int* tree_mask, int num_splits,
                             void* workspace, unsigned long long ws_bytes, void* hip_stream);
int fa_decode_tree_paged_bf16(const void* q, const void* k_pages, const void* v_pages, void* o,
                              float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                              int head_dim, int num_pages, int page_size, const int* block_table,
                              int max_pages_per_seq, const int* kv_lens, int causal, int window,
                              const float* sinks, const int* tree_mask, int num_splits,
                              void* workspace, unsigned long long ws_bytes, void* hip_stream);
int fa_decode_tree_paged_kv8_f16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                 float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                                 int head_dim, int num_pages, int page_size, const int* block_table,
                                 int max_pages_per_seq, const int* kv_lens, int causal, int window,
                                 const float* sinks, const int* tree_mask, int num_splits,
                                 void* workspace, unsigned long long ws_bytes, void* hip_stream,
                                 const float* k_scale, const float* v_scale);
int fa_decode_tree_paged_kv8_bf16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                  float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                                  int head_dim, int num_pages, int page_size,
                                  const int* block_table, int max_pages_per_seq, const int* kv_lens,
                                  int causal, int window, const float* sinks, const int* tree_mask,
                                  int num_splits, void* workspace, unsigned long long ws_bytes,
                                  void* hip_stream, const float* k_scale, const float* v_scale);

#ifdef __cplusplus
}
#endif

#endif /* FA_MI355X_TREE_H */
