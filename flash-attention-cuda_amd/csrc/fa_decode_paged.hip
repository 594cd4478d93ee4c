// fa_decode_paged.hip -- the decode-attention entries of include/fa_mi355x.h
// over a paged 16-bit K/V cache (fa_decode_paged_f16 / fa_decode_paged_bf16):
// the body of the contiguous entries (csrc/fa_decode_host.hpp) with
// kv_capacity = max_pages_per_seq * page_size, launching
// csrc/fa_decode_kernel.hpp with PAGED = true.
#include "fa_decode_host.hpp"

using namespace fa;

extern "C" int fa_decode_paged_f16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                   float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                                   int head_dim, int num_pages, int page_size, const int* block_table,
                                   int max_pages_per_seq, const int* kv_lens, int causal,
                                   int num_splits, void* workspace, unsigned long long ws_bytes,
                                   void* hip_stream) {
  return decode_entry<true, false>(FA_DTYPE_F16, q, k_pages, v_pages, o, lse, batch, heads_q, heads_kv,
                                   seqlen_q, 0, head_dim,
                                   {num_pages, page_size, block_table, max_pages_per_seq}, kv_lens,
                                   causal, 0, num_splits, workspace, ws_bytes, hip_stream, nullptr, nullptr);
}

extern "C" int fa_decode_paged_bf16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                    float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                                    int head_dim, int num_pages, int page_size, const int* block_table,
                                    int max_pages_per_seq, const int* kv_lens, int causal,
                                    int num_splits, void* workspace, unsigned long long ws_bytes,
                                    void* hip_stream) {
  return decode_entry<true, false>(FA_DTYPE_BF16, q, k_pages, v_pages, o, lse, batch, heads_q, heads_kv,
                                   seqlen_q, 0, head_dim,
                                   {num_pages, page_size, block_table, max_pages_per_seq}, kv_lens,
                                   causal, 0, num_splits, workspace, ws_bytes, hip_stream, nullptr, nullptr);
}
