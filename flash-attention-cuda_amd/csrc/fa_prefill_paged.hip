// fa_prefill_paged.hip -- the prefill-attention entries of include/fa_mi355x.h
// over a paged 16-bit K/V cache (fa_prefill_paged_f16 / fa_prefill_paged_bf16):
// the entry body of csrc/fa_prefill_host.hpp launching
// csrc/fa_prefill_kernel.hpp with PAGED = true and KV = T.
#include "fa_prefill_host.hpp"

using namespace fa;

extern "C" int fa_prefill_paged_f16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                    float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                                    int head_dim, int num_pages, int page_size, const int* block_table,
                                    int max_pages_per_seq, const int* kv_lens, const int* q_lens,
                                    int causal, void* hip_stream) {
  return prefill_entry<true, false>(FA_DTYPE_F16, q, k_pages, v_pages, o, lse, batch, heads_q, heads_kv,
                                    seqlen_q, 0, head_dim,
                                    {num_pages, page_size, block_table, max_pages_per_seq}, kv_lens,
                                    q_lens, causal, 0, hip_stream, nullptr, nullptr);
}

extern "C" int fa_prefill_paged_bf16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                     float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                                     int head_dim, int num_pages, int page_size, const int* block_table,
                                     int max_pages_per_seq, const int* kv_lens, const int* q_lens,
                                     int causal, void* hip_stream) {
  return prefill_entry<true, false>(FA_DTYPE_BF16, q, k_pages, v_pages, o, lse, batch, heads_q, heads_kv,
                                    seqlen_q, 0, head_dim,
                                    {num_pages, page_size, block_table, max_pages_per_seq}, kv_lens,
                                    q_lens, causal, 0, hip_stream, nullptr, nullptr);
}
