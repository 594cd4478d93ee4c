// fa_decode_paged_kv8.hip -- the decode-attention entries of
// include/fa_mi355x.h over a paged FP8 (OCP E4M3) K/V cache
// (fa_decode_paged_kv8_f16 / fa_decode_paged_kv8_bf16): the body of the paged
// 16-bit entries (csrc/fa_decode_host.hpp) with one byte per pool element and
// one fp32 scale per K/V head for K and for V, launching
// csrc/fa_decode_kernel.hpp with PAGED = true and KV = unsigned char
// (DESIGN.md §3.0i).
#include "fa_decode_host.hpp"

using namespace fa;

extern "C" int fa_decode_paged_kv8_f16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                       float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                                       int head_dim, int num_pages, int page_size, const int* block_table,
                                       int max_pages_per_seq, const int* kv_lens, int causal,
                                       int num_splits, void* workspace, unsigned long long ws_bytes,
                                       void* hip_stream, const float* k_scale, const float* v_scale) {
  return decode_entry<true, true>(FA_DTYPE_F16, q, k_pages, v_pages, o, lse, batch, heads_q, heads_kv,
                                  seqlen_q, 0, head_dim,
                                  {num_pages, page_size, block_table, max_pages_per_seq}, kv_lens,
                                  causal, 0, num_splits, workspace, ws_bytes, hip_stream, k_scale, v_scale);
}

extern "C" int fa_decode_paged_kv8_bf16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                        float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                                        int head_dim, int num_pages, int page_size, const int* block_table,
                                        int max_pages_per_seq, const int* kv_lens, int causal,
                                        int num_splits, void* workspace, unsigned long long ws_bytes,
                                        void* hip_stream, const float* k_scale, const float* v_scale) {
  return decode_entry<true, true>(FA_DTYPE_BF16, q, k_pages, v_pages, o, lse, batch, heads_q, heads_kv,
                                  seqlen_q, 0, head_dim,
                                  {num_pages, page_size, block_table, max_pages_per_seq}, kv_lens,
                                  causal, 0, num_splits, workspace, ws_bytes, hip_stream, k_scale, v_scale);
}
