// fa_cache_append_varlen.hip -- the packed (cu_seqlens, token-major) cache-append
// entries of include/fa_mi355x.h over the four cache forms: the host body of
// fa_cache_append.hip (csrc/fa_cache_append_host.hpp) with VARLEN = true,
// launching the packed twin of csrc/fa_cache_append_kernel.hpp (DESIGN.md
// §3.0l).
#include "fa_cache_append_host.hpp"

using namespace fa;

extern "C" int fa_cache_append_varlen_16(const void* k_new, const void* v_new, void* k_cache,
                                         void* v_cache, int batch, int heads_kv, int total_new,
                                         int kv_capacity, int head_dim, const int* kv_lens,
                                         const int* cu_seqlens, void* hip_stream) {
  return append_entry<false, false, true>(FA_DTYPE_F16, k_new, v_new, k_cache, v_cache, batch, heads_kv,
                                          total_new, kv_capacity, head_dim, {}, kv_lens, cu_seqlens,
                                          hip_stream, nullptr, nullptr);
}

extern "C" int fa_cache_append_varlen_paged_16(const void* k_new, const void* v_new, void* k_pages,
                                               void* v_pages, int batch, int heads_kv, int total_new,
                                               int head_dim, int num_pages, int page_size,
                                               const int* block_table, int max_pages_per_seq,
                                               const int* kv_lens, const int* cu_seqlens,
                                               void* hip_stream) {
  return append_entry<true, false, true>(FA_DTYPE_F16, k_new, v_new, k_pages, v_pages, batch, heads_kv,
                                         total_new, 0, head_dim,
                                         {num_pages, page_size, block_table, max_pages_per_seq}, kv_lens,
                                         cu_seqlens, hip_stream, nullptr, nullptr);
}

#define FA_APPEND_VARLEN_KV8(SUFFIX, DTYPE)                                                          \
  extern "C" int fa_cache_append_varlen_kv8_##SUFFIX(                                                \
      const void* k_new, const void* v_new, void* k_cache, void* v_cache, int batch, int heads_kv,   \
      int total_new, int kv_capacity, int head_dim, const int* kv_lens, const int* cu_seqlens,       \
      void* hip_stream, const float* k_scale, const float* v_scale) {                                \
    return append_entry<false, true, true>(DTYPE, k_new, v_new, k_cache, v_cache, batch, heads_kv,   \
                                           total_new, kv_capacity, head_dim, {}, kv_lens,            \
                                           cu_seqlens, hip_stream, k_scale, v_scale);                \
  }                                                                                                  \
  extern "C" int fa_cache_append_varlen_paged_kv8_##SUFFIX(                                          \
      const void* k_new, const void* v_new, void* k_pages, void* v_pages, int batch, int heads_kv,   \
      int total_new, int head_dim, int num_pages, int page_size, const int* block_table,             \
      int max_pages_per_seq, const int* kv_lens, const int* cu_seqlens, void* hip_stream,            \
      const float* k_scale, const float* v_scale) {                                                  \
    return append_entry<true, true, true>(DTYPE, k_new, v_new, k_pages, v_pages, batch, heads_kv,    \
                                          total_new, 0, head_dim,                                    \
                                          {num_pages, page_size, block_table, max_pages_per_seq},    \
                                          kv_lens, cu_seqlens, hip_stream, k_scale, v_scale);        \
  }
FA_APPEND_VARLEN_KV8(f16, FA_DTYPE_F16)
FA_APPEND_VARLEN_KV8(bf16, FA_DTYPE_BF16)
#undef FA_APPEND_VARLEN_KV8
