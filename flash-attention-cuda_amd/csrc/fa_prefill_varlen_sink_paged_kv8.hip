// fa_prefill_varlen_sink_paged_kv8.hip -- the attention-sink twins of
// fa_prefill_varlen_win_paged_kv8.hip's entries
// (fa_prefill_varlen_sink_paged_kv8_f16 / _bf16 of include/fa_mi355x.h): the
// same argument list with `const float* sinks` after `window`, the same entry
// body (csrc/fa_prefill_host.hpp) with WIN = SINK = true, launching the
// Sinked<Windowed<>> instantiations of csrc/fa_prefill_kernel.hpp (DESIGN.md
// §3.0n).  A unit of its own so that the build stays parallel.
#include "fa_prefill_host.hpp"

using namespace fa;

extern "C" int fa_prefill_varlen_sink_paged_kv8_f16(const void* q, const void* k_pages,
    const void* v_pages, void* o, float* lse, int batch, int heads_q, int heads_kv, int total_q,
    int head_dim, int num_pages, int page_size, const int* block_table, int max_pages_per_seq,
    const int* kv_lens, const int* cu_seqlens_q, int causal, int window, const float* sinks,
    void* hip_stream, const float* k_scale, const float* v_scale) {
  return prefill_entry<true, true, true, true, true>(FA_DTYPE_F16, q, k_pages, v_pages, o, lse,
      batch, heads_q, heads_kv, total_q, 0, head_dim,
      {num_pages, page_size, block_table, max_pages_per_seq}, kv_lens, cu_seqlens_q, causal, window,
      hip_stream, k_scale, v_scale, sinks);
}

extern "C" int fa_prefill_varlen_sink_paged_kv8_bf16(const void* q, const void* k_pages,
    const void* v_pages, void* o, float* lse, int batch, int heads_q, int heads_kv, int total_q,
    int head_dim, int num_pages, int page_size, const int* block_table, int max_pages_per_seq,
    const int* kv_lens, const int* cu_seqlens_q, int causal, int window, const float* sinks,
    void* hip_stream, const float* k_scale, const float* v_scale) {
  return prefill_entry<true, true, true, true, true>(FA_DTYPE_BF16, q, k_pages, v_pages, o, lse,
      batch, heads_q, heads_kv, total_q, 0, head_dim,
      {num_pages, page_size, block_table, max_pages_per_seq}, kv_lens, cu_seqlens_q, causal, window,
      hip_stream, k_scale, v_scale, sinks);
}
