// fa_prefill_varlen_win_paged_kv8.hip -- the sliding-window twins of
// fa_prefill_varlen_paged_kv8.hip's entries
// (fa_prefill_varlen_win_paged_kv8_f16 / _bf16 of include/fa_mi355x.h): the
// same argument list with `int window` after `causal`, the same entry body
// (csrc/fa_prefill_host.hpp) with WIN = true, launching the Windowed<>
// instantiations of csrc/fa_prefill_kernel.hpp.  A unit of
// its own so that the build stays parallel.
#include "fa_prefill_host.hpp"

using namespace fa;

#define FA_PREFILL_VARLEN(SUFFIX, DTYPE)                                                              \
  extern "C" int fa_prefill_varlen_win_paged_kv8_##SUFFIX(                                            \
      const void* q, const void* k_pages, const void* v_pages, void* o, float* lse, int batch,        \
      int heads_q, int heads_kv, int total_q, int head_dim, int num_pages, int page_size,             \
      const int* block_table, int max_pages_per_seq, const int* kv_lens,                              \
      const int* cu_seqlens_q, int causal, int window, void* hip_stream, const float* k_scale,        \
      const float* v_scale) {                                                                         \
    return prefill_entry<true, true, true, true>(DTYPE, q, k_pages, v_pages, o, lse, batch, heads_q,  \
        heads_kv, total_q, 0, head_dim, {num_pages, page_size, block_table, max_pages_per_seq},       \
        kv_lens, cu_seqlens_q, causal, window, hip_stream, k_scale, v_scale);                         \
  }
FA_PREFILL_VARLEN(f16, FA_DTYPE_F16)
FA_PREFILL_VARLEN(bf16, FA_DTYPE_BF16)
#undef FA_PREFILL_VARLEN
