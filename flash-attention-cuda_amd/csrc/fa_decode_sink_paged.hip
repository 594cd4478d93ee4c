// fa_decode_sink_paged.hip -- the attention-sink twins of
// fa_decode_win_paged.hip's entries (fa_decode_sink_paged_f16 / _bf16 of
// include/fa_mi355x.h): the same argument list with `const float* sinks` after
// `window`, the same entry body (csrc/fa_decode_host.hpp) with WIN = SINK =
// true, launching the Sinked<Windowed<>> instantiations of
// csrc/fa_decode_kernel.hpp.  A unit of its own so that the
// build stays parallel.
#include "fa_decode_host.hpp"

using namespace fa;

extern "C" int fa_decode_sink_paged_f16(const void* q, const void* k_pages, const void* v_pages,
    void* o, float* lse, int batch, int heads_q, int heads_kv, int seqlen_q, int head_dim,
    int num_pages, int page_size, const int* block_table, int max_pages_per_seq, const int* kv_lens,
    int causal, int window, const float* sinks, int num_splits, void* workspace,
    unsigned long long ws_bytes, void* hip_stream) {
  return decode_entry<true, false, true, true>(FA_DTYPE_F16, q, k_pages, v_pages, o, lse, batch,
      heads_q, heads_kv, seqlen_q, 0, head_dim,
      {num_pages, page_size, block_table, max_pages_per_seq}, kv_lens, causal, window, num_splits,
      workspace, ws_bytes, hip_stream, nullptr, nullptr, sinks);
}

extern "C" int fa_decode_sink_paged_bf16(const void* q, const void* k_pages, const void* v_pages,
    void* o, float* lse, int batch, int heads_q, int heads_kv, int seqlen_q, int head_dim,
    int num_pages, int page_size, const int* block_table, int max_pages_per_seq, const int* kv_lens,
    int causal, int window, const float* sinks, int num_splits, void* workspace,
    unsigned long long ws_bytes, void* hip_stream) {
  return decode_entry<true, false, true, true>(FA_DTYPE_BF16, q, k_pages, v_pages, o, lse, batch,
      heads_q, heads_kv, seqlen_q, 0, head_dim,
      {num_pages, page_size, block_table, max_pages_per_seq}, kv_lens, causal, window, num_splits,
      workspace, ws_bytes, hip_stream, nullptr, nullptr, sinks);
}
