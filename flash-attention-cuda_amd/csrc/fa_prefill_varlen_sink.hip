// fa_prefill_varlen_sink.hip -- the attention-sink twins of
// fa_prefill_varlen_win.hip's entries (fa_prefill_varlen_sink_f16 / _bf16 of
// include/fa_mi355x.h): the same argument list with `const float* sinks` after
// `window`, the same entry body (csrc/fa_prefill_host.hpp) with WIN = SINK =
// true, launching the Sinked<Windowed<>> instantiations of
// csrc/fa_prefill_kernel.hpp.  A unit of its own so that the
// build stays parallel.
#include "fa_prefill_host.hpp"

using namespace fa;

extern "C" int fa_prefill_varlen_sink_f16(const void* q, const void* k, const void* v, void* o,
    float* lse, int batch, int heads_q, int heads_kv, int total_q, int kv_capacity, int head_dim,
    const int* kv_lens, const int* cu_seqlens_q, int causal, int window, const float* sinks,
    void* hip_stream) {
  return prefill_entry<false, false, true, true, true>(FA_DTYPE_F16, q, k, v, o, lse, batch,
      heads_q, heads_kv, total_q, kv_capacity, head_dim, {}, kv_lens, cu_seqlens_q, causal, window,
      hip_stream, nullptr, nullptr, sinks);
}

extern "C" int fa_prefill_varlen_sink_bf16(const void* q, const void* k, const void* v, void* o,
    float* lse, int batch, int heads_q, int heads_kv, int total_q, int kv_capacity, int head_dim,
    const int* kv_lens, const int* cu_seqlens_q, int causal, int window, const float* sinks,
    void* hip_stream) {
  return prefill_entry<false, false, true, true, true>(FA_DTYPE_BF16, q, k, v, o, lse, batch,
      heads_q, heads_kv, total_q, kv_capacity, head_dim, {}, kv_lens, cu_seqlens_q, causal, window,
      hip_stream, nullptr, nullptr, sinks);
}
