// fa_decode_sink_kv8.hip -- the attention-sink twins of fa_decode_win_kv8.hip's
// entries (fa_decode_sink_kv8_f16 / _bf16 of include/fa_mi355x.h): the same
// argument list with `const float* sinks` after `window`, the same entry body
// (csrc/fa_decode_host.hpp) with WIN = SINK = true, launching the
// Sinked<Windowed<>> instantiations of csrc/fa_decode_kernel.hpp (DESIGN.md
// §3.0n).  A unit of its own so that the build stays parallel.
#include "fa_decode_host.hpp"

using namespace fa;

extern "C" int fa_decode_sink_kv8_f16(const void* q, const void* k, const void* v, void* o,
    float* lse, int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity, int head_dim,
    const int* kv_lens, int causal, int window, const float* sinks, int num_splits, void* workspace,
    unsigned long long ws_bytes, void* hip_stream, const float* k_scale, const float* v_scale) {
  return decode_entry<false, true, true, true>(FA_DTYPE_F16, q, k, v, o, lse, batch, heads_q,
      heads_kv, seqlen_q, kv_capacity, head_dim, {}, kv_lens, causal, window, num_splits, workspace,
      ws_bytes, hip_stream, k_scale, v_scale, sinks);
}

extern "C" int fa_decode_sink_kv8_bf16(const void* q, const void* k, const void* v, void* o,
    float* lse, int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity, int head_dim,
    const int* kv_lens, int causal, int window, const float* sinks, int num_splits, void* workspace,
    unsigned long long ws_bytes, void* hip_stream, const float* k_scale, const float* v_scale) {
  return decode_entry<false, true, true, true>(FA_DTYPE_BF16, q, k, v, o, lse, batch, heads_q,
      heads_kv, seqlen_q, kv_capacity, head_dim, {}, kv_lens, causal, window, num_splits, workspace,
      ws_bytes, hip_stream, k_scale, v_scale, sinks);
}
