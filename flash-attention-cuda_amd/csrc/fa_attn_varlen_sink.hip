// fa_attn_varlen_sink.hip -- the attention-sink twins of fa_attn_varlen_win.hip's
// entries (fa_attn_varlen_sink_f16 / _bf16 of include/fa_mi355x.h): the same
// argument list with `const float* sinks` last, the same entry body
// (csrc/fa_attn_varlen_host.hpp) with WIN = SINK = true, launching the
// PrefillPacked<Sinked<Windowed<PrefillTokenKV>>> instantiations of
// csrc/fa_prefill_kernel.hpp.  A unit of its own so that the
// build stays parallel.
#include "fa_attn_varlen_host.hpp"

using namespace fa;

#define FA_ATTN_VARLEN_SINK(SUFFIX, DTYPE)                                                            \
  extern "C" int fa_attn_varlen_sink_##SUFFIX(                                                        \
      const void* q, const void* k, const void* v, void* o, float* lse, int batch, int heads_q,       \
      int heads_kv, int total_q, int total_k, int head_dim, long long q_stride, long long k_stride,   \
      long long v_stride, const int* cu_seqlens_q, const int* cu_seqlens_k, int seqlen_q,             \
      int seqlen_k, int causal, int window, void* hip_stream, const float* sinks) {                   \
    return attn_varlen_entry<true, true>(DTYPE, q, k, v, o, lse, batch, heads_q, heads_kv, total_q,   \
        total_k, head_dim, q_stride, k_stride, v_stride, cu_seqlens_q, cu_seqlens_k, seqlen_q,        \
        seqlen_k, causal, window, hip_stream, sinks);                                                 \
  }
FA_ATTN_VARLEN_SINK(f16, FA_DTYPE_F16)
FA_ATTN_VARLEN_SINK(bf16, FA_DTYPE_BF16)
#undef FA_ATTN_VARLEN_SINK
