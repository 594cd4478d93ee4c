// fa_prefill.hip -- the prefill-attention entries of include/fa_mi355x.h over a
// contiguous 16-bit K/V cache (fa_prefill_f16 / fa_prefill_bf16): the entry
// body of csrc/fa_prefill_host.hpp launching csrc/fa_prefill_kernel.hpp with
// PAGED = false and KV = T.
#include "fa_prefill_host.hpp"

using namespace fa;

extern "C" int fa_prefill_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                              int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                              int head_dim, const int* kv_lens, const int* q_lens, int causal,
                              void* hip_stream) {
  return prefill_entry<false, false>(FA_DTYPE_F16, q, k, v, o, lse, batch, heads_q, heads_kv, seqlen_q,
                                     kv_capacity, head_dim, {}, kv_lens, q_lens, causal, 0, hip_stream,
                                     nullptr, nullptr);
}

extern "C" int fa_prefill_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                               int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                               int head_dim, const int* kv_lens, const int* q_lens, int causal,
                               void* hip_stream) {
  return prefill_entry<false, false>(FA_DTYPE_BF16, q, k, v, o, lse, batch, heads_q, heads_kv, seqlen_q,
                                     kv_capacity, head_dim, {}, kv_lens, q_lens, causal, 0, hip_stream,
                                     nullptr, nullptr);
}
