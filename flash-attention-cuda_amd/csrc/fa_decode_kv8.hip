// fa_decode_kv8.hip -- the decode-attention entries of include/fa_mi355x.h over
// a contiguous FP8 (OCP E4M3) K/V cache (fa_decode_kv8_f16 /
// fa_decode_kv8_bf16): the body of the 16-bit entries
// (csrc/fa_decode_host.hpp) with one byte per cache element and one fp32 scale
// per K/V head for K and for V, launching csrc/fa_decode_kernel.hpp with
// KV = unsigned char.
#include "fa_decode_host.hpp"

using namespace fa;

extern "C" int fa_decode_kv8_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                                 int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                                 int head_dim, const int* kv_lens, int causal, int num_splits,
                                 void* workspace, unsigned long long ws_bytes, void* hip_stream,
                                 const float* k_scale, const float* v_scale) {
  return decode_entry<false, true>(FA_DTYPE_F16, q, k, v, o, lse, batch, heads_q, heads_kv, seqlen_q,
                                   kv_capacity, head_dim, {}, kv_lens, causal, 0, num_splits, workspace,
                                   ws_bytes, hip_stream, k_scale, v_scale);
}

extern "C" int fa_decode_kv8_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                                  int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                                  int head_dim, const int* kv_lens, int causal, int num_splits,
                                  void* workspace, unsigned long long ws_bytes, void* hip_stream,
                                  const float* k_scale, const float* v_scale) {
  return decode_entry<false, true>(FA_DTYPE_BF16, q, k, v, o, lse, batch, heads_q, heads_kv, seqlen_q,
                                   kv_capacity, head_dim, {}, kv_lens, causal, 0, num_splits, workspace,
                                   ws_bytes, hip_stream, k_scale, v_scale);
}
