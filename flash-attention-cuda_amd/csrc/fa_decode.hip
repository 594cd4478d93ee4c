// fa_decode.hip -- the decode-attention entries of include/fa_mi355x.h over a
// contiguous 16-bit K/V cache (fa_decode_f16 / fa_decode_bf16), plus the split
// plan and the workspace size that all decode entries share.  The entry body,
// the launcher, geometry, plan and workspace layout are csrc/fa_decode_host.hpp;
// the kernel is csrc/fa_decode_kernel.hpp.  It is not a tile config:
// fa_config_info() does not list it.
#include "fa_decode_host.hpp"

using namespace fa;

extern "C" int fa_decode_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                             int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                             int head_dim, const int* kv_lens, int causal, int num_splits,
                             void* workspace, unsigned long long ws_bytes, void* hip_stream) {
  return decode_entry<false, false>(FA_DTYPE_F16, q, k, v, o, lse, batch, heads_q, heads_kv, seqlen_q,
                                    kv_capacity, head_dim, {}, kv_lens, causal, 0, num_splits, workspace,
                                    ws_bytes, hip_stream, nullptr, nullptr);
}

extern "C" int fa_decode_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                              int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                              int head_dim, const int* kv_lens, int causal, int num_splits,
                              void* workspace, unsigned long long ws_bytes, void* hip_stream) {
  return decode_entry<false, false>(FA_DTYPE_BF16, q, k, v, o, lse, batch, heads_q, heads_kv, seqlen_q,
                                    kv_capacity, head_dim, {}, kv_lens, causal, 0, num_splits, workspace,
                                    ws_bytes, hip_stream, nullptr, nullptr);
}

extern "C" int fa_decode_num_splits(int batch, int heads_q, int heads_kv, int seqlen_q,
                                    int kv_capacity, int head_dim) {
  if (head_dim != 128 && head_dim != 64) return 1;
  return decode_plan(decode_geom(batch, heads_q, heads_kv, seqlen_q), kv_capacity);
}

extern "C" unsigned long long fa_decode_ws_bytes(int batch, int heads_q, int heads_kv, int seqlen_q,
                                                 int kv_capacity, int head_dim, int num_splits) {
  if (head_dim != 128 && head_dim != 64) return 0;
  const DecodeGeom ge = decode_geom(batch, heads_q, heads_kv, seqlen_q);
  if (!ge.ok || kv_capacity <= 0 || num_splits < 0 || num_splits > kDecodeMaxSplits) return 0;
  return decode_ws_total(ge, head_dim, num_splits > 0 ? num_splits : decode_plan(ge, kv_capacity));
}
