// fa_prefill_varlen_kv8.hip -- the packed (cu_seqlens, token-major Q) prefill
// entries of include/fa_mi355x.h over a contiguous FP8 (OCP E4M3) K/V cache
// (fa_prefill_varlen_kv8_f16 / _bf16): the entry body of
// fa_prefill_kv8.hip (csrc/fa_prefill_host.hpp) with VARLEN = true, launching the
// PrefillPacked instantiations of csrc/fa_prefill_kernel.hpp.
#include "fa_prefill_host.hpp"

using namespace fa;

#define FA_PREFILL_VARLEN(SUFFIX, DTYPE)                                                              \
  extern "C" int fa_prefill_varlen_kv8_##SUFFIX(                                                      \
      const void* q, const void* k, const void* v, void* o, float* lse, int batch,                    \
      int heads_q, int heads_kv, int total_q, int kv_capacity, int head_dim, const int* kv_lens,      \
      const int* cu_seqlens_q, int causal, void* hip_stream, const float* k_scale,                    \
      const float* v_scale) {                                                                         \
    return prefill_entry<false, true, true>(DTYPE, q, k, v, o, lse, batch, heads_q, heads_kv,         \
        total_q, kv_capacity, head_dim, {}, kv_lens, cu_seqlens_q, causal, 0, hip_stream, k_scale,    \
        v_scale);                                                                                     \
  }
FA_PREFILL_VARLEN(f16, FA_DTYPE_F16)
FA_PREFILL_VARLEN(bf16, FA_DTYPE_BF16)
#undef FA_PREFILL_VARLEN
