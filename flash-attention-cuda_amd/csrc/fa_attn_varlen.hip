// fa_attn_varlen.hip -- attention over token-major Q, K and V with no cache
// (fa_attn_varlen_f16 / _bf16 of include/fa_mi355x.h): ragged batches by
// cu_seqlens_q / cu_seqlens_k, self-attention, or uniform [B][S][H][D]; GQA;
// runtime token strides.  The entry body is csrc/fa_attn_varlen_host.hpp,
// launching the PrefillPacked<PrefillTokenKV> instantiations of
// csrc/fa_prefill_kernel.hpp.
#include "fa_attn_varlen_host.hpp"

using namespace fa;

#define FA_ATTN_VARLEN(SUFFIX, DTYPE)                                                                 \
  extern "C" int fa_attn_varlen_##SUFFIX(                                                             \
      const void* q, const void* k, const void* v, void* o, float* lse, int batch, int heads_q,       \
      int heads_kv, int total_q, int total_k, int head_dim, long long q_stride, long long k_stride,   \
      long long v_stride, const int* cu_seqlens_q, const int* cu_seqlens_k, int seqlen_q,             \
      int seqlen_k, int causal, void* hip_stream) {                                                   \
    return attn_varlen_entry<>(DTYPE, q, k, v, o, lse, batch, heads_q, heads_kv, total_q, total_k,    \
        head_dim, q_stride, k_stride, v_stride, cu_seqlens_q, cu_seqlens_k, seqlen_q, seqlen_k,       \
        causal, 0, hip_stream);                                                                       \
  }
FA_ATTN_VARLEN(f16, FA_DTYPE_F16)
FA_ATTN_VARLEN(bf16, FA_DTYPE_BF16)
#undef FA_ATTN_VARLEN
