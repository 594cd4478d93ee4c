// fa_attn_bwd.hip -- backward pass (dQ, dK, dV) of the attention over token-major
// Q, K and V (fa_attn_varlen_bwd_f16 of include/fa_mi355x.h).  The entry body
// is csrc/fa_attn_bwd_host.hpp, launching the three kernels of
// csrc/fa_attn_bwd_kernel.hpp.
#include "fa_attn_bwd_host.hpp"

using namespace fa;

extern "C" int fa_attn_varlen_bwd_f16(
    const void* dout, const void* q, const void* k, const void* v, const void* out, const float* lse,
    void* dq, void* dk, void* dv, float* delta, int batch, int heads_q, int heads_kv, int total_q,
    int total_k, int head_dim, long long do_stride, long long q_stride, long long k_stride,
    long long v_stride, const int* cu_seqlens_q, const int* cu_seqlens_k, int seqlen_q, int seqlen_k,
    int causal, void* hip_stream) {
  return attn_varlen_bwd_entry<f16>(dout, q, k, v, out, lse, dq, dk, dv, delta, batch, heads_q, heads_kv,
      total_q, total_k, head_dim, do_stride, q_stride, k_stride, v_stride, cu_seqlens_q, cu_seqlens_k,
      seqlen_q, seqlen_k, causal, hip_stream);
}
