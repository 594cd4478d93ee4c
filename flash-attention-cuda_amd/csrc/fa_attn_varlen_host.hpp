// Host side of the fa_attn_varlen_* entries of include/fa_mi355x.h: attention
// over token-major Q, K and V with no cache, the sibling of
// fa_prefill_host.hpp.  One entry body (attn_varlen_entry, stamped into C
// entries by FA_ATTN_VARLEN_ENTRIES below) over the
// PrefillPacked<[Sinked<Windowed<]PrefillTokenKV[>>]> instantiations of
// fa_prefill_kernel.hpp; prefill_entry's checks in prefill_entry's order, with
// the strides and the two modes (cu_seqlens / uniform) where the page geometry
// stands there.  No workspace, no sync, nothing read from the device: the grid
// is heads_q * (total_q / 128 + batch) workgroups, from shapes alone.
#pragma once

#include "fa_prefill_host.hpp"

namespace fa {

// 0 = dense; otherwise a multiple of 8 elements (16-byte loads) that is no
// shorter than one token's heads * head_dim elements (`dense`).  *bytes: the
// stride the kernel steps by.  `rows`: the rows one descriptor spans, whose
// byte range ((rows - 1) * stride + one row) has to fit a 32-bit int (it is a
// multiple of 16, so that is: not past kBelowWindow, which it must not reach).
inline bool attn_stride_ok(long long stride, long long dense, int rows, int head_dim, int* bytes) {
  if (stride < 0 || stride % 8 != 0) return false;
  const long long s = stride ? stride : dense;
  if ((rows - 1) * s * 2 + 2 * head_dim > (long long)kBelowWindow) return false;
  *bytes = (int)(s * 2);
  return true;
}

// WIN / SINK: as for prefill_entry (the fa_attn_varlen_win_* / _sink_* entries).
template <bool WIN, bool SINK>
static int attn_varlen_entry(int dtype, const void* q, const void* k, const void* v, void* o, float* lse,
                             int batch, int heads_q, int heads_kv, int total_q, int total_k,
                             int head_dim, long long q_stride, long long k_stride, long long v_stride,
                             const int* cu_q, const int* cu_k, int seqlen_q, int seqlen_k, int causal,
                             int window, const float* sinks, void* hip_stream) {
  static_assert(WIN || !SINK, "the sink kernels are instantiated over the windowed ones");
  using P = std::conditional_t<SINK, Sinked<Windowed<PrefillTokenKV>>,
                               std::conditional_t<WIN, Windowed<PrefillTokenKV>, PrefillTokenKV>>;
  if (batch < 0 || heads_q < 0 || heads_kv < 0 || total_k < 0 || head_dim < 0) return FA_ERR_BAD_SHAPE;
  if (WIN && window < 0) return FA_ERR_BAD_SHAPE;
  if (head_dim != 128 && head_dim != 64) return FA_ERR_UNSUPPORTED_HEAD_DIM;
  if (total_q < 0) return FA_ERR_BAD_SHAPE;
  if (WIN && window > 0 && !causal) return FA_ERR_BAD_SHAPE;
  // the strides: 16-byte loads, and one block's rows in a 32-bit byte range
  int q_sb = 0, k_sb = 0, v_sb = 0;
  if (!attn_stride_ok(q_stride, (long long)heads_q * head_dim, kPrefillBM, head_dim, &q_sb) ||
      !attn_stride_ok(k_stride, (long long)heads_kv * head_dim, 64, head_dim, &k_sb) ||
      !attn_stride_ok(v_stride, (long long)heads_kv * head_dim, 64, head_dim, &v_sb))
    return FA_ERR_BAD_SHAPE;
  // the modes: both cu arrays, cu_seqlens_q alone (self-attention: the keys'
  // spans are the queries'), or neither (uniform lengths, totals = B * seqlen)
  if (cu_k && !cu_q) return FA_ERR_BAD_SHAPE;
  if (!cu_q) {
    if (seqlen_q < 0 || seqlen_k < 0) return FA_ERR_BAD_SHAPE;
    if ((long long)batch * seqlen_q != total_q || (long long)batch * seqlen_k != total_k)
      return FA_ERR_BAD_SHAPE;
  }
  if (batch == 0 || heads_q == 0 || total_q == 0) return FA_OK;
  if (heads_kv == 0 || heads_q % heads_kv != 0) return FA_ERR_BAD_SHAPE;
  // a given stride shorter than a token's heads: rows would overlap
  if ((q_stride && q_stride < (long long)heads_q * head_dim) ||
      (k_stride && k_stride < (long long)heads_kv * head_dim) ||
      (v_stride && v_stride < (long long)heads_kv * head_dim))
    return FA_ERR_BAD_SHAPE;
  // LSE rows, and the byte range of one block's dense O rows
  if ((long long)heads_q * total_q > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  if ((long long)kPrefillBM * heads_q * 2 * head_dim > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  // key indices (up to the end of the last tile) are 32-bit ints in the kernel
  if (total_k > 0x7fffffff - 64) return FA_ERR_BAD_SHAPE;
  const long long nqb = (long long)total_q / kPrefillBM + batch;  // virtual block ids per head
  const long long nwg = heads_q * nqb;
  if (nqb > 0x7fffffffLL || nwg > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  hipStream_t stream = (hipStream_t)hip_stream;
  if (total_k == 0)
    return decode_empty_cache<SINK, true>(o, lse, sinks, (size_t)heads_q * total_q, heads_q, total_q,
                                          head_dim, stream);
  if (!q || !k || !v || !o) return FA_ERR_NULL_POINTER;
  P p = {};
  p.q = q;
  p.k = k;
  p.v = v;
  p.o = o;
  p.lse = lse;
  p.q_lens = cu_q;
  p.cu_k = cu_q ? (cu_k ? cu_k : cu_q) : nullptr;
  p.useq_q = seqlen_q;
  p.useq_k = seqlen_k;
  p.q_sb = q_sb;
  p.k_sb = k_sb;
  p.v_sb = v_sb;
  p.hq = heads_q;
  p.hkv = heads_kv;
  p.sq = total_q;
  p.cap = total_k;
  p.group = heads_q / heads_kv;
  p.nqb = batch;  // the kernel takes the sequence count here
  p.causal = causal ? 1 : 0;
  p.c = 1.4426950408889634f / sqrtf((float)head_dim);
  decode_set_variant<false, WIN, SINK>(p, total_k, window, sinks, nullptr, nullptr);
  const unsigned grid = (unsigned)nwg;
  return dispatch_elem_dim(dtype, head_dim, [&](auto e) {
    using E = decltype(e);
    return prefill_launch_inst<typename E::type, E::hdim, false, false, true>(p, grid, stream);
  });
}

}  // namespace fa

// PREFIX_f16 and PREFIX_bf16 of include/fa_mi355x.h, the variant's groups from
// fa_decode_host.hpp (`sinks` comes last here):
// FA_ATTN_VARLEN_ENTRIES(fa_attn_varlen_sink, SINK).
#define FA_ATTN_VARLEN_ENTRY(NAME, DTYPE, VARIANT)                                                  \
  extern "C" int NAME(const void* q, const void* k, const void* v, void* o, float* lse, int batch,  \
                      int heads_q, int heads_kv, int total_q, int total_k, int head_dim,            \
                      long long q_stride, long long k_stride, long long v_stride,                   \
                      const int* cu_seqlens_q, const int* cu_seqlens_k, int seqlen_q, int seqlen_k, \
                      int causal FA_##VARIANT##_WINDOW, void* hip_stream FA_##VARIANT##_SINKS) {    \
    return fa::attn_varlen_entry<FA_##VARIANT##_FLAGS>(                                             \
        DTYPE, q, k, v, o, lse, batch, heads_q, heads_kv, total_q, total_k, head_dim, q_stride,     \
        k_stride, v_stride, cu_seqlens_q, cu_seqlens_k, seqlen_q, seqlen_k, causal,                 \
        FA_##VARIANT##_ARGS, hip_stream);                                                           \
  }
#define FA_ATTN_VARLEN_ENTRIES(PREFIX, VARIANT)                 \
  FA_ATTN_VARLEN_ENTRY(PREFIX##_f16, FA_DTYPE_F16, VARIANT)     \
  FA_ATTN_VARLEN_ENTRY(PREFIX##_bf16, FA_DTYPE_BF16, VARIANT)
