// Host side of the fa_attn_varlen_bwd_* entries of include/fa_mi355x.h and of
// their sliding-window and attention-sink twins, fa_attn_bwd_win_* and
// fa_attn_bwd_sink_*: the backward pass of the attention over token-major Q, K
// and V.  One entry body (attn_varlen_bwd_entry,
// stamped into C entries by FA_ATTN_BWD_ENTRY below); attn_varlen_entry's
// checks in attn_varlen_entry's order, then three launches on the caller's
// stream (delta, dK/dV, dQ: fa_attn_bwd_kernel.hpp) and, with sinks, a fourth
// (dsinks).  No sync, nothing read from the device, no workspace but the
// caller's delta: the grids are total_q / 128 + batch, heads_kv * (total_k /
// 128 + batch), heads_q * (total_q / 128 + batch) and heads_q workgroups, from
// shapes alone.
#pragma once

#include "fa_attn_bwd_kernel.hpp"
#include "fa_attn_varlen_host.hpp"

namespace fa {

// P: AttnBwdParams, or Windowed<AttnBwdParams> for the _win kernels
template <class T, int HDIM, class P>
static int attn_bwd_launch(const P& p, unsigned g_delta, unsigned g_dkdv, unsigned g_dq,
                           hipStream_t stream) {
  hipLaunchKernelGGL((fa_attn_bwd_delta_kernel<T, HDIM>), dim3(g_delta), dim3(256), 0, stream, p);
  if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
  hipLaunchKernelGGL((fa_attn_bwd_dkdv_kernel<T, HDIM, P>), dim3(g_dkdv), dim3(256), 0, stream, p);
  if (hipGetLastError() != hipSuccess) return FA_ERR_LAUNCH;
  hipLaunchKernelGGL((fa_attn_bwd_dq_kernel<T, HDIM, P>), dim3(g_dq), dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
}

// dsinks, where the caller gave it, of a problem without a row or without a key: zeros
static inline bool attn_bwd_zero_dsinks(float* dsinks, int heads_q, hipStream_t stream) {
  return !dsinks || hipMemsetAsync(dsinks, 0, (size_t)heads_q * sizeof(float), stream) == hipSuccess;
}

// T: the element type (one translation unit per type, so the two compile in
// parallel).  WIN / SINK: as for attn_varlen_entry (the fa_attn_bwd_win_* /
// _sink_* entries).  SINK: `sinks` NULL is the _win entry, and `dsinks` is then
// zero-filled if it is given; with `sinks`, `dsinks` is required and written.
template <class T, bool WIN, bool SINK>
static int attn_varlen_bwd_entry(const void* dout, const void* q, const void* k, const void* v,
                                 const void* out, const float* lse, void* dq, void* dk, void* dv,
                                 float* delta, int batch, int heads_q, int heads_kv, int total_q,
                                 int total_k, int head_dim, long long do_stride, long long q_stride,
                                 long long k_stride, long long v_stride, const int* cu_q, const int* cu_k,
                                 int seqlen_q, int seqlen_k, int causal, [[maybe_unused]] int window,
                                 [[maybe_unused]] const float* sinks, [[maybe_unused]] float* dsinks,
                                 void* hip_stream) {
  static_assert(WIN || !SINK, "the sink entries run the windowed kernels");
  using P = std::conditional_t<WIN, Windowed<AttnBwdParams>, AttnBwdParams>;
  if (batch < 0 || heads_q < 0 || heads_kv < 0 || total_k < 0 || head_dim < 0) return FA_ERR_BAD_SHAPE;
  if (WIN && window < 0) return FA_ERR_BAD_SHAPE;
  if (head_dim != 128 && head_dim != 64) return FA_ERR_UNSUPPORTED_HEAD_DIM;
  if (total_q < 0) return FA_ERR_BAD_SHAPE;
  if (WIN && window > 0 && !causal) return FA_ERR_BAD_SHAPE;
  // the strides: 16-byte loads, and one block's rows (128 of each tensor here:
  // a workgroup addresses its 128 keys from the block's first as it does its
  // 128 query rows) in a 32-bit byte range
  int do_sb = 0, q_sb = 0, k_sb = 0, v_sb = 0;
  if (!attn_stride_ok(do_stride, (long long)heads_q * head_dim, kBwdBM, head_dim, &do_sb) ||
      !attn_stride_ok(q_stride, (long long)heads_q * head_dim, kBwdBM, head_dim, &q_sb) ||
      !attn_stride_ok(k_stride, (long long)heads_kv * head_dim, kBwdBN, head_dim, &k_sb) ||
      !attn_stride_ok(v_stride, (long long)heads_kv * head_dim, kBwdBN, head_dim, &v_sb))
    return FA_ERR_BAD_SHAPE;
  if (cu_k && !cu_q) return FA_ERR_BAD_SHAPE;
  if (!cu_q) {
    if (seqlen_q < 0 || seqlen_k < 0) return FA_ERR_BAD_SHAPE;
    if ((long long)batch * seqlen_q != total_q || (long long)batch * seqlen_k != total_k)
      return FA_ERR_BAD_SHAPE;
  }
  hipStream_t stream = (hipStream_t)hip_stream;
  if (heads_q == 0) return FA_OK;
  if (batch == 0 || total_q == 0) {
    // no query row: every key's gradient is zero
    const size_t bytes = (size_t)total_k * (size_t)heads_kv * head_dim * 2;
    if constexpr (SINK)
      if (!attn_bwd_zero_dsinks(dsinks, heads_q, stream)) return FA_ERR_HIP;
    if (bytes == 0) return FA_OK;
    if (!dk || !dv) return FA_ERR_NULL_POINTER;
    if (hipMemsetAsync(dk, 0, bytes, stream) != hipSuccess) return FA_ERR_HIP;
    return hipMemsetAsync(dv, 0, bytes, stream) == hipSuccess ? FA_OK : FA_ERR_HIP;
  }
  if (heads_kv == 0 || heads_q % heads_kv != 0) return FA_ERR_BAD_SHAPE;
  if ((do_stride && do_stride < (long long)heads_q * head_dim) ||
      (q_stride && q_stride < (long long)heads_q * head_dim) ||
      (k_stride && k_stride < (long long)heads_kv * head_dim) ||
      (v_stride && v_stride < (long long)heads_kv * head_dim))
    return FA_ERR_BAD_SHAPE;
  // LSE / delta rows, and the byte range of one block's dense dQ, dK and dV rows
  if ((long long)heads_q * total_q > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  if ((long long)kBwdBM * heads_q * 2 * head_dim > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  if ((long long)kBwdBN * heads_kv * 2 * head_dim > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  if (total_k > 0x7fffffff - 64) return FA_ERR_BAD_SHAPE;
  // the windowed kernels form off + row - W and key + W from ints
  if (WIN && (long long)total_q + total_k > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  const long long nqb = (long long)total_q / kBwdBM + batch;
  const long long nkb = (long long)total_k / kBwdBN + batch;
  if (nqb > 0x7fffffffLL || heads_q * nqb > 0x7fffffffLL || heads_kv * nkb > 0x7fffffffLL)
    return FA_ERR_BAD_SHAPE;
  if (total_k == 0) {
    // rows but no keys: dQ = 0 for every row (and out = 0, so delta = 0: dsinks = 0)
    if (!dq) return FA_ERR_NULL_POINTER;
    if constexpr (SINK)
      if (!attn_bwd_zero_dsinks(dsinks, heads_q, stream)) return FA_ERR_HIP;
    return hipMemsetAsync(dq, 0, (size_t)total_q * (size_t)heads_q * head_dim * 2, stream) == hipSuccess
               ? FA_OK
               : FA_ERR_HIP;
  }
  if (!dout || !q || !k || !v || !out || !dq || !dk || !dv) return FA_ERR_NULL_POINTER;
  if (!lse || !delta) return FA_ERR_NULL_POINTER;
  if constexpr (SINK)
    if (sinks && !dsinks) return FA_ERR_NULL_POINTER;
  P p = {};
  p.dout = dout, p.q = q, p.k = k, p.v = v, p.out = out, p.lse = lse;
  p.dq = dq, p.dk = dk, p.dv = dv, p.delta = delta;
  p.cu_q = cu_q;
  p.cu_k = cu_q ? (cu_k ? cu_k : cu_q) : nullptr;
  p.useq_q = seqlen_q, p.useq_k = seqlen_k;
  p.do_sb = do_sb, p.q_sb = q_sb, p.k_sb = k_sb, p.v_sb = v_sb;
  p.hq = heads_q, p.hkv = heads_kv, p.group = heads_q / heads_kv;
  p.tq = total_q, p.tk = total_k, p.nseq = batch;
  p.causal = causal ? 1 : 0;
  p.c = 1.0f / sqrtf((float)head_dim);
  // no window (and so every non-causal call): W = total_k, which excludes no key
  if constexpr (WIN) p.window = window > 0 ? std::min(window, total_k) : total_k;
  const unsigned gd = (unsigned)nqb, gk = (unsigned)(heads_kv * nkb), gq = (unsigned)(heads_q * nqb);
  const int rc = head_dim == 128 ? attn_bwd_launch<T, 128>(p, gd, gk, gq, stream)
                                 : attn_bwd_launch<T, 64>(p, gd, gk, gq, stream);
  if constexpr (SINK) {
    if (rc != FA_OK) return rc;
    if (!sinks) return attn_bwd_zero_dsinks(dsinks, heads_q, stream) ? FA_OK : FA_ERR_HIP;
    AttnBwdSinkParams sp = {};
    sp.lse = lse, sp.delta = delta, sp.sinks = sinks, sp.dsinks = dsinks;
    sp.cu_q = cu_q, sp.useq_q = seqlen_q, sp.nseq = batch, sp.tq = total_q;
    hipLaunchKernelGGL((fa_attn_bwd_dsinks_kernel<kBwdSinkThreads>), dim3((unsigned)heads_q),
                       dim3(kBwdSinkThreads), 0, stream, sp);
    return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
  }
  return rc;
}

}  // namespace fa

// NAME of include/fa_mi355x.h over element type T, the variant's window group
// and flags from fa_decode_host.hpp; the sink entries take `sinks` and `dsinks`
// after the stream: FA_ATTN_BWD_ENTRY(fa_attn_bwd_sink_f16, fa::f16, SINK).
#define FA_BWD_PLAIN_SINKS
#define FA_BWD_PLAIN_ARGS 0, nullptr, nullptr
#define FA_BWD_WIN_SINKS
#define FA_BWD_WIN_ARGS window, nullptr, nullptr
#define FA_BWD_SINK_SINKS , const float* sinks, float* dsinks
#define FA_BWD_SINK_ARGS window, sinks, dsinks
#define FA_ATTN_BWD_ENTRY(NAME, T, VARIANT)                                                           \
  extern "C" int NAME(const void* dout, const void* q, const void* k, const void* v, const void* out, \
                      const float* lse, void* dq, void* dk, void* dv, float* delta, int batch,        \
                      int heads_q, int heads_kv, int total_q, int total_k, int head_dim,              \
                      long long do_stride, long long q_stride, long long k_stride,                    \
                      long long v_stride, const int* cu_seqlens_q, const int* cu_seqlens_k,           \
                      int seqlen_q, int seqlen_k, int causal FA_##VARIANT##_WINDOW,                   \
                      void* hip_stream FA_BWD_##VARIANT##_SINKS) {                                    \
    return fa::attn_varlen_bwd_entry<T, FA_##VARIANT##_FLAGS>(                                        \
        dout, q, k, v, out, lse, dq, dk, dv, delta, batch, heads_q, heads_kv, total_q, total_k,       \
        head_dim, do_stride, q_stride, k_stride, v_stride, cu_seqlens_q, cu_seqlens_k, seqlen_q,      \
        seqlen_k, causal, FA_BWD_##VARIANT##_ARGS, hip_stream);                                       \
  }
