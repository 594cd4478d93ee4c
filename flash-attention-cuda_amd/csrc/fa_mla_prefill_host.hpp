// Host side of the fa_mla_prefill_varlen_* entries of
// include/fa_mi355x_mla_prefill.h: attention over token-major Q, K and V with
// 192-dim queries / keys, 128-dim values and the caller's softmax scale
// (DESIGN.md §3.0v).  One entry body and the macro that stamps the two C
// entries; attn_varlen_entry's checks in attn_varlen_entry's order, with
// softmax_scale checked where the MLA decode entries check theirs.  No
// workspace, no sync, nothing read from the device: the grid is heads_q *
// (total_q / 128 + batch) workgroups, from shapes alone.
#pragma once

#include <string.h>

#include "fa_attn_varlen_host.hpp"
#include "fa_mi355x_mla_prefill.h"
#include "fa_mla_prefill_kernel.hpp"

namespace fa {

template <class T>
static int mla_prefill_launch_inst(const MlaPrefillParams& p, unsigned grid, hipStream_t stream) {
  constexpr auto kernel = fa_mla_prefill_kernel<T>;
  static std::once_flag flags[64];
  static hipError_t errs[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return FA_ERR_HIP;
  std::call_once(flags[dev], [dev] {
    errs[dev] = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    kMlaPfLdsBytes);
  });
  if (errs[dev] != hipSuccess) return FA_ERR_HIP;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), kMlaPfLdsBytes, stream, p);
  return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
}

static int mla_prefill_entry(int dtype, const void* q, const void* k, const void* v, void* o, float* lse,
                             int batch, int heads_q, int heads_kv, int total_q, int total_k,
                             long long q_stride, long long k_stride, long long v_stride, const int* cu_q,
                             const int* cu_k, int seqlen_q, int seqlen_k, int causal, float softmax_scale,
                             void* hip_stream) {
  if (batch < 0 || heads_q < 0 || heads_kv < 0 || total_k < 0) return FA_ERR_BAD_SHAPE;
  {
    // finite and > 0, on the bits: the units are compiled with -fno-honor-nans
    unsigned bits;
    memcpy(&bits, &softmax_scale, 4);
    if ((bits >> 31) != 0 || (bits & 0x7f800000u) == 0x7f800000u || bits == 0) return FA_ERR_BAD_SHAPE;
  }
  if (total_q < 0) return FA_ERR_BAD_SHAPE;
  // the strides: 16-byte loads, and one block's / tile's rows in a 32-bit byte range
  int q_sb = 0, k_sb = 0, v_sb = 0;
  if (!attn_stride_ok(q_stride, (long long)heads_q * kMlaPfDqk, kMlaPfBM, kMlaPfDqk, &q_sb) ||
      !attn_stride_ok(k_stride, (long long)heads_kv * kMlaPfDqk, 64, kMlaPfDqk, &k_sb) ||
      !attn_stride_ok(v_stride, (long long)heads_kv * kMlaPfDv, 64, kMlaPfDv, &v_sb))
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
  if ((q_stride && q_stride < (long long)heads_q * kMlaPfDqk) ||
      (k_stride && k_stride < (long long)heads_kv * kMlaPfDqk) ||
      (v_stride && v_stride < (long long)heads_kv * kMlaPfDv))
    return FA_ERR_BAD_SHAPE;
  // LSE rows, and the byte range of one block's dense O rows
  if ((long long)heads_q * total_q > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  if ((long long)kMlaPfBM * heads_q * kMlaPfVRow > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  // key indices are 32-bit ints in the kernel: up to the end of the last tile,
  // and len - nq + q0 + 128 <= len + 128 where a block's key range is cut
  if (total_k > 0x7fffffff - kMlaPfBM) return FA_ERR_BAD_SHAPE;
  const long long nqb = (long long)total_q / kMlaPfBM + batch;  // virtual block ids per head
  const long long nwg = heads_q * nqb;
  if (nqb > 0x7fffffffLL || nwg > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  hipStream_t stream = (hipStream_t)hip_stream;
  if (total_k == 0)
    return decode_empty_cache<false, true>(o, lse, nullptr, (size_t)heads_q * total_q, heads_q, total_q,
                                           kMlaPfDv, stream);
  if (!q || !k || !v || !o) return FA_ERR_NULL_POINTER;
  MlaPrefillParams p = {};
  p.q = q;
  p.k = k;
  p.v = v;
  p.o = o;
  p.lse = lse;
  p.cu_q = cu_q;
  p.cu_k = cu_q ? (cu_k ? cu_k : cu_q) : nullptr;
  p.useq_q = seqlen_q;
  p.useq_k = seqlen_k;
  p.q_sb = q_sb;
  p.k_sb = k_sb;
  p.v_sb = v_sb;
  p.hq = heads_q;
  p.hkv = heads_kv;
  p.group = heads_q / heads_kv;
  p.tq = total_q;
  p.tk = total_k;
  p.nseq = batch;
  p.causal = causal ? 1 : 0;
  p.c = 1.4426950408889634f * softmax_scale;
  const unsigned grid = (unsigned)nwg;
  return dtype == FA_DTYPE_BF16 ? mla_prefill_launch_inst<__bf16>(p, grid, stream)
                                : mla_prefill_launch_inst<f16>(p, grid, stream);
}

}  // namespace fa

// PREFIX_f16 and PREFIX_bf16 of include/fa_mi355x_mla_prefill.h
#define FA_MLA_PREFILL_ENTRY(NAME, DTYPE)                                                           \
  extern "C" int NAME(const void* q, const void* k, const void* v, void* o, float* lse, int batch,  \
                      int heads_q, int heads_kv, int total_q, int total_k, long long q_stride,      \
                      long long k_stride, long long v_stride, const int* cu_seqlens_q,              \
                      const int* cu_seqlens_k, int seqlen_q, int seqlen_k, int causal,              \
                      float softmax_scale, void* hip_stream) {                                      \
    return fa::mla_prefill_entry(DTYPE, q, k, v, o, lse, batch, heads_q, heads_kv, total_q,         \
                                 total_k, q_stride, k_stride, v_stride, cu_seqlens_q, cu_seqlens_k, \
                                 seqlen_q, seqlen_k, causal, softmax_scale, hip_stream);            \
  }
#define FA_MLA_PREFILL_ENTRIES(PREFIX)               \
  FA_MLA_PREFILL_ENTRY(PREFIX##_f16, FA_DTYPE_F16)   \
  FA_MLA_PREFILL_ENTRY(PREFIX##_bf16, FA_DTYPE_BF16)
