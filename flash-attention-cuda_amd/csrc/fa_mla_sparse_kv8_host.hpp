// Host side of the FP8 MLA sparse entries of include/fa_mi355x_mla_sparse_kv8.h:
// the entry body (mla_sparse_entry's checks in its order; ckv_scale is a device
// pointer, NULL = 1.0, and is never looked at here), the parameters and the
// launch.  The geometry, the split plan and the workspace are MLA decode's with
// batch = tokens and seqlen_q = 1 (mla_geom, mla_plan, decode_ws_total of
// fa_mla_decode_host.hpp), so fa_mla_decode_num_splits and
// fa_mla_decode_ws_bytes answer for these entries.
#pragma once

#include "fa_mi355x_mla_sparse_kv8.h"
#include "fa_mla_decode_host.hpp"
#include "fa_mla_sparse_kv8_kernel.hpp"

namespace fa {

template <class T, bool WIDE>
static int mla_sparse_kv8_launch_inst(const MlaSparseKv8Params& p, unsigned grid, hipStream_t stream) {
  constexpr auto kernel = fa_mla_sparse_kv8_kernel<T, WIDE>;
  constexpr int lds = WIDE ? kMlaSparse8LdsWide : kMlaSparse8LdsNarrow;
  static std::once_flag flags[64];
  static hipError_t errs[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return FA_ERR_HIP;
  std::call_once(flags[dev], [dev] {
    errs[dev] = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  });
  if (errs[dev] != hipSuccess) return FA_ERR_HIP;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, stream, p);
  return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
}

static int mla_sparse_kv8_entry(int dtype, const void* q, const void* ckv8, const int* indices,
                                const float* ckv_scale, void* o, float* lse, int num_tokens, int heads_q,
                                int topk, int num_rows, float softmax_scale, int num_splits, void* ws,
                                unsigned long long ws_bytes, void* hip_stream) {
  if (num_tokens < 0 || heads_q < 0 || topk < 0 || num_rows < 0 || num_splits < 0) return FA_ERR_BAD_SHAPE;
  {
    // finite and > 0, on the bits: the units are compiled with -fno-honor-nans
    unsigned bits;
    memcpy(&bits, &softmax_scale, 4);
    if ((bits >> 31) != 0 || (bits & 0x7f800000u) == 0x7f800000u || bits == 0) return FA_ERR_BAD_SHAPE;
  }
  if (num_tokens == 0 || heads_q == 0) return FA_OK;
  if ((long long)num_tokens * heads_q > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  hipStream_t stream = (hipStream_t)hip_stream;
  if (topk == 0 || num_rows == 0) {
    // every entry is a hole: O = 0, LSE = -inf, and neither the pool, the list nor the scale is looked at
    if (!o) return FA_ERR_NULL_POINTER;
    const size_t nrow = (size_t)num_tokens * heads_q, nwords = nrow * (kMlaDv / 2);
    hipLaunchKernelGGL(fa_mla_fill_empty_kernel<0>, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0,
                       stream, static_cast<unsigned*>(o), lse, nwords, nrow);
    return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
  }
  if (!q || !ckv8 || !indices || !o) return FA_ERR_NULL_POINTER;
  const DecodeGeom ge = mla_geom(num_tokens, heads_q, 1);
  if (num_splits > kDecodeMaxSplits) return FA_ERR_BAD_CONFIG;
  const int ns = num_splits > 0 ? num_splits : mla_plan(ge, topk);
  if (ge.units * ns > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  if (ns > 1) {
    if (ge.units > (long long)(kDecodeCtrBytes / 4)) return FA_ERR_BAD_CONFIG;
    if (!ws || ws_bytes < decode_ws_total(ge, kMlaDv, ns) || (reinterpret_cast<uintptr_t>(ws) & 15) != 0)
      return FA_ERR_WORKSPACE;
  }
  MlaSparseKv8Params p = {};
  p.q = q;
  p.k = ckv8;
  p.v = ckv8;
  p.o = o;
  p.lse = lse;
  p.hq = heads_q;
  p.hkv = 1;
  p.sq = 1;
  p.cap = topk;
  p.group = ge.group;
  p.rows = ge.rows;
  p.rgroups = ge.rgroups;
  p.num_splits = ns;
  p.c = 1.4426950408889634f * softmax_scale;
  if (ns > 1) decode_set_workspace(p, ge, ns, ws);
  p.indices = indices;
  p.topk = topk;
  p.num_rows = num_rows;
  p.k_scale = ckv_scale;
  const unsigned grid = (unsigned)(ge.units * ns);
  const bool wide = ge.nb == 4;
  if (dtype == FA_DTYPE_BF16)
    return wide ? mla_sparse_kv8_launch_inst<__bf16, true>(p, grid, stream)
                : mla_sparse_kv8_launch_inst<__bf16, false>(p, grid, stream);
  return wide ? mla_sparse_kv8_launch_inst<f16, true>(p, grid, stream)
              : mla_sparse_kv8_launch_inst<f16, false>(p, grid, stream);
}

}  // namespace fa

// fa_mla_sparse_kv8_f16 and fa_mla_sparse_kv8_bf16 of include/fa_mi355x_mla_sparse_kv8.h
#define FA_MLA_SPARSE_KV8_ENTRY(NAME, DTYPE)                                                                \
  extern "C" int NAME(const void* q, const void* ckv8, const int* indices, const float* ckv_scale, void* o, \
                      float* lse, int num_tokens, int heads_q, int topk, int num_rows, float softmax_scale, \
                      int num_splits, void* workspace, unsigned long long ws_bytes, void* hip_stream) {     \
    return fa::mla_sparse_kv8_entry(DTYPE, q, ckv8, indices, ckv_scale, o, lse, num_tokens, heads_q, topk,  \
                                    num_rows, softmax_scale, num_splits, workspace, ws_bytes, hip_stream);  \
  }
