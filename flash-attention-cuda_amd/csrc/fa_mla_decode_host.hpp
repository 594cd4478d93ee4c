// Host side of the MLA decode entries of include/fa_mi355x_mla.h, shared by
// the two cache forms (fa_mla_decode.hip: contiguous, fa_mla_decode_paged.hip:
// page pool + block table): the geometry (one latent head, two regimes), the
// decode entries' split plan and workspace layout with head_dim = 512 in the
// slab size, so that one per-stream workspace serves both families, the one
// entry body and the macro that stamps a unit's two C entries.  The body takes
// the cache type as a kernel family (MlaKernels16 here; MlaKernelsKv8 of
// fa_mla_decode_kv8_host.hpp for the E4M3 cache of include/fa_mi355x_mla_kv8.h).
#pragma once

#include <string.h>

#include "fa_decode_host.hpp"
#include "fa_mi355x_mla.h"
#include "fa_mla_decode_kernel.hpp"

namespace fa {

// rows = Hq * Sq over the one latent head: one 16-row block (narrow) or row
// groups of 64 (wide)
inline DecodeGeom mla_geom(int batch, int heads_q, int seqlen_q) {
  DecodeGeom ge;
  if (batch <= 0 || heads_q <= 0 || seqlen_q < 1 || seqlen_q > 16) return ge;
  ge.group = heads_q;
  ge.rows = heads_q * seqlen_q;
  ge.nb = ge.rows <= 16 ? 1 : 4;
  ge.rw = 16 * ge.nb;
  ge.rgroups = (ge.rows + ge.rw - 1) / ge.rw;
  ge.units = (long long)batch * ge.rgroups;
  ge.ok = true;
  return ge;
}

// The decode plan; wide, capped at 8 pieces: the last arriver of a unit merges
// its pieces alone, and a wide piece's slab is 64 x 512 fp32 = 128 KB where
// decode's is at most 32 KB (measured: DESIGN.md §3.0t)
inline int mla_plan(const DecodeGeom& ge, int kv_capacity) {
  const int ns = decode_plan(ge, kv_capacity);
  return ge.nb == 4 ? std::min(ns, 8) : ns;
}

// The 16-bit cache's kernels: what differs between the cache types on the host
struct MlaKernels16 {
  static constexpr bool kKv8 = false;
  static constexpr int kRow = kMlaRow;        // bytes per cache row
  static constexpr int kLds = kMlaLdsBytes;   // dynamic LDS per workgroup
  template <bool PAGED>
  using Params = std::conditional_t<PAGED, DecodePagedParams, DecodeParams>;
  template <class T, bool WIDE, bool PAGED>
  static constexpr auto kernel = fa_mla_decode_kernel<T, WIDE, PAGED, Params<PAGED>>;
};

template <class K, class T, bool WIDE, bool PAGED, class P>
static int mla_launch_inst(const P& p, unsigned grid, hipStream_t stream) {
  constexpr auto kernel = K::template kernel<T, WIDE, PAGED>;
  static std::once_flag flags[64];
  static hipError_t errs[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return FA_ERR_HIP;
  std::call_once(flags[dev], [dev] {
    errs[dev] = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    K::kLds);
  });
  if (errs[dev] != hipSuccess) return FA_ERR_HIP;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), K::kLds, stream, p);
  return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
}

// The body of the MLA decode entries; the statuses and their order are
// decode_entry's where the arguments correspond (softmax_scale is checked
// where that body checks the window).  PAGED: `ckv` is the pool, `pg`
// describes it and kv_capacity (passed as 0) becomes max_pages_per_seq *
// page_size.  K: the cache type's kernels; ckv_scale: the E4M3 cache's scale
// (device float[1] or NULL), read on the device only.
template <bool PAGED, class K = MlaKernels16>
static int mla_decode_entry(int dtype, const void* q, const void* ckv, void* o, float* lse, int batch,
                            int heads_q, int seqlen_q, int kv_capacity, const DecodePages& pg,
                            const int* kv_lens, int causal, float softmax_scale, int num_splits, void* ws,
                            unsigned long long ws_bytes, void* hip_stream,
                            [[maybe_unused]] const float* ckv_scale = nullptr) {
  using P = typename K::template Params<PAGED>;
  if (batch < 0 || heads_q < 0 || kv_capacity < 0 || num_splits < 0) return FA_ERR_BAD_SHAPE;
  if (seqlen_q < 1 || seqlen_q > 16) return FA_ERR_BAD_SHAPE;
  {
    // finite and > 0, on the bits: the units are compiled with -fno-honor-nans
    unsigned bits;
    memcpy(&bits, &softmax_scale, 4);
    if ((bits >> 31) != 0 || (bits & 0x7f800000u) == 0x7f800000u || bits == 0) return FA_ERR_BAD_SHAPE;
  }
  if constexpr (PAGED) {
    if (const int st = decode_check_pages(pg, kMlaDqk, &kv_capacity)) return st;
  }
  if (batch == 0 || heads_q == 0) return FA_OK;
  if ((long long)batch * heads_q * seqlen_q > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  if constexpr (!PAGED) {
    // an element's rows are addressed through one buffer resource whose byte
    // range (cap * 1152, or cap * 576 of bytes) is a 32-bit int
    if ((long long)kv_capacity * K::kRow > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
    if (!kv_lens && causal && kv_capacity < seqlen_q && kv_capacity > 0) return FA_ERR_BAD_SHAPE;
  }
  hipStream_t stream = (hipStream_t)hip_stream;
  const size_t nrow = (size_t)batch * heads_q * seqlen_q;
  if (kv_capacity == 0) {
    if (!o) return FA_ERR_NULL_POINTER;
    const size_t nwords = nrow * (kMlaDv / 2);
    hipLaunchKernelGGL(fa_mla_fill_empty_kernel<0>, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0,
                       stream, static_cast<unsigned*>(o), lse, nwords, nrow);
    return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
  }
  if (!q || !ckv || !o || (PAGED && !pg.block_table)) return FA_ERR_NULL_POINTER;
  const DecodeGeom ge = mla_geom(batch, heads_q, seqlen_q);
  if (num_splits > kDecodeMaxSplits) return FA_ERR_BAD_CONFIG;
  const int ns = num_splits > 0 ? num_splits : mla_plan(ge, kv_capacity);
  if (ge.units * ns > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  if (ns > 1) {
    if (ge.units > (long long)(kDecodeCtrBytes / 4)) return FA_ERR_BAD_CONFIG;
    if (!ws || ws_bytes < decode_ws_total(ge, kMlaDv, ns) || (reinterpret_cast<uintptr_t>(ws) & 15) != 0)
      return FA_ERR_WORKSPACE;
  }
  P p = {};
  p.q = q;
  p.k = ckv;
  p.v = ckv;
  p.o = o;
  p.lse = lse;
  p.kv_lens = kv_lens;
  p.hq = heads_q;
  p.hkv = 1;
  p.sq = seqlen_q;
  p.cap = kv_capacity;
  p.group = ge.group;
  p.rows = ge.rows;
  p.rgroups = ge.rgroups;
  p.num_splits = ns;
  p.causal = causal ? 1 : 0;
  p.c = 1.4426950408889634f * softmax_scale;
  if (ns > 1) decode_set_workspace(p, ge, ns, ws);
  if constexpr (K::kKv8) p.k_scale = p.v_scale = ckv_scale;
  if constexpr (PAGED) decode_set_pages<K::kKv8>(p, pg, 1, kMlaDqk);
  const unsigned grid = (unsigned)(ge.units * ns);
  const bool wide = ge.nb == 4;
  if (dtype == FA_DTYPE_BF16)
    return wide ? mla_launch_inst<K, __bf16, true, PAGED>(p, grid, stream)
                : mla_launch_inst<K, __bf16, false, PAGED>(p, grid, stream);
  return wide ? mla_launch_inst<K, f16, true, PAGED>(p, grid, stream)
              : mla_launch_inst<K, f16, false, PAGED>(p, grid, stream);
}

}  // namespace fa

#define FA_MLA_CONTIG_PARAMS int kv_capacity
#define FA_MLA_CONTIG_ARGS kv_capacity, {}
#define FA_MLA_PAGED_PARAMS int num_pages, int page_size, const int *block_table, int max_pages_per_seq
#define FA_MLA_PAGED_ARGS 0, {num_pages, page_size, block_table, max_pages_per_seq}
// the cache type: KV16 | KV8, the latter with `ckv_scale` after the stream
#define FA_MLA_KV16_PARAMS
#define FA_MLA_KV16_ARGS
#define FA_MLA_KV16_KERNELS fa::MlaKernels16
#define FA_MLA_KV8_PARAMS , const float* ckv_scale
#define FA_MLA_KV8_ARGS , ckv_scale
#define FA_MLA_KV8_KERNELS fa::MlaKernelsKv8

// PREFIX_f16 and PREFIX_bf16 of include/fa_mi355x_mla.h (KV16) or
// include/fa_mi355x_mla_kv8.h (KV8)
#define FA_MLA_ENTRY(NAME, DTYPE, CACHE, PAGED, KV)                                                    \
  extern "C" int NAME(const void* q, const void* ckv, void* o, float* lse, int batch, int heads_q,     \
                      int seqlen_q, FA_MLA_##CACHE##_PARAMS, const int* kv_lens, int causal,           \
                      float softmax_scale, int num_splits, void* workspace,                            \
                      unsigned long long ws_bytes, void* hip_stream FA_MLA_##KV##_PARAMS) {            \
    return fa::mla_decode_entry<PAGED, FA_MLA_##KV##_KERNELS>(                                         \
        DTYPE, q, ckv, o, lse, batch, heads_q, seqlen_q, FA_MLA_##CACHE##_ARGS, kv_lens, causal,       \
        softmax_scale, num_splits, workspace, ws_bytes, hip_stream FA_MLA_##KV##_ARGS);                \
  }
#define FA_MLA_ENTRIES(PREFIX, CACHE, PAGED, KV)                 \
  FA_MLA_ENTRY(PREFIX##_f16, FA_DTYPE_F16, CACHE, PAGED, KV)     \
  FA_MLA_ENTRY(PREFIX##_bf16, FA_DTYPE_BF16, CACHE, PAGED, KV)
