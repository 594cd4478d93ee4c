// Host side of the prefill entries of include/fa_mi355x.h, shared by the four
// cache families (fa_prefill.hip: contiguous, fa_prefill_paged.hip: page pool +
// block table, fa_prefill_kv8.hip and fa_prefill_paged_kv8.hip: the same two
// over FP8 bytes): the one entry body (prefill_entry), the one launcher under
// it and the macro that stamps a unit's C entries (FA_PREFILL_ENTRIES), the
// twin of fa_decode_host.hpp.  No workspace and no plan: a
// workgroup is (batch element, query head, 128-row query block).
#pragma once

#include "fa_decode_host.hpp"
#include "fa_prefill_kernel.hpp"

namespace fa {

template <class T, int HDIM, bool PAGED, bool KV8, bool VARLEN, class P>
static int prefill_launch_inst(const P& p, unsigned grid, hipStream_t stream) {
  using KV = std::conditional_t<KV8, unsigned char, T>;
  if constexpr (VARLEN) {
    PrefillPacked<P> pp;
    static_cast<P&>(pp) = p;
    hipLaunchKernelGGL((fa_prefill_kernel<T, HDIM, PAGED, PrefillPacked<P>, KV>), dim3(grid), dim3(256), 0,
                       stream, pp);
  } else {
    hipLaunchKernelGGL((fa_prefill_kernel<T, HDIM, PAGED, P, KV>), dim3(grid), dim3(256), 0, stream, p);
  }
  return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
}

// The body of every prefill entry.  PAGED: `k` / `v` are the page pools, `pg`
// describes them and kv_capacity (passed as 0) becomes max_pages_per_seq *
// page_size; otherwise `pg` is unused.  KV8: the cache holds E4M3 bytes and
// k_scale / v_scale go to the kernel; otherwise they are unused.  The checks
// come in decode_entry's order; everything is returned before any launch.
// VARLEN (the fa_prefill_varlen_* entries): q and o are packed token-major
// [total_q][heads_q][head_dim], lse [heads_q][total_q];
// `seqlen_q` is total_q, `q_lens` is cu_seqlens (int32[batch + 1], required)
// and `batch` the number of sequences.  The grid is sized from shapes alone:
// heads_q * (total_q / 128 + batch) workgroups (fa_varlen_map.hpp).
// WIN (the fa_prefill[_varlen]_win_* and _sink_* entries): `window` is the
// sliding window W and the kernels are the Windowed<> instantiations,
// with decode_entry's rules: a negative W is refused with the negative shapes,
// W > 0 without causal right after the seqlen_q check, and W = 0 (no window)
// runs as W = capacity.  Without WIN `window` is not looked at.
// SINK (the fa_prefill[_varlen]_sink_* entries; with WIN): `sinks` goes to the
// Sinked<Windowed<>> instantiations (nullptr: no sinks); every status is the
// windowed twin's.
template <bool PAGED, bool KV8, bool VARLEN, bool WIN, bool SINK>
static int prefill_entry(int dtype, const void* q, const void* k, const void* v, void* o, float* lse,
                         int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                         int head_dim, const DecodePages& pg, const int* kv_lens, const int* q_lens,
                         int causal, int window, const float* sinks, void* hip_stream,
                         const float* k_scale, const float* v_scale) {
  static_assert(WIN || !SINK, "the sink kernels are instantiated over the windowed ones");
  using P0 = std::conditional_t<PAGED, std::conditional_t<KV8, PrefillPagedKv8Params, PrefillPagedParams>,
                                std::conditional_t<KV8, PrefillKv8Params, PrefillParams>>;
  using P = std::conditional_t<SINK, Sinked<Windowed<P0>>, std::conditional_t<WIN, Windowed<P0>, P0>>;
  if (batch < 0 || heads_q < 0 || heads_kv < 0 || kv_capacity < 0 || head_dim < 0)
    return FA_ERR_BAD_SHAPE;
  if (WIN && window < 0) return FA_ERR_BAD_SHAPE;
  if (head_dim != 128 && head_dim != 64) return FA_ERR_UNSUPPORTED_HEAD_DIM;
  if (VARLEN ? seqlen_q < 0 : seqlen_q < 1) return FA_ERR_BAD_SHAPE;
  if (WIN && window > 0 && !causal) return FA_ERR_BAD_SHAPE;
  if constexpr (PAGED) {
    if (const int st = decode_check_pages(pg, head_dim, &kv_capacity)) return st;
  }
  if (batch == 0 || heads_q == 0 || (VARLEN && seqlen_q == 0)) return FA_OK;
  if (heads_kv == 0 || heads_q % heads_kv != 0) return FA_ERR_BAD_SHAPE;
  // LSE rows and the rows of one head's Q / O (one buffer resource) are 32-bit
  if constexpr (VARLEN) {
    // LSE rows, and the byte range of one block's token-major Q / O rows
    if ((long long)heads_q * seqlen_q > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
    if ((long long)kPrefillBM * heads_q * 2 * head_dim > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  } else {
    if ((long long)batch * heads_q * seqlen_q > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
    if ((long long)seqlen_q * 2 * head_dim > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  }
  if constexpr (!PAGED) {
    // a head's cache rows are addressed through one buffer resource whose byte
    // range (cap * 2 * head_dim) is a 32-bit int (FP8: the same capacities)
    if ((long long)kv_capacity * 2 * head_dim > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  }
  // VARLEN: virtual block ids per head; the padded entries: query blocks per head and element
  const long long nqb = VARLEN ? (long long)seqlen_q / kPrefillBM + batch
                               : (seqlen_q + kPrefillBM - 1) / kPrefillBM;
  const long long nwg = (VARLEN ? 1LL : (long long)batch) * heads_q * nqb;
  if (nqb > 0x7fffffffLL || nwg > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  hipStream_t stream = (hipStream_t)hip_stream;
  if (kv_capacity == 0) {
    const size_t nrow = (VARLEN ? (size_t)1 : (size_t)batch) * heads_q * seqlen_q;
    return decode_empty_cache<SINK, VARLEN>(o, lse, sinks, nrow, heads_q, seqlen_q, head_dim, stream);
  }
  if (!q || !k || !v || !o || (PAGED && !pg.block_table) || (VARLEN && !q_lens))
    return FA_ERR_NULL_POINTER;
  P p = {};
  p.q = q;
  p.k = k;
  p.v = v;
  p.o = o;
  p.lse = lse;
  p.kv_lens = kv_lens;
  p.q_lens = q_lens;
  p.hq = heads_q;
  p.hkv = heads_kv;
  p.sq = seqlen_q;
  p.cap = kv_capacity;
  p.group = heads_q / heads_kv;
  p.nqb = VARLEN ? batch : (int)nqb;  // VARLEN: the kernel takes the sequence count here
  p.bhk = (unsigned)batch * (unsigned)heads_kv;
  p.causal = causal ? 1 : 0;
  p.c = 1.4426950408889634f / sqrtf((float)head_dim);
  decode_set_variant<KV8, WIN, SINK>(p, kv_capacity, window, sinks, k_scale, v_scale);
  if constexpr (PAGED) decode_set_pages<KV8>(p, pg, heads_kv, head_dim);
  const unsigned grid = (unsigned)nwg;
  return dispatch_elem_dim(dtype, head_dim, [&](auto e) {
    using E = decltype(e);
    return prefill_launch_inst<typename E::type, E::hdim, PAGED, KV8, VARLEN>(p, grid, stream);
  });
}

}  // namespace fa

// PREFIX_f16 and PREFIX_bf16 of include/fa_mi355x.h from the argument groups of
// fa_decode_host.hpp, e.g. FA_PREFILL_ENTRIES(fa_prefill_varlen_sink_paged,
// true, PAGED, SINK, KV16).  VARLEN: the fa_prefill_varlen_* entries, which
// name `seqlen_q` / `q_lens` total_q / cu_seqlens_q there (the C names differ,
// the lists do not).
#define FA_PREFILL_ENTRY(NAME, DTYPE, VARLEN, CACHE, VARIANT, SCALES)                               \
  extern "C" int NAME(const void* q, const void* k, const void* v, void* o, float* lse, int batch,  \
                      int heads_q, int heads_kv, int seqlen_q, FA_##CACHE##_PARAMS,                 \
                      const int* kv_lens, const int* q_lens,                                        \
                      int causal FA_##VARIANT##_WINDOW FA_##VARIANT##_SINKS,                        \
                      void* hip_stream FA_##SCALES##_PARAMS) {                                      \
    return fa::prefill_entry<FA_##CACHE##_FLAG, FA_##SCALES##_FLAG, VARLEN, FA_##VARIANT##_FLAGS>(  \
        DTYPE, q, k, v, o, lse, batch, heads_q, heads_kv, seqlen_q, FA_##CACHE##_ARGS, kv_lens,     \
        q_lens, causal, FA_##VARIANT##_ARGS, hip_stream, FA_##SCALES##_ARGS);                       \
  }
#define FA_PREFILL_ENTRIES(PREFIX, VARLEN, CACHE, VARIANT, SCALES)                  \
  FA_PREFILL_ENTRY(PREFIX##_f16, FA_DTYPE_F16, VARLEN, CACHE, VARIANT, SCALES)      \
  FA_PREFILL_ENTRY(PREFIX##_bf16, FA_DTYPE_BF16, VARLEN, CACHE, VARIANT, SCALES)
