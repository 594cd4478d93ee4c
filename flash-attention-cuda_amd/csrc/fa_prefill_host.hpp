// Host side of the prefill entries of include/fa_mi355x.h, shared by the four
// cache families (fa_prefill.hip: contiguous, fa_prefill_paged.hip: page pool +
// block table, fa_prefill_kv8.hip and fa_prefill_paged_kv8.hip: the same two
// over FP8 bytes): the one entry body (prefill_entry) and the one launcher
// under it, the twin of fa_decode_host.hpp.  No workspace and no plan: a
// workgroup is (batch element, query head, 128-row query block).
#pragma once

#include "fa_decode_host.hpp"
#include "fa_prefill_kernel.hpp"

namespace fa {

template <class T, int HDIM, bool PAGED, bool KV8, class P>
static int prefill_launch_inst(const P& p, unsigned grid, hipStream_t stream) {
  using KV = std::conditional_t<KV8, unsigned char, T>;
  hipLaunchKernelGGL((fa_prefill_kernel<T, HDIM, PAGED, P, KV>), dim3(grid), dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
}

// The body of all eight entries.  PAGED: `k` / `v` are the page pools, `pg`
// describes them and kv_capacity (passed as 0) becomes max_pages_per_seq *
// page_size; otherwise `pg` is unused.  KV8: the cache holds E4M3 bytes and
// k_scale / v_scale go to the kernel; otherwise they are unused.  The checks
// come in decode_entry's order; everything is returned before any launch.
template <bool PAGED, bool KV8>
static int prefill_entry(int dtype, const void* q, const void* k, const void* v, void* o, float* lse,
                         int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                         int head_dim, const DecodePages& pg, const int* kv_lens, const int* q_lens,
                         int causal, void* hip_stream, const float* k_scale, const float* v_scale) {
  using P = std::conditional_t<PAGED, std::conditional_t<KV8, PrefillPagedKv8Params, PrefillPagedParams>,
                               std::conditional_t<KV8, PrefillKv8Params, PrefillParams>>;
  if (batch < 0 || heads_q < 0 || heads_kv < 0 || kv_capacity < 0 || head_dim < 0)
    return FA_ERR_BAD_SHAPE;
  if (head_dim != 128 && head_dim != 64) return FA_ERR_UNSUPPORTED_HEAD_DIM;
  if (seqlen_q < 1) return FA_ERR_BAD_SHAPE;
  if constexpr (PAGED) {
    // a 64-key tile must not straddle two pages
    if (pg.page_size <= 0 || pg.page_size % 64 != 0) return FA_ERR_BAD_SHAPE;
    if (pg.num_pages <= 0 || pg.max_pages_per_seq < 0) return FA_ERR_BAD_SHAPE;
    // a head's rows of one page lie in a 32-bit byte range (the FP8 entries
    // keep the 16-bit bound: both accept the same page sizes)
    if ((long long)pg.page_size * 2 * head_dim > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
    // key indices (up to the end of the last tile) are 32-bit ints in the kernel
    if ((long long)pg.max_pages_per_seq * pg.page_size > 0x7fffffffLL - 64) return FA_ERR_BAD_SHAPE;
    kv_capacity = pg.max_pages_per_seq * pg.page_size;
  }
  if (batch == 0 || heads_q == 0) return FA_OK;
  if (heads_kv == 0 || heads_q % heads_kv != 0) return FA_ERR_BAD_SHAPE;
  // LSE rows and the rows of one head's Q / O (one buffer resource) are 32-bit
  if ((long long)batch * heads_q * seqlen_q > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  if ((long long)seqlen_q * 2 * head_dim > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  if constexpr (!PAGED) {
    // a head's cache rows are addressed through one buffer resource whose byte
    // range (cap * 2 * head_dim) is a 32-bit int (FP8: the same capacities)
    if ((long long)kv_capacity * 2 * head_dim > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  }
  const int nqb = (seqlen_q + kPrefillBM - 1) / kPrefillBM;
  if ((long long)batch * heads_q * nqb > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  hipStream_t stream = (hipStream_t)hip_stream;
  if (kv_capacity == 0) {
    // rows but no keys: O = 0, LSE = -inf for every row; nothing else runs
    if (!o) return FA_ERR_NULL_POINTER;
    return decode_fill_empty(o, lse, (size_t)batch * heads_q * seqlen_q, head_dim, stream) ? FA_OK
                                                                                            : FA_ERR_HIP;
  }
  if (!q || !k || !v || !o || (PAGED && !pg.block_table)) return FA_ERR_NULL_POINTER;
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
  p.nqb = nqb;
  p.bhk = (unsigned)batch * (unsigned)heads_kv;
  p.causal = causal ? 1 : 0;
  p.c = 1.4426950408889634f / sqrtf((float)head_dim);
  if constexpr (PAGED) {
    p.table = pg.block_table;
    p.max_pages = pg.max_pages_per_seq;
    p.num_pages = pg.num_pages;
    p.tpp = pg.page_size / 64;
    using CacheElem = std::conditional_t<KV8, unsigned char, f16>;  // f16 and bf16: one size
    p.head_bytes = (unsigned long long)pg.page_size * sizeof(CacheElem) * head_dim;
    p.page_bytes = p.head_bytes * heads_kv;
  }
  if constexpr (KV8) {
    p.k_scale = k_scale;
    p.v_scale = v_scale;
  }
  const unsigned grid = (unsigned)((long long)batch * heads_q * nqb);
  if (dtype == FA_DTYPE_BF16)
    return head_dim == 128 ? prefill_launch_inst<__bf16, 128, PAGED, KV8>(p, grid, stream)
                           : prefill_launch_inst<__bf16, 64, PAGED, KV8>(p, grid, stream);
  return head_dim == 128 ? prefill_launch_inst<f16, 128, PAGED, KV8>(p, grid, stream)
                         : prefill_launch_inst<f16, 64, PAGED, KV8>(p, grid, stream);
}

}  // namespace fa
