// Host side of the fused RoPE + cache-append entries of include/fa_mi355x.h,
// shared by fa_rope_append.hip (padded [B][H][Sn][D] with new_lens) and
// fa_rope_append_varlen.hip (packed [T][H][D] with cu_seqlens): one entry body
// (rope_append_entry) that checks the arguments before any HIP call -- the
// append's checks in append_entry's order (csrc/fa_cache_append_host.hpp), the
// rotary ones between them -- and launches csrc/fa_rope_append_kernel.hpp
// (DESIGN.md §3.0o).
#pragma once

#include <algorithm>
#include <cstdint>

#include "fa_cache_append_host.hpp"
#include "fa_rope_append_kernel.hpp"

namespace fa {

// workgroups (at four head slots each) from which a launch gives each workgroup
// four head slots: four per CU of the 256
constexpr long long kRopeWideWorkgroups = 1024;

struct RopeArgs {
  const void* q;
  void* q_out;
  int heads_q;
  const float* cos;
  const float* sin;
  int rope_len, rotary_dim, interleaved;
};

template <class T, bool PAGED, bool KV8, bool VARLEN>
static int rope_append_launch(int head_dim, const RopeAppendParams& p, dim3 grid, hipStream_t stream) {
  using S = std::conditional_t<VARLEN, PackedSrc<T>, T>;
  if (head_dim == 128)
    hipLaunchKernelGGL((fa_rope_append_kernel<S, 128, PAGED, KV8>), grid, dim3(256), 0, stream, p);
  else
    hipLaunchKernelGGL((fa_rope_append_kernel<S, 64, PAGED, KV8>), grid, dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
}

// The body of all sixteen entries; PAGED, KV8, VARLEN and the append's
// arguments as for append_entry.  `dtype` is always the 16-bit type of k_new,
// v_new and q.  A capacity of 0 (or heads_kv of 0) leaves no K/V row to write:
// the query heads are still rotated, and the K/V pointers are not looked at.
template <bool PAGED, bool KV8, bool VARLEN = false>
static int rope_append_entry(int dtype, const RopeArgs& ra, const void* k_new, const void* v_new,
                             void* k_cache, void* v_cache, int batch, int heads_kv, int seqlen_new,
                             int kv_capacity, int head_dim, const DecodePages& pg, const int* kv_lens,
                             const int* new_lens, void* hip_stream, const float* k_scale,
                             const float* v_scale) {
  if (batch < 0 || heads_kv < 0 || kv_capacity < 0 || head_dim < 0 || ra.heads_q < 0)
    return FA_ERR_BAD_SHAPE;
  if (head_dim != 128 && head_dim != 64) return FA_ERR_UNSUPPORTED_HEAD_DIM;
  // token indices (up to the end of a wave's last row) are 32-bit ints in the kernel
  if (seqlen_new < (VARLEN ? 0 : 1) || seqlen_new > 0x7fffffff - 64) return FA_ERR_BAD_SHAPE;
  if (ra.rotary_dim < 16 || ra.rotary_dim > head_dim || ra.rotary_dim % 16 != 0) return FA_ERR_BAD_SHAPE;
  if (ra.rope_len < 1) return FA_ERR_BAD_SHAPE;
  if constexpr (PAGED) {
    if (const int st = decode_check_pages(pg, head_dim, &kv_capacity)) return st;
  }
  if (batch == 0 || (heads_kv == 0 && ra.heads_q == 0) || (VARLEN && seqlen_new == 0)) return FA_OK;
  if constexpr (!PAGED) {
    if ((long long)kv_capacity * 2 * head_dim > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  }
  const int tb = head_dim == 128 ? append_block_tokens<128>() : append_block_tokens<64>();
  // VARLEN: the virtual block ids are the grid's x, a 32-bit int in the kernel
  if (VARLEN && (long long)seqlen_new / tb + batch > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  // the head slots are a 32-bit int in the kernel
  if ((long long)heads_kv + ra.heads_q > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  const int kvs = kv_capacity == 0 ? 0 : heads_kv;  // K/V head slots: none when no row exists
  if (kvs == 0 && ra.heads_q == 0) return FA_OK;    // nothing to write
  if ((kvs > 0 && (!k_new || !v_new || !k_cache || !v_cache || (PAGED && !pg.block_table))) ||
      !kv_lens || (VARLEN && !new_lens))
    return FA_ERR_NULL_POINTER;
  if (!ra.cos || !ra.sin) return FA_ERR_NULL_POINTER;
  if (ra.heads_q > 0 && (!ra.q || !ra.q_out)) return FA_ERR_NULL_POINTER;
  // the kernel reads the tables in 16-byte pieces
  if (((uintptr_t)ra.cos | (uintptr_t)ra.sin) & 15) return FA_ERR_BAD_SHAPE;
  RopeAppendParams rp = {};
  AppendParams& p = rp.a;
  p.k_new = k_new;
  p.v_new = v_new;
  p.k_cache = k_cache;
  p.v_cache = v_cache;
  p.kv_lens = kv_lens;
  p.new_lens = new_lens;
  p.batch = batch;
  p.hkv = heads_kv;
  p.sn = seqlen_new;
  p.cap = kv_capacity;
  if constexpr (PAGED) {
    p.table = pg.block_table;
    p.max_pages = pg.max_pages_per_seq;
    p.num_pages = pg.num_pages;
    p.page_size = pg.page_size;
    p.head_bytes = (unsigned long long)pg.page_size * (KV8 ? 1 : 2) * head_dim;
    p.page_bytes = p.head_bytes * heads_kv;
  }
  if constexpr (KV8) {
    p.k_scale = k_scale;
    p.v_scale = v_scale;
  }
  rp.q = ra.q;
  rp.q_out = ra.q_out;
  rp.cos = ra.cos;
  rp.sin = ra.sin;
  rp.hq = ra.heads_q;
  rp.kvs = kvs;
  rp.rope_len = ra.rope_len;
  rp.rdim = ra.rotary_dim;
  rp.interleaved = ra.interleaved != 0;
  // head slots and batch past the grid limit are strided over inside the kernel.
  // A workgroup keeps its tokens' cos / sin rows in registers over its head
  // slots, so a launch with workgroups to spare (a prefill) gives each four
  // slots: a quarter of the table loads.  A small launch (a decode step) keeps
  // one slot per workgroup: it is latency-bound and wants the parallelism.
  const long long gx = VARLEN ? (long long)seqlen_new / tb + batch : ((long long)seqlen_new + tb - 1) / tb;
  const int slots = kvs + ra.heads_q;
  const int gy4 = (slots + 3) / 4;
  const bool wide = gx * (VARLEN ? 1 : std::min(batch, 65535)) * gy4 >= kRopeWideWorkgroups;
  const dim3 grid((unsigned)gx, (unsigned)std::min(wide ? gy4 : slots, 65535),
                  VARLEN ? 1u : (unsigned)std::min(batch, 65535));
  hipStream_t stream = (hipStream_t)hip_stream;
  if (dtype == FA_DTYPE_BF16)
    return rope_append_launch<__bf16, PAGED, KV8, VARLEN>(head_dim, rp, grid, stream);
  return rope_append_launch<f16, PAGED, KV8, VARLEN>(head_dim, rp, grid, stream);
}

// The sixteen entries' argument lists: NAME(append's arguments..., then)
//   const void* q, void* q_out, int heads_q, const float* cos, const float* sin,
//   int rope_len, int rotary_dim, int interleaved
// after hip_stream (16-bit caches) or after v_scale (FP8 caches).
#define FA_ROPE_TAIL                                                                            \
  const void *q, void *q_out, int heads_q, const float *cos, const float *sin, int rope_len,   \
      int rotary_dim, int interleaved
#define FA_ROPE_ARGS RopeArgs{q, q_out, heads_q, cos, sin, rope_len, rotary_dim, interleaved}

// VARLEN: instantiated by the two units with `total_new` / `cu_seqlens` in
// seqlen_new's / new_lens' place (the C names differ, the lists do not).
#define FA_ROPE_APPEND_ENTRIES(PREFIX, VARLEN, SUFFIX, DTYPE)                                        \
  extern "C" int PREFIX##_##SUFFIX(const void* k_new, const void* v_new, void* k_cache,             \
                                   void* v_cache, int batch, int heads_kv, int seqlen_new,          \
                                   int kv_capacity, int head_dim, const int* kv_lens,               \
                                   const int* new_lens, void* hip_stream, FA_ROPE_TAIL) {           \
    return rope_append_entry<false, false, VARLEN>(DTYPE, FA_ROPE_ARGS, k_new, v_new, k_cache,      \
                                                   v_cache, batch, heads_kv, seqlen_new,            \
                                                   kv_capacity, head_dim, {}, kv_lens, new_lens,    \
                                                   hip_stream, nullptr, nullptr);                   \
  }                                                                                                  \
  extern "C" int PREFIX##_paged_##SUFFIX(                                                            \
      const void* k_new, const void* v_new, void* k_pages, void* v_pages, int batch, int heads_kv,   \
      int seqlen_new, int head_dim, int num_pages, int page_size, const int* block_table,            \
      int max_pages_per_seq, const int* kv_lens, const int* new_lens, void* hip_stream,              \
      FA_ROPE_TAIL) {                                                                                \
    return rope_append_entry<true, false, VARLEN>(                                                   \
        DTYPE, FA_ROPE_ARGS, k_new, v_new, k_pages, v_pages, batch, heads_kv, seqlen_new, 0,         \
        head_dim, {num_pages, page_size, block_table, max_pages_per_seq}, kv_lens, new_lens,         \
        hip_stream, nullptr, nullptr);                                                               \
  }                                                                                                  \
  extern "C" int PREFIX##_kv8_##SUFFIX(                                                              \
      const void* k_new, const void* v_new, void* k_cache, void* v_cache, int batch, int heads_kv,   \
      int seqlen_new, int kv_capacity, int head_dim, const int* kv_lens, const int* new_lens,        \
      void* hip_stream, const float* k_scale, const float* v_scale, FA_ROPE_TAIL) {                  \
    return rope_append_entry<false, true, VARLEN>(DTYPE, FA_ROPE_ARGS, k_new, v_new, k_cache,        \
                                                  v_cache, batch, heads_kv, seqlen_new, kv_capacity, \
                                                  head_dim, {}, kv_lens, new_lens, hip_stream,       \
                                                  k_scale, v_scale);                                 \
  }                                                                                                  \
  extern "C" int PREFIX##_paged_kv8_##SUFFIX(                                                        \
      const void* k_new, const void* v_new, void* k_pages, void* v_pages, int batch, int heads_kv,   \
      int seqlen_new, int head_dim, int num_pages, int page_size, const int* block_table,            \
      int max_pages_per_seq, const int* kv_lens, const int* new_lens, void* hip_stream,              \
      const float* k_scale, const float* v_scale, FA_ROPE_TAIL) {                                    \
    return rope_append_entry<true, true, VARLEN>(                                                    \
        DTYPE, FA_ROPE_ARGS, k_new, v_new, k_pages, v_pages, batch, heads_kv, seqlen_new, 0,         \
        head_dim, {num_pages, page_size, block_table, max_pages_per_seq}, kv_lens, new_lens,         \
        hip_stream, k_scale, v_scale);                                                               \
  }

}  // namespace fa
