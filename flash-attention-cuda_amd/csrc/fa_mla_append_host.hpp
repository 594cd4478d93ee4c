// Host side of the MLA cache writers of include/fa_mi355x_mla_append.h: the two
// entry bodies (the checks in the header's order, all before any HIP call), the
// parameters and the launches of csrc/fa_mla_append_kernel.hpp.  Neither kernel
// has a workspace or LDS.
#pragma once

#include <algorithm>
#include <cstdint>

#include "fa_decode_host.hpp"
#include "fa_mi355x_mla_append.h"
#include "fa_mla_append_kernel.hpp"

namespace fa {

// workgroups from which a launch gives each query workgroup four head groups
// (fa_rope_append_host.hpp's rule: a prefill has workgroups to spare and saves
// three quarters of the table loads, a decode step wants the parallelism)
constexpr long long kMlaAppendWideWorkgroups = 1024;

// what the two bodies share: the sizes, the page geometry, the sequences.  On
// FA_OK *empty says that nothing is to be done; BT: the kernel's token block.
template <bool PAGED>
static int mla_append_sizes(int batch, int total_new, int seqlen_new, int* kv_capacity, const DecodePages& pg,
                            const int* cu_seqlens, int row_bytes, int bt, bool* empty) {
  *empty = true;
  if (batch < 0 || *kv_capacity < 0) return FA_ERR_BAD_SHAPE;
  // token indices (up to the end of a wave's last row) are 32-bit ints in the kernel
  if (total_new < 0 || total_new > 0x7fffffff - 64) return FA_ERR_BAD_SHAPE;
  if constexpr (PAGED) {
    if (const int st = decode_check_pages(pg, 576, kv_capacity)) return st;
  }
  if (batch == 0 || total_new == 0) return FA_OK;
  if (!cu_seqlens && (seqlen_new < 0 || (long long)batch * seqlen_new != total_new)) return FA_ERR_BAD_SHAPE;
  if constexpr (!PAGED) {
    // the MLA readers' bound: an element's rows span a 32-bit byte range
    if ((long long)*kv_capacity * row_bytes > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  }
  // the virtual block ids are the grid's x, a 32-bit int in the kernel
  if ((long long)total_new / bt + batch > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  *empty = false;
  return FA_OK;
}

static bool mla_stride_ok(long long s, int width) { return s >= width && s % 8 == 0; }

struct MlaAppendQ {
  const void* q_pe;
  void* q_out;
  int heads_q;
  long long qs_t, qs_h, qo_t, qo_h;
  const float* cos;
  const float* sin;
  int rope_len, interleaved;
};

template <class T, bool PAGED, bool KV8>
static int mla_append_entry(const void* ckv_new, const void* kpe_new, void* ckv_cache, long long ckv_stride,
                            long long kpe_stride, int batch, int total_new, int seqlen_new, int kv_capacity,
                            const DecodePages& pg, const int* cu_seqlens, const int* kv_lens, const MlaAppendQ& q,
                            void* hip_stream, const float* ckv_scale) {
  if (q.heads_q < 0 || q.rope_len < 0) return FA_ERR_BAD_SHAPE;
  bool empty;
  if (const int st = mla_append_sizes<PAGED>(batch, total_new, seqlen_new, &kv_capacity, pg, cu_seqlens,
                                             KV8 ? 576 : 1152, kMlaAppendTokens, &empty))
    return st;
  if (empty) return FA_OK;
  const int kvs = kv_capacity == 0 ? 0 : 1;  // the latent slot: none when no row exists
  if (kvs == 0 && q.heads_q == 0) return FA_OK;
  // the rows are moved in 16-byte pieces: strides in multiples of 8 elements, no shorter than a row
  if (kvs && !(mla_stride_ok(ckv_stride, 512) && mla_stride_ok(kpe_stride, 64))) return FA_ERR_BAD_SHAPE;
  if (q.heads_q > 0 && !(mla_stride_ok(q.qs_t, 64) && mla_stride_ok(q.qs_h, 64) && mla_stride_ok(q.qo_t, 576) &&
                         mla_stride_ok(q.qo_h, 576)))
    return FA_ERR_BAD_SHAPE;
  if ((kvs && (!ckv_new || !kpe_new || !ckv_cache || (PAGED && !pg.block_table))) || !kv_lens)
    return FA_ERR_NULL_POINTER;
  if (!q.cos != !q.sin || (q.heads_q > 0 && (!q.cos || !q.q_pe || !q.q_out))) return FA_ERR_NULL_POINTER;
  if (q.cos && q.rope_len < 1) return FA_ERR_BAD_SHAPE;
  if (((uintptr_t)q.cos | (uintptr_t)q.sin) & 15) return FA_ERR_BAD_SHAPE;
  if (kvs && (((uintptr_t)ckv_new | (uintptr_t)kpe_new | (uintptr_t)ckv_cache) & 15)) return FA_ERR_BAD_SHAPE;
  if (q.heads_q > 0 && (((uintptr_t)q.q_pe | (uintptr_t)q.q_out) & 15)) return FA_ERR_BAD_SHAPE;
  MlaAppendParams p = {};
  p.ckv_new = ckv_new;
  p.kpe_new = kpe_new;
  p.cache = ckv_cache;
  p.ckv_stride = ckv_stride;
  p.kpe_stride = kpe_stride;
  p.q_pe = q.q_pe;
  p.q_out = q.q_out;
  p.qs_t = q.qs_t;
  p.qs_h = q.qs_h;
  p.qo_t = q.qo_t;
  p.qo_h = q.qo_h;
  p.cos = q.cos;
  p.sin = q.sin;
  p.cu = cu_seqlens;
  p.kv_lens = kv_lens;
  p.scale = KV8 ? ckv_scale : nullptr;
  p.batch = batch;
  p.total = total_new;
  p.sn = seqlen_new;
  p.cap = kv_capacity;
  if constexpr (PAGED) {
    p.table = pg.block_table;
    p.max_pages = pg.max_pages_per_seq;
    p.num_pages = pg.num_pages;
    p.page_size = pg.page_size;
  }
  p.hq = q.heads_q;
  p.kvs = kvs;
  p.rope_len = q.rope_len;
  p.interleaved = q.interleaved != 0;
  const long long gx = (long long)total_new / kMlaAppendTokens + batch;
  const int hgroups = (q.heads_q + 7) / 8, hg4 = (hgroups + 3) / 4;
  const bool wide = gx * hg4 >= kMlaAppendWideWorkgroups;
  const dim3 grid((unsigned)gx, (unsigned)(kvs + std::min(wide ? hg4 : hgroups, 65534)));
  hipLaunchKernelGGL((fa_mla_append_kernel<T, PAGED, KV8>), grid, dim3(256), 0, (hipStream_t)hip_stream, p);
  return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
}

template <class T, bool PAGED>
static int mla_indexer_append_entry(const void* k_new, void* k_pool, float* k_scale, long long k_stride, int batch,
                                    int total_new, int seqlen_new, int kv_capacity, const DecodePages& pg,
                                    const int* cu_seqlens, const int* kv_lens, int scale_pow2, void* hip_stream) {
  bool empty;
  if (const int st = mla_append_sizes<PAGED>(batch, total_new, seqlen_new, &kv_capacity, pg, cu_seqlens, 576,
                                             kMlaIdxAppendTokens, &empty))
    return st;
  if (empty || kv_capacity == 0) return FA_OK;
  if (!mla_stride_ok(k_stride, 128)) return FA_ERR_BAD_SHAPE;
  if (!k_new || !k_pool || !k_scale || !kv_lens || (PAGED && !pg.block_table)) return FA_ERR_NULL_POINTER;
  if (((uintptr_t)k_new | (uintptr_t)k_pool) & 15) return FA_ERR_BAD_SHAPE;
  MlaIdxAppendParams p = {};
  p.k_new = k_new;
  p.pool = k_pool;
  p.k_scale = k_scale;
  p.k_stride = k_stride;
  p.cu = cu_seqlens;
  p.kv_lens = kv_lens;
  p.batch = batch;
  p.total = total_new;
  p.sn = seqlen_new;
  p.cap = kv_capacity;
  if constexpr (PAGED) {
    p.table = pg.block_table;
    p.max_pages = pg.max_pages_per_seq;
    p.num_pages = pg.num_pages;
    p.page_size = pg.page_size;
  }
  p.pow2 = scale_pow2 != 0;
  const dim3 grid((unsigned)((long long)total_new / kMlaIdxAppendTokens + batch));
  hipLaunchKernelGGL((fa_mla_indexer_append_kernel<T, PAGED>), grid, dim3(256), 0, (hipStream_t)hip_stream, p);
  return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
}

}  // namespace fa

// the cache group: CONTIG | PAGED
#define FA_MLA_APP_CONTIG_PARAMS int kv_capacity
#define FA_MLA_APP_CONTIG_ARGS kv_capacity, {}
#define FA_MLA_APP_CONTIG_PAGED false
#define FA_MLA_APP_PAGED_PARAMS int num_pages, int page_size, const int *block_table, int max_pages_per_seq
#define FA_MLA_APP_PAGED_ARGS 0, {num_pages, page_size, block_table, max_pages_per_seq}
#define FA_MLA_APP_PAGED_PAGED true
// the cache type: KV16 | KV8, the latter with `ckv_scale` after the stream
#define FA_MLA_APP_KV16_PARAMS
#define FA_MLA_APP_KV16_SCALE nullptr
#define FA_MLA_APP_KV16_KV8 false
#define FA_MLA_APP_KV8_PARAMS , const float* ckv_scale
#define FA_MLA_APP_KV8_SCALE ckv_scale
#define FA_MLA_APP_KV8_KV8 true

#define FA_MLA_APPEND_ENTRY(NAME, T, CACHE, KV)                                                               \
  extern "C" int NAME(const void* ckv_new, const void* kpe_new, void* ckv_cache, long long ckv_stride,        \
                      long long kpe_stride, int batch, int total_new, int seqlen_new,                         \
                      FA_MLA_APP_##CACHE##_PARAMS, const int* cu_seqlens, const int* kv_lens,                 \
                      const void* q_pe, void* q_out, int heads_q, long long q_pe_token_stride,                \
                      long long q_pe_head_stride, long long q_out_token_stride, long long q_out_head_stride,  \
                      const float* cos, const float* sin, int rope_len, int interleaved,                      \
                      void* hip_stream FA_MLA_APP_##KV##_PARAMS) {                                            \
    return fa::mla_append_entry<T, FA_MLA_APP_##CACHE##_PAGED, FA_MLA_APP_##KV##_KV8>(                        \
        ckv_new, kpe_new, ckv_cache, ckv_stride, kpe_stride, batch, total_new, seqlen_new,                    \
        FA_MLA_APP_##CACHE##_ARGS, cu_seqlens, kv_lens,                                                       \
        fa::MlaAppendQ{q_pe, q_out, heads_q, q_pe_token_stride, q_pe_head_stride, q_out_token_stride,         \
                       q_out_head_stride, cos, sin, rope_len, interleaved},                                   \
        hip_stream, FA_MLA_APP_##KV##_SCALE);                                                                 \
  }
#define FA_MLA_APPEND_ENTRIES(PREFIX, CACHE, KV)             \
  FA_MLA_APPEND_ENTRY(PREFIX##_f16, fa::f16, CACHE, KV)      \
  FA_MLA_APPEND_ENTRY(PREFIX##_bf16, __bf16, CACHE, KV)

#define FA_MLA_INDEXER_APPEND_ENTRY(NAME, T, CACHE)                                                           \
  extern "C" int NAME(const void* k_new, void* k_pool, float* k_scale, long long k_stride, int batch,         \
                      int total_new, int seqlen_new, FA_MLA_APP_##CACHE##_PARAMS, const int* cu_seqlens,      \
                      const int* kv_lens, int scale_pow2, void* hip_stream) {                                 \
    return fa::mla_indexer_append_entry<T, FA_MLA_APP_##CACHE##_PAGED>(                                       \
        k_new, k_pool, k_scale, k_stride, batch, total_new, seqlen_new, FA_MLA_APP_##CACHE##_ARGS,            \
        cu_seqlens, kv_lens, scale_pow2, hip_stream);                                                         \
  }
