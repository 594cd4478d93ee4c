// Host side of the cache-append entries of include/fa_mi355x.h, shared by
// fa_cache_append.hip (new tokens as padded [B][Hkv][Sn][D] with new_lens) and
// fa_cache_append_varlen.hip (packed [T][Hkv][D] with cu_seqlens): the one
// entry body (append_entry, in the manner of decode_entry in
// csrc/fa_decode_host.hpp) checks the arguments before any HIP call and
// launches csrc/fa_cache_append_kernel.hpp.
#pragma once

#include <algorithm>

#include "fa_cache_append_kernel.hpp"
#include "fa_decode_host.hpp"

namespace fa {

template <class T, bool PAGED, bool KV8, bool VARLEN>
static int append_launch(int head_dim, const AppendParams& p, dim3 grid, hipStream_t stream) {
  using S = std::conditional_t<VARLEN, PackedSrc<T>, T>;
  if (head_dim == 128)
    hipLaunchKernelGGL((fa_cache_append_kernel<S, 128, PAGED, KV8>), grid, dim3(256), 0, stream, p);
  else
    hipLaunchKernelGGL((fa_cache_append_kernel<S, 64, PAGED, KV8>), grid, dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
}

// The body of all twelve entries.  PAGED: the caches are the page pools, `pg`
// describes them and kv_capacity (passed as 0) becomes max_pages_per_seq *
// page_size.  KV8: the caches hold E4M3 bytes, `dtype` is the source's type
// and the scales go to the kernel; otherwise all three are unused (a 16-bit
// cache takes a bit copy).  The checks the decode entries share with these
// come in decode_entry's order, so a cache one side accepts the other does.
// VARLEN: k_new / v_new are packed [total_new][heads_kv][head_dim];
// `seqlen_new` is total_new (0: FA_OK, nothing enqueued), `new_lens` is
// cu_seqlens (int32[batch + 1], required) and `batch` the number of sequences;
// the grid's x is total_new / TB + batch virtual block ids (fa_varlen_map.hpp).
template <bool PAGED, bool KV8, bool VARLEN = false>
static int append_entry(int dtype, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                        int batch, int heads_kv, int seqlen_new, int kv_capacity, int head_dim,
                        const DecodePages& pg, const int* kv_lens, const int* new_lens,
                        void* hip_stream, const float* k_scale, const float* v_scale) {
  if (batch < 0 || heads_kv < 0 || kv_capacity < 0 || head_dim < 0) return FA_ERR_BAD_SHAPE;
  if (head_dim != 128 && head_dim != 64) return FA_ERR_UNSUPPORTED_HEAD_DIM;
  // token indices (up to the end of a wave's last row) are 32-bit ints in the kernel
  if (seqlen_new < (VARLEN ? 0 : 1) || seqlen_new > 0x7fffffff - 64) return FA_ERR_BAD_SHAPE;
  if constexpr (PAGED) {
    if (const int st = decode_check_pages(pg, head_dim, &kv_capacity)) return st;
  }
  if (batch == 0 || heads_kv == 0 || (VARLEN && seqlen_new == 0)) return FA_OK;
  if constexpr (!PAGED) {
    if ((long long)kv_capacity * 2 * head_dim > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  }
  const int tb = head_dim == 128 ? append_block_tokens<128>() : append_block_tokens<64>();
  // VARLEN: the virtual block ids are the grid's x, a 32-bit int in the kernel
  if (VARLEN && (long long)seqlen_new / tb + batch > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  if (kv_capacity == 0) return FA_OK;  // no row exists: nothing to write
  if (!k_new || !v_new || !k_cache || !v_cache || !kv_lens || (PAGED && !pg.block_table) ||
      (VARLEN && !new_lens))
    return FA_ERR_NULL_POINTER;
  AppendParams p = {};
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
  // heads and batch past the grid limit are strided over inside the kernel
  const dim3 grid(VARLEN ? (unsigned)(seqlen_new / tb + batch) : (unsigned)((seqlen_new + tb - 1) / tb),
                  (unsigned)std::min(heads_kv, 65535), VARLEN ? 1u : (unsigned)std::min(batch, 65535));
  hipStream_t stream = (hipStream_t)hip_stream;
  if constexpr (KV8) {
    if (dtype == FA_DTYPE_BF16)
      return append_launch<__bf16, PAGED, true, VARLEN>(head_dim, p, grid, stream);
    return append_launch<f16, PAGED, true, VARLEN>(head_dim, p, grid, stream);
  } else {
    return append_launch<unsigned short, PAGED, false, VARLEN>(head_dim, p, grid, stream);
  }
}

}  // namespace fa
