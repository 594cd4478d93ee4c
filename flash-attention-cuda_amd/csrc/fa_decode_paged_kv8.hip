// fa_decode_paged_kv8.hip -- host side of the paged decode-attention entries
// over an FP8 (OCP E4M3) page pool of include/fa_mi355x.h
// (fa_decode_paged_kv8_f16 / fa_decode_paged_kv8_bf16): the checks, the split
// plan and the workspace of fa_decode_paged.hip, one byte per pool element and
// one fp32 scale per K/V head for K and for V.  The kernel is
// csrc/fa_decode_kernel.hpp with PAGED = true and KV = unsigned char
// (DESIGN.md §3.0i).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include <mutex>

#include "fa_decode_host.hpp"
#include "fa_decode_kernel.hpp"
#include "fa_mi355x.h"

namespace fa {

// the twelve instantiations this file launches
template <class T, int HDIM, int NB>
constexpr auto fa_decode_paged_kv8_kernel =
    fa_decode_kernel<T, HDIM, NB, true, DecodePagedKv8Params, unsigned char>;

template <class T, int HDIM, int NB>
static int pkv8_launch_inst(const DecodePagedKv8Params& p, unsigned grid, hipStream_t stream) {
  constexpr int kLds = decode_lds_bytes<HDIM, NB>();
  static std::once_flag flags[64];
  static hipError_t errs[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return FA_ERR_HIP;
  std::call_once(flags[dev], [dev] {
    errs[dev] = hipFuncSetAttribute((const void*)fa_decode_paged_kv8_kernel<T, HDIM, NB>,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
  });
  if (errs[dev] != hipSuccess) return FA_ERR_HIP;
  hipLaunchKernelGGL((fa_decode_paged_kv8_kernel<T, HDIM, NB>), dim3(grid), dim3(256), kLds, stream, p);
  return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
}

template <class T, int HDIM>
static int pkv8_launch_nb(int nb, const DecodePagedKv8Params& p, unsigned grid, hipStream_t stream) {
  switch (nb) {
    case 1: return pkv8_launch_inst<T, HDIM, 1>(p, grid, stream);
    case 2: return pkv8_launch_inst<T, HDIM, 2>(p, grid, stream);
    default: return pkv8_launch_inst<T, HDIM, 4>(p, grid, stream);
  }
}

static int pkv8_entry(int dtype, const void* q, const void* k_pages, const void* v_pages, void* o,
                       float* lse, int batch, int heads_q, int heads_kv, int seqlen_q, int head_dim,
                       int num_pages, int page_size, const int* block_table, int max_pages_per_seq,
                       const int* kv_lens, int causal, int num_splits, void* ws,
                       unsigned long long ws_bytes, void* hip_stream, const float* k_scale,
                       const float* v_scale) {
  if (batch < 0 || heads_q < 0 || heads_kv < 0 || head_dim < 0 || num_splits < 0)
    return FA_ERR_BAD_SHAPE;
  if (head_dim != 128 && head_dim != 64) return FA_ERR_UNSUPPORTED_HEAD_DIM;
  if (seqlen_q < 1 || seqlen_q > 16) return FA_ERR_BAD_SHAPE;
  // a 64-key tile must not straddle two pages
  if (page_size <= 0 || page_size % 64 != 0) return FA_ERR_BAD_SHAPE;
  if (num_pages <= 0 || max_pages_per_seq < 0) return FA_ERR_BAD_SHAPE;
  // the 16-bit entries' bound (their byte range page_size * 2 * head_dim is a
  // 32-bit int; here it is half that): both accept the same page sizes
  if ((long long)page_size * 2 * head_dim > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  // key indices (up to the end of the last tile) are 32-bit ints in the kernel
  if ((long long)max_pages_per_seq * page_size > 0x7fffffffLL - 64) return FA_ERR_BAD_SHAPE;
  const int kv_capacity = max_pages_per_seq * page_size;
  if (batch == 0 || heads_q == 0) return FA_OK;
  if (heads_kv == 0 || heads_q % heads_kv != 0) return FA_ERR_BAD_SHAPE;
  if ((long long)batch * heads_q * seqlen_q > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  hipStream_t stream = (hipStream_t)hip_stream;
  const size_t nrow = (size_t)batch * heads_q * seqlen_q;
  if (kv_capacity == 0) {
    // rows but no keys: O = 0, LSE = -inf; nothing else runs
    if (!o) return FA_ERR_NULL_POINTER;
    return decode_fill_empty(o, lse, nrow, head_dim, stream) ? FA_OK : FA_ERR_HIP;
  }
  if (!q || !k_pages || !v_pages || !o || !block_table) return FA_ERR_NULL_POINTER;
  const DecodeGeom ge = decode_geom(batch, heads_q, heads_kv, seqlen_q);
  if (num_splits > kDecodeMaxSplits) return FA_ERR_BAD_CONFIG;
  const int ns = num_splits > 0 ? num_splits : decode_plan(ge, kv_capacity);
  if (ge.units * ns > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  if (ns > 1) {
    if (ge.units > (long long)(kDecodeCtrBytes / 4)) return FA_ERR_BAD_CONFIG;
    if (!ws || ws_bytes < decode_ws_total(ge, head_dim, ns) || (reinterpret_cast<uintptr_t>(ws) & 15) != 0)
      return FA_ERR_WORKSPACE;
  }
  DecodePagedKv8Params p = {};
  p.q = q;
  p.k = k_pages;
  p.v = v_pages;
  p.o = o;
  p.lse = lse;
  p.kv_lens = kv_lens;
  p.k_scale = k_scale;
  p.v_scale = v_scale;
  p.hq = heads_q;
  p.hkv = heads_kv;
  p.sq = seqlen_q;
  p.cap = kv_capacity;
  p.group = ge.group;
  p.rows = ge.rows;
  p.rgroups = ge.rgroups;
  p.num_splits = ns;
  p.causal = causal ? 1 : 0;
  p.c = 1.4426950408889634f / sqrtf((float)head_dim);
  if (ns > 1) decode_set_workspace(p, ge, ns, ws);
  p.table = block_table;
  p.max_pages = max_pages_per_seq;
  p.num_pages = num_pages;
  p.tpp = page_size / 64;
  p.adv_pages = 4 / p.tpp;
  p.adv_tiles = 4 % p.tpp;
  p.head_bytes = (unsigned long long)page_size * head_dim;  // one byte per element
  p.page_bytes = p.head_bytes * heads_kv;
  const unsigned grid = (unsigned)(ge.units * ns);
  if (dtype == FA_DTYPE_BF16)
    return head_dim == 128 ? pkv8_launch_nb<__bf16, 128>(ge.nb, p, grid, stream)
                           : pkv8_launch_nb<__bf16, 64>(ge.nb, p, grid, stream);
  return head_dim == 128 ? pkv8_launch_nb<f16, 128>(ge.nb, p, grid, stream)
                         : pkv8_launch_nb<f16, 64>(ge.nb, p, grid, stream);
}

}  // namespace fa

using namespace fa;

extern "C" int fa_decode_paged_kv8_f16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                       float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                                       int head_dim, int num_pages, int page_size, const int* block_table,
                                       int max_pages_per_seq, const int* kv_lens, int causal,
                                       int num_splits, void* workspace, unsigned long long ws_bytes,
                                       void* hip_stream, const float* k_scale, const float* v_scale) {
  return pkv8_entry(FA_DTYPE_F16, q, k_pages, v_pages, o, lse, batch, heads_q, heads_kv, seqlen_q,
                    head_dim, num_pages, page_size, block_table, max_pages_per_seq, kv_lens, causal,
                    num_splits, workspace, ws_bytes, hip_stream, k_scale, v_scale);
}

extern "C" int fa_decode_paged_kv8_bf16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                        float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                                        int head_dim, int num_pages, int page_size, const int* block_table,
                                        int max_pages_per_seq, const int* kv_lens, int causal,
                                        int num_splits, void* workspace, unsigned long long ws_bytes,
                                        void* hip_stream, const float* k_scale, const float* v_scale) {
  return pkv8_entry(FA_DTYPE_BF16, q, k_pages, v_pages, o, lse, batch, heads_q, heads_kv, seqlen_q,
                    head_dim, num_pages, page_size, block_table, max_pages_per_seq, kv_lens, causal,
                    num_splits, workspace, ws_bytes, hip_stream, k_scale, v_scale);
}
