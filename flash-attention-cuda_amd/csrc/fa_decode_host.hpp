// Host side of the decode entries of include/fa_mi355x.h, shared by the four
// cache families (fa_decode.hip: contiguous, fa_decode_paged.hip: page pool +
// block table, fa_decode_kv8.hip and fa_decode_paged_kv8.hip: the same two over
// FP8 bytes): geometry, split plan and workspace layout, so that all cut a
// problem the same way and one per-stream workspace serves any of them, then
// the one entry body (decode_entry) and the one launcher under it, the pieces
// the other families' entry bodies share with it, and the macro that stamps a
// unit's C entries from named argument groups (FA_DECODE_ENTRIES).
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <type_traits>

#include "fa_decode_kernel.hpp"
#include "fa_mi355x.h"

namespace fa {

// CUs of the current device (cached per device id; 256 if the query fails)
inline int decode_num_cus() {
  static std::atomic<int> cache[64];  // 0: not asked yet (entries may run on several host threads)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int n = cache[dev].load(std::memory_order_relaxed);
  if (!n) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    cache[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

// Workspace layout, shared with the causal split tier (fa_fwd.hip): arrival
// counters in the FIXED first 64 KB, then the per-row log2-sum-exp, then the
// fp32 partial O slabs.
constexpr unsigned long long kDecodeCtrBytes = 65536;
// most pieces a cache is cut into: the last arriver reads every piece's slab
// (64 pieces x 16 rows x 512 B = 512 KB for one 16-row unit)
constexpr int kDecodeMaxSplits = 64;
// the plan fills the CUs kDecodeFill times over (decode section)
constexpr int kDecodeFill = 1;

struct DecodeGeom {
  bool ok = false;
  int group = 0, rows = 0, nb = 0, rw = 0, rgroups = 0;
  long long units = 0;  // (batch, kv head, row group)
};

inline DecodeGeom decode_geom(int batch, int heads_q, int heads_kv, int seqlen_q) {
  DecodeGeom ge;
  if (batch <= 0 || heads_q <= 0 || heads_kv <= 0 || seqlen_q < 1 || seqlen_q > 16 ||
      heads_q % heads_kv != 0)
    return ge;
  ge.group = heads_q / heads_kv;
  ge.rows = ge.group * seqlen_q;
  ge.nb = ge.rows <= 16 ? 1 : (ge.rows <= 32 ? 2 : 4);
  ge.rw = 16 * ge.nb;
  ge.rgroups = (ge.rows + ge.rw - 1) / ge.rw;
  ge.units = (long long)batch * heads_kv * ge.rgroups;
  ge.ok = true;
  return ge;
}

// 1 when the units already fill the CUs; otherwise enough pieces to fill them
// kDecodeFill times, pieces no shorter than one round of the four waves (256
// keys), at most kDecodeMaxSplits
inline int decode_plan(const DecodeGeom& ge, int kv_capacity) {
  if (!ge.ok || kv_capacity <= 0) return 1;
  const long long cus = decode_num_cus();
  if (ge.units >= cus) return 1;
  const long long want = (cus * kDecodeFill + ge.units - 1) / ge.units;
  const long long longest = std::max(1, kv_capacity / 256);
  return (int)std::min(std::min(want, longest), (long long)kDecodeMaxSplits);
}

inline unsigned long long decode_lse_bytes(const DecodeGeom& ge, int ns) {
  const unsigned long long n = (unsigned long long)ge.units * ns * ge.rw * 4;
  return (n + 255) / 256 * 256;
}
inline unsigned long long decode_ws_total(const DecodeGeom& ge, int head_dim, int ns) {
  if (ns <= 1) return 0;
  return kDecodeCtrBytes + decode_lse_bytes(ge, ns) +
         (unsigned long long)ge.units * ns * ge.rw * head_dim * 4;
}

// rows but no keys: O = 0, LSE = -inf (memsets on the stream, no kernel)
inline bool decode_fill_empty(void* o, float* lse, size_t nrow, int head_dim, hipStream_t stream) {
  if (hipMemsetAsync(o, 0, nrow * head_dim * 2, stream) != hipSuccess) return false;
  return !lse || hipMemsetD32Async((hipDeviceptr_t)lse, (int)0xff800000u, nrow, stream) == hipSuccess;
}

// the same with sinks: O = 0, LSE = the row's head's sink (read on the device:
// one small kernel).  PACKED: the packed prefill's [Hq][T] LSE.
template <bool PACKED>
inline bool decode_fill_empty_sink(void* o, float* lse, const float* sinks, size_t nrow, int heads_q,
                                   int seqlen_q, int head_dim, hipStream_t stream) {
  if (!sinks || !lse) return decode_fill_empty(o, lse, nrow, head_dim, stream);
  if (hipMemsetAsync(o, 0, nrow * head_dim * 2, stream) != hipSuccess) return false;
  hipLaunchKernelGGL((fa_sink_fill_lse_kernel<PACKED>), dim3((unsigned)((nrow + 255) / 256)), dim3(256), 0,
                     stream, lse, sinks, nrow, heads_q, seqlen_q);
  return hipGetLastError() == hipSuccess;
}

// the workspace's three regions for a launch of ns > 1 pieces
template <class Params>
inline void decode_set_workspace(Params& p, const DecodeGeom& ge, int ns, void* ws) {
  char* w = static_cast<char*>(ws);
  p.ws_ctr = reinterpret_cast<unsigned*>(w);
  p.ws_lse = reinterpret_cast<float*>(w + kDecodeCtrBytes);
  p.ws_o = reinterpret_cast<float*>(w + kDecodeCtrBytes + decode_lse_bytes(ge, ns));
}

// One kernel instantiation: the once-per-device dynamic-LDS attribute (the
// flag tables are this instantiation's own), then the launch.
template <class T, int HDIM, int NB, bool PAGED, class P, class KV>
static int decode_launch_inst(const P& p, unsigned grid, hipStream_t stream) {
  constexpr int kLds = decode_lds_bytes<HDIM, NB>();
  constexpr auto kernel = fa_decode_kernel<T, HDIM, NB, PAGED, P, KV>;
  static std::once_flag flags[64];
  static hipError_t errs[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return FA_ERR_HIP;
  std::call_once(flags[dev], [dev] {
    errs[dev] = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    kLds);
  });
  if (errs[dev] != hipSuccess) return FA_ERR_HIP;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), kLds, stream, p);
  return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
}

template <class T, int HDIM, bool PAGED, bool KV8, class P>
static int decode_launch_nb(int nb, const P& p, unsigned grid, hipStream_t stream) {
  using KV = std::conditional_t<KV8, unsigned char, T>;
  switch (nb) {
    case 1: return decode_launch_inst<T, HDIM, 1, PAGED, P, KV>(p, grid, stream);
    case 2: return decode_launch_inst<T, HDIM, 2, PAGED, P, KV>(p, grid, stream);
    default: return decode_launch_inst<T, HDIM, 4, PAGED, P, KV>(p, grid, stream);
  }
}

// The capacity a windowed decode plans its split from: the tiles a call can
// touch are those holding [len - Sq + 1 - W, len), at most ceil((W + Sq - 1) /
// 64) + 1 of them.  Callers size the workspace with fa_decode_ws_bytes at this
// capacity (window <= 0: the capacity itself).
inline int decode_window_capacity(int kv_capacity, int seqlen_q, int window) {
  if (window <= 0) return kv_capacity;
  const long long eff = 64 * (((long long)window + seqlen_q - 1 + 63) / 64) + 64;
  return (int)std::min<long long>(kv_capacity, eff);
}

// what the paged entries take in place of kv_capacity
struct DecodePages {
  int num_pages, page_size;
  const int* block_table;
  int max_pages_per_seq;
};

// The page-geometry checks of every paged entry (decode, prefill, append and
// RoPE append alike); on FA_OK *kv_capacity is the logical capacity.
inline int decode_check_pages(const DecodePages& pg, int head_dim, int* kv_capacity) {
  // a 64-key tile must not straddle two pages
  if (pg.page_size <= 0 || pg.page_size % 64 != 0) return FA_ERR_BAD_SHAPE;
  if (pg.num_pages <= 0 || pg.max_pages_per_seq < 0) return FA_ERR_BAD_SHAPE;
  // a head's rows of one page are addressed through one buffer resource whose
  // byte range (page_size * 2 * head_dim) is a 32-bit int.  The FP8 entries
  // keep the 16-bit bound (their range is half that): both accept the same
  // page sizes
  if ((long long)pg.page_size * 2 * head_dim > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  // key indices (up to the end of the last tile) are 32-bit ints in the kernel
  if ((long long)pg.max_pages_per_seq * pg.page_size > 0x7fffffffLL - 64) return FA_ERR_BAD_SHAPE;
  *kv_capacity = pg.max_pages_per_seq * pg.page_size;
  return FA_OK;
}

// the paged fields the decode and prefill kernels share (decode adds its own)
template <bool KV8, class Params>
inline void decode_set_pages(Params& p, const DecodePages& pg, int heads_kv, int head_dim) {
  p.table = pg.block_table;
  p.max_pages = pg.max_pages_per_seq;
  p.num_pages = pg.num_pages;
  p.tpp = pg.page_size / 64;
  using CacheElem = std::conditional_t<KV8, unsigned char, f16>;  // f16 and bf16: one size
  p.head_bytes = (unsigned long long)pg.page_size * sizeof(CacheElem) * head_dim;
  p.page_bytes = p.head_bytes * heads_kv;
}

// the fields a variant adds: the window (W = 0, no window, runs as W =
// capacity, which masks nothing), the sinks, the FP8 scales and (decode only)
// the tree mask
template <bool KV8, bool WIN, bool SINK, class Params>
inline void decode_set_variant(Params& p, [[maybe_unused]] int kv_capacity, [[maybe_unused]] int window,
                               [[maybe_unused]] const float* sinks,
                               [[maybe_unused]] const float* k_scale,
                               [[maybe_unused]] const float* v_scale,
                               [[maybe_unused]] const int* tree_mask = nullptr) {
  if constexpr (WIN) p.window = window > 0 ? std::min(window, kv_capacity) : kv_capacity;
  if constexpr (SINK) p.sinks = sinks;
  if constexpr (ParamsTreed<Params>::value) p.tree = tree_mask;
  if constexpr (KV8) {
    p.k_scale = k_scale;
    p.v_scale = v_scale;
  }
}

// rows but no keys, as a status: O = 0, LSE = -inf (SINK: the row's head's
// sink); nothing else runs.  PACKED: as for decode_fill_empty_sink.
template <bool SINK, bool PACKED>
static int decode_empty_cache(void* o, float* lse, [[maybe_unused]] const float* sinks, size_t nrow,
                              [[maybe_unused]] int heads_q, [[maybe_unused]] int seqlen_q, int head_dim,
                              hipStream_t stream) {
  if (!o) return FA_ERR_NULL_POINTER;
  bool ok;
  if constexpr (SINK)
    ok = decode_fill_empty_sink<PACKED>(o, lse, sinks, nrow, heads_q, seqlen_q, head_dim, stream);
  else
    ok = decode_fill_empty(o, lse, nrow, head_dim, stream);
  return ok ? FA_OK : FA_ERR_HIP;
}

// The element type and head_dim of a launch as a type: launch(ElemDim<T, HDIM>{})
// for the one of the four that (dtype, head_dim) names (head_dim is 128 or 64).
template <class T, int HDIM>
struct ElemDim {
  using type = T;
  static constexpr int hdim = HDIM;
};
template <class Launch>
inline int dispatch_elem_dim(int dtype, int head_dim, Launch&& launch) {
  if (dtype == FA_DTYPE_BF16)
    return head_dim == 128 ? launch(ElemDim<__bf16, 128>{}) : launch(ElemDim<__bf16, 64>{});
  return head_dim == 128 ? launch(ElemDim<f16, 128>{}) : launch(ElemDim<f16, 64>{});
}

// The body of every decode entry.  PAGED: `k` / `v` are the page pools, `pg`
// describes them and kv_capacity (passed as 0) becomes max_pages_per_seq *
// page_size; otherwise `pg` is unused.  KV8: the cache holds E4M3 bytes and
// k_scale / v_scale go to the kernel; otherwise they are unused.  The twelve
// kernels a <PAGED, KV8> pair can launch are instantiated from here.
// WIN (the fa_decode_win_* and fa_decode_sink_* entries): `window` is the
// sliding window W and the kernels are the Windowed<> instantiations; a
// negative W is refused with the negative shapes, W > 0 without causal right
// after the seqlen_q check, W = 0 (no window) runs as W = capacity, which
// masks nothing, and num_splits = 0 plans from decode_window_capacity().
// Without WIN `window` is not looked at (the entries pass 0).
// SINK (the fa_decode_sink_* entries; with WIN): `sinks`
// goes to the Sinked<Windowed<>> instantiations (nullptr: no sinks); the
// statuses, the plan and the workspace are the windowed twin's.
// TREE (the fa_decode_tree_* entries of include/fa_mi355x_tree.h; with SINK):
// `tree_mask` goes to the Treed<Sinked<Windowed<>>> instantiations (nullptr:
// the chain); the mask replaces the causal rule, so causal = 0 is refused, and
// so is a window shorter than the drafts (0 < W < seqlen_q), both where the
// sink twin refuses a window without causal; everything else is that twin's.
// Without TREE `tree_mask` is not looked at (the entries pass nullptr).
template <bool PAGED, bool KV8, bool WIN, bool SINK, bool TREE>
static int decode_entry(int dtype, const void* q, const void* k, const void* v, void* o, float* lse,
                        int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                        int head_dim, const DecodePages& pg, const int* kv_lens, int causal,
                        int window, const float* sinks, const int* tree_mask, int num_splits,
                        void* ws, unsigned long long ws_bytes, void* hip_stream, const float* k_scale,
                        const float* v_scale) {
  static_assert(WIN || !SINK, "the sink kernels are instantiated over the windowed ones");
  using P0 = std::conditional_t<PAGED, std::conditional_t<KV8, DecodePagedKv8Params, DecodePagedParams>,
                                std::conditional_t<KV8, DecodeKv8Params, DecodeParams>>;
  static_assert(SINK || !TREE, "the tree kernels are instantiated over the sink ones");
  using P = std::conditional_t<
      TREE, Treed<Sinked<Windowed<P0>>>,
      std::conditional_t<SINK, Sinked<Windowed<P0>>, std::conditional_t<WIN, Windowed<P0>, P0>>>;
  if (batch < 0 || heads_q < 0 || heads_kv < 0 || kv_capacity < 0 || head_dim < 0 || num_splits < 0)
    return FA_ERR_BAD_SHAPE;
  if (WIN && window < 0) return FA_ERR_BAD_SHAPE;
  if (head_dim != 128 && head_dim != 64) return FA_ERR_UNSUPPORTED_HEAD_DIM;
  if (seqlen_q < 1 || seqlen_q > 16) return FA_ERR_BAD_SHAPE;
  if (WIN && window > 0 && !causal) return FA_ERR_BAD_SHAPE;
  if (TREE && (!causal || (window > 0 && window < seqlen_q))) return FA_ERR_BAD_SHAPE;
  if constexpr (PAGED) {
    if (const int st = decode_check_pages(pg, head_dim, &kv_capacity)) return st;
  }
  if (batch == 0 || heads_q == 0) return FA_OK;
  if (heads_kv == 0 || heads_q % heads_kv != 0) return FA_ERR_BAD_SHAPE;
  if ((long long)batch * heads_q * seqlen_q > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  if constexpr (!PAGED) {
    // a head's cache rows are addressed through one buffer resource whose byte
    // range (cap * 2 * head_dim) is a 32-bit int.  The FP8 entries keep the
    // 16-bit bound (their range is half that): both accept the same capacities
    if ((long long)kv_capacity * 2 * head_dim > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
    if (!kv_lens && causal && kv_capacity < seqlen_q && kv_capacity > 0) return FA_ERR_BAD_SHAPE;
  }
  hipStream_t stream = (hipStream_t)hip_stream;
  const size_t nrow = (size_t)batch * heads_q * seqlen_q;
  if (kv_capacity == 0)
    return decode_empty_cache<SINK, false>(o, lse, sinks, nrow, heads_q, seqlen_q, head_dim, stream);
  if (!q || !k || !v || !o || (PAGED && !pg.block_table)) return FA_ERR_NULL_POINTER;
  const DecodeGeom ge = decode_geom(batch, heads_q, heads_kv, seqlen_q);
  if (num_splits > kDecodeMaxSplits) return FA_ERR_BAD_CONFIG;
  const int ns = num_splits > 0
                     ? num_splits
                     : decode_plan(ge, WIN ? decode_window_capacity(kv_capacity, seqlen_q, window)
                                           : kv_capacity);
  if (ge.units * ns > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  if (ns > 1) {
    // one arrival counter per unit in the 64-KB region (the plan splits only
    // when units are fewer than CUs; a forced split of more units is refused)
    if (ge.units > (long long)(kDecodeCtrBytes / 4)) return FA_ERR_BAD_CONFIG;
    // the slabs take 16-B sc1 stores / loads: a 16-byte aligned workspace
    if (!ws || ws_bytes < decode_ws_total(ge, head_dim, ns) || (reinterpret_cast<uintptr_t>(ws) & 15) != 0)
      return FA_ERR_WORKSPACE;
  }
  P p = {};
  p.q = q;
  p.k = k;
  p.v = v;
  p.o = o;
  p.lse = lse;
  p.kv_lens = kv_lens;
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
  decode_set_variant<KV8, WIN, SINK>(p, kv_capacity, window, sinks, k_scale, v_scale, tree_mask);
  if constexpr (PAGED) {
    decode_set_pages<KV8>(p, pg, heads_kv, head_dim);
    p.adv_pages = 4 / p.tpp;
    p.adv_tiles = 4 % p.tpp;
  }
  const unsigned grid = (unsigned)(ge.units * ns);
  return dispatch_elem_dim(dtype, head_dim, [&](auto e) {
    using E = decltype(e);
    return decode_launch_nb<typename E::type, E::hdim, PAGED, KV8>(ge.nb, p, grid, stream);
  });
}

}  // namespace fa

// The argument groups an entry's C list is composed of, each once as
// parameters and once as what the entry bodies take for it (FLAG / FLAGS: the
// bodies' template arguments).  An entry macro picks one of each kind by tag:
//   cache:   CONTIG | PAGED       in kv_capacity's place
//   variant: PLAIN | WIN | SINK   `window` (and `sinks`) after `causal`
//            TREE (decode only)   SINK's, then `tree_mask`
//   scales:  KV16 | KV8           the FP8 scales, last
#define FA_CONTIG_PARAMS int kv_capacity, int head_dim
#define FA_CONTIG_ARGS kv_capacity, head_dim, {}
#define FA_CONTIG_FLAG false
#define FA_PAGED_PARAMS \
  int head_dim, int num_pages, int page_size, const int* block_table, int max_pages_per_seq
#define FA_PAGED_ARGS 0, head_dim, {num_pages, page_size, block_table, max_pages_per_seq}
#define FA_PAGED_FLAG true

// (the token-major attention entries take `sinks` last, hence two groups)
#define FA_PLAIN_WINDOW
#define FA_PLAIN_SINKS
#define FA_PLAIN_ARGS 0, nullptr
#define FA_PLAIN_FLAGS false, false
#define FA_WIN_WINDOW , int window
#define FA_WIN_SINKS
#define FA_WIN_ARGS window, nullptr
#define FA_WIN_FLAGS true, false
#define FA_SINK_WINDOW , int window
#define FA_SINK_SINKS , const float* sinks
#define FA_SINK_ARGS window, sinks
#define FA_SINK_FLAGS true, true
// (the decode entries alone take a tree mask, hence a group of its own: MASK)
#define FA_PLAIN_MASK
#define FA_PLAIN_MASK_ARG nullptr
#define FA_PLAIN_MASK_FLAG false
#define FA_WIN_MASK
#define FA_WIN_MASK_ARG nullptr
#define FA_WIN_MASK_FLAG false
#define FA_SINK_MASK
#define FA_SINK_MASK_ARG nullptr
#define FA_SINK_MASK_FLAG false
#define FA_TREE_WINDOW , int window
#define FA_TREE_SINKS , const float* sinks
#define FA_TREE_ARGS window, sinks
#define FA_TREE_FLAGS true, true
#define FA_TREE_MASK , const int* tree_mask
#define FA_TREE_MASK_ARG tree_mask
#define FA_TREE_MASK_FLAG true

#define FA_KV16_PARAMS
#define FA_KV16_ARGS nullptr, nullptr
#define FA_KV16_FLAG false
#define FA_KV8_PARAMS , const float* k_scale, const float* v_scale
#define FA_KV8_ARGS k_scale, v_scale
#define FA_KV8_FLAG true

// PREFIX_f16 and PREFIX_bf16 of include/fa_mi355x.h (TREE: of
// include/fa_mi355x_tree.h), e.g.
// FA_DECODE_ENTRIES(fa_decode_win_paged_kv8, PAGED, WIN, KV8); the paged lists
// name `k` / `v` k_pages / v_pages there.
#define FA_DECODE_ENTRY(NAME, DTYPE, CACHE, VARIANT, SCALES)                                        \
  extern "C" int NAME(const void* q, const void* k, const void* v, void* o, float* lse, int batch,  \
                      int heads_q, int heads_kv, int seqlen_q, FA_##CACHE##_PARAMS,                 \
                      const int* kv_lens, int causal FA_##VARIANT##_WINDOW FA_##VARIANT##_SINKS     \
                          FA_##VARIANT##_MASK,                                                      \
                      int num_splits, void* workspace, unsigned long long ws_bytes,                 \
                      void* hip_stream FA_##SCALES##_PARAMS) {                                      \
    return fa::decode_entry<FA_##CACHE##_FLAG, FA_##SCALES##_FLAG, FA_##VARIANT##_FLAGS,            \
                            FA_##VARIANT##_MASK_FLAG>(                                              \
        DTYPE, q, k, v, o, lse, batch, heads_q, heads_kv, seqlen_q, FA_##CACHE##_ARGS, kv_lens,     \
        causal, FA_##VARIANT##_ARGS, FA_##VARIANT##_MASK_ARG, num_splits, workspace, ws_bytes,      \
        hip_stream, FA_##SCALES##_ARGS);                                                            \
  }
#define FA_DECODE_ENTRIES(PREFIX, CACHE, VARIANT, SCALES)                 \
  FA_DECODE_ENTRY(PREFIX##_f16, FA_DTYPE_F16, CACHE, VARIANT, SCALES)     \
  FA_DECODE_ENTRY(PREFIX##_bf16, FA_DTYPE_BF16, CACHE, VARIANT, SCALES)
