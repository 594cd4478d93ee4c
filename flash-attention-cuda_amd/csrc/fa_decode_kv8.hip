// fa_decode_kv8.hip -- host side of the decode-attention entries over an FP8
// (OCP E4M3) K/V cache of include/fa_mi355x.h (fa_decode_kv8_f16 /
// fa_decode_kv8_bf16): the checks, the split plan and the workspace of
// fa_decode.hip (csrc/fa_decode_host.hpp), one byte per cache element and one
// fp32 scale per K/V head for K and for V.  The kernel is
// csrc/fa_decode_kernel.hpp with KV = unsigned char.
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
constexpr auto fa_decode_kv8_kernel = fa_decode_kernel<T, HDIM, NB, false, DecodeKv8Params, unsigned char>;

template <class T, int HDIM, int NB>
static int kv8_launch_inst(const DecodeKv8Params& p, unsigned grid, hipStream_t stream) {
  constexpr int kLds = decode_lds_bytes<HDIM, NB>();
  static std::once_flag flags[64];
  static hipError_t errs[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return FA_ERR_HIP;
  std::call_once(flags[dev], [dev] {
    errs[dev] = hipFuncSetAttribute((const void*)fa_decode_kv8_kernel<T, HDIM, NB>,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
  });
  if (errs[dev] != hipSuccess) return FA_ERR_HIP;
  hipLaunchKernelGGL((fa_decode_kv8_kernel<T, HDIM, NB>), dim3(grid), dim3(256), kLds, stream, p);
  return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
}

template <class T, int HDIM>
static int kv8_launch_nb(int nb, const DecodeKv8Params& p, unsigned grid, hipStream_t stream) {
  switch (nb) {
    case 1: return kv8_launch_inst<T, HDIM, 1>(p, grid, stream);
    case 2: return kv8_launch_inst<T, HDIM, 2>(p, grid, stream);
    default: return kv8_launch_inst<T, HDIM, 4>(p, grid, stream);
  }
}

static int kv8_entry(int dtype, const void* q, const void* k, const void* v, void* o, float* lse,
                        int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                        int head_dim, const int* kv_lens, int causal, int num_splits, void* ws,
                        unsigned long long ws_bytes, void* hip_stream, const float* k_scale,
                        const float* v_scale) {
  if (batch < 0 || heads_q < 0 || heads_kv < 0 || kv_capacity < 0 || head_dim < 0 || num_splits < 0)
    return FA_ERR_BAD_SHAPE;
  if (head_dim != 128 && head_dim != 64) return FA_ERR_UNSUPPORTED_HEAD_DIM;
  if (seqlen_q < 1 || seqlen_q > 16) return FA_ERR_BAD_SHAPE;
  if (batch == 0 || heads_q == 0) return FA_OK;
  if (heads_kv == 0 || heads_q % heads_kv != 0) return FA_ERR_BAD_SHAPE;
  if ((long long)batch * heads_q * seqlen_q > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  // the 16-bit entries' bound (their byte range cap * 2 * head_dim is a 32-bit
  // int; here it is half that): both accept the same capacities
  if ((long long)kv_capacity * 2 * head_dim > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  if (!kv_lens && causal && kv_capacity < seqlen_q && kv_capacity > 0) return FA_ERR_BAD_SHAPE;
  hipStream_t stream = (hipStream_t)hip_stream;
  const size_t nrow = (size_t)batch * heads_q * seqlen_q;
  if (kv_capacity == 0) {
    // rows but no keys: O = 0, LSE = -inf; nothing else runs
    if (!o) return FA_ERR_NULL_POINTER;
    return decode_fill_empty(o, lse, nrow, head_dim, stream) ? FA_OK : FA_ERR_HIP;
  }
  if (!q || !k || !v || !o) return FA_ERR_NULL_POINTER;
  const DecodeGeom ge = decode_geom(batch, heads_q, heads_kv, seqlen_q);
  if (num_splits > kDecodeMaxSplits) return FA_ERR_BAD_CONFIG;
  const int ns = num_splits > 0 ? num_splits : decode_plan(ge, kv_capacity);
  if (ge.units * ns > 0x7fffffffLL) return FA_ERR_BAD_SHAPE;
  if (ns > 1) {
    // one arrival counter per unit in the 64-KB region (the plan splits only
    // when units are fewer than CUs; a forced split of more units is refused)
    if (ge.units > (long long)(kDecodeCtrBytes / 4)) return FA_ERR_BAD_CONFIG;
    // the slabs take 16-B sc1 stores / loads: a 16-byte aligned workspace
    if (!ws || ws_bytes < decode_ws_total(ge, head_dim, ns) || (reinterpret_cast<uintptr_t>(ws) & 15) != 0)
      return FA_ERR_WORKSPACE;
  }
  DecodeKv8Params p = {};
  p.q = q;
  p.k = k;
  p.v = v;
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
  const unsigned grid = (unsigned)(ge.units * ns);
  if (dtype == FA_DTYPE_BF16)
    return head_dim == 128 ? kv8_launch_nb<__bf16, 128>(ge.nb, p, grid, stream)
                           : kv8_launch_nb<__bf16, 64>(ge.nb, p, grid, stream);
  return head_dim == 128 ? kv8_launch_nb<f16, 128>(ge.nb, p, grid, stream)
                         : kv8_launch_nb<f16, 64>(ge.nb, p, grid, stream);
}

}  // namespace fa

using namespace fa;

extern "C" int fa_decode_kv8_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                                 int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                                 int head_dim, const int* kv_lens, int causal, int num_splits,
                                 void* workspace, unsigned long long ws_bytes, void* hip_stream,
                                 const float* k_scale, const float* v_scale) {
  return kv8_entry(FA_DTYPE_F16, q, k, v, o, lse, batch, heads_q, heads_kv, seqlen_q, kv_capacity,
                   head_dim, kv_lens, causal, num_splits, workspace, ws_bytes, hip_stream, k_scale,
                   v_scale);
}

extern "C" int fa_decode_kv8_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                                  int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                                  int head_dim, const int* kv_lens, int causal, int num_splits,
                                  void* workspace, unsigned long long ws_bytes, void* hip_stream,
                                  const float* k_scale, const float* v_scale) {
  return kv8_entry(FA_DTYPE_BF16, q, k, v, o, lse, batch, heads_q, heads_kv, seqlen_q, kv_capacity,
                   head_dim, kv_lens, causal, num_splits, workspace, ws_bytes, hip_stream, k_scale,
                   v_scale);
}
