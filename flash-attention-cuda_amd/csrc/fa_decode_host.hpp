// Host-side geometry, split plan and workspace layout of the decode entries,
// shared by fa_decode.hip (contiguous cache) and fa_decode_paged.hip (page
// pool + block table), so that both cut a problem the same way and one
// per-stream workspace serves either.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

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

// the workspace's three regions for a launch of ns > 1 pieces
template <class Params>
inline void decode_set_workspace(Params& p, const DecodeGeom& ge, int ns, void* ws) {
  char* w = static_cast<char*>(ws);
  p.ws_ctr = reinterpret_cast<unsigned*>(w);
  p.ws_lse = reinterpret_cast<float*>(w + kDecodeCtrBytes);
  p.ws_o = reinterpret_cast<float*>(w + kDecodeCtrBytes + decode_lse_bytes(ge, ns));
}

}  // namespace fa
