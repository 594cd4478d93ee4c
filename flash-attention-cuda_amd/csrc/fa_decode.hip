// fa_decode.hip -- decode attention over a contiguous 16-bit K/V cache, plus
// the split plan and the workspace size that all decode entries share:
// fa_decode_f16 / _bf16 of include/fa_mi355x.h, stamped by FA_DECODE_ENTRIES
// next to the host body in csrc/fa_decode_host.hpp; the kernel is
// csrc/fa_decode_kernel.hpp.  A unit of its own so that the
// build stays parallel.
#include "fa_decode_host.hpp"

using namespace fa;

FA_DECODE_ENTRIES(fa_decode, CONTIG, PLAIN, KV16)

extern "C" int fa_decode_num_splits(int batch, int heads_q, int heads_kv, int seqlen_q,
                                    int kv_capacity, int head_dim) {
  if (head_dim != 128 && head_dim != 64) return 1;
  return decode_plan(decode_geom(batch, heads_q, heads_kv, seqlen_q), kv_capacity);
}

extern "C" unsigned long long fa_decode_ws_bytes(int batch, int heads_q, int heads_kv, int seqlen_q,
                                                 int kv_capacity, int head_dim, int num_splits) {
  if (head_dim != 128 && head_dim != 64) return 0;
  const DecodeGeom ge = decode_geom(batch, heads_q, heads_kv, seqlen_q);
  if (!ge.ok || kv_capacity <= 0 || num_splits < 0 || num_splits > kDecodeMaxSplits) return 0;
  return decode_ws_total(ge, head_dim, num_splits > 0 ? num_splits : decode_plan(ge, kv_capacity));
}
