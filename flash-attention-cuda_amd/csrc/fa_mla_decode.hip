// fa_mla_decode.hip -- MLA decode over a contiguous latent cache, plus the
// split plan and the workspace size both MLA units share: fa_mla_decode_f16 /
// _bf16, fa_mla_decode_num_splits and fa_mla_decode_ws_bytes of
// include/fa_mi355x_mla.h.  The host body is csrc/fa_mla_decode_host.hpp, the
// kernel csrc/fa_mla_decode_kernel.hpp.
#include "fa_mla_decode_host.hpp"

using namespace fa;

FA_MLA_ENTRIES(fa_mla_decode, CONTIG, false, KV16)

extern "C" int fa_mla_decode_num_splits(int batch, int heads_q, int seqlen_q, int kv_capacity) {
  return mla_plan(mla_geom(batch, heads_q, seqlen_q), kv_capacity);
}

extern "C" unsigned long long fa_mla_decode_ws_bytes(int batch, int heads_q, int seqlen_q,
                                                     int num_splits) {
  const DecodeGeom ge = mla_geom(batch, heads_q, seqlen_q);
  if (!ge.ok || num_splits < 0 || num_splits > kDecodeMaxSplits) return 0;
  return decode_ws_total(ge, kMlaDv, num_splits);
}
