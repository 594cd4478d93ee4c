// fa_mla_prefill.hip -- MLA prefill (192-dim Q/K, 128-dim V, the caller's
// softmax scale) over token-major Q, K and V: fa_mla_prefill_varlen_f16 /
// _bf16 of include/fa_mi355x_mla_prefill.h.  The host body is
// csrc/fa_mla_prefill_host.hpp, the kernel csrc/fa_mla_prefill_kernel.hpp
// (DESIGN.md §3.0v).
#include "fa_mla_prefill_host.hpp"

using namespace fa;

FA_MLA_PREFILL_ENTRIES(fa_mla_prefill_varlen)
