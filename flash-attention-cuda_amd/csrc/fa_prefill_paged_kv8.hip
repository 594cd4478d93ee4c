// fa_prefill_paged_kv8.hip -- prefill attention over a paged FP8 (E4M3) K/V
// cache: fa_prefill_paged_kv8_f16 / _bf16 of include/fa_mi355x.h, stamped by
// FA_PREFILL_ENTRIES next to the host body in csrc/fa_prefill_host.hpp; the
// kernel is csrc/fa_prefill_kernel.hpp.  A unit of its own
// so that the build stays parallel.
#include "fa_prefill_host.hpp"

FA_PREFILL_ENTRIES(fa_prefill_paged_kv8, false, PAGED, PLAIN, KV8)
