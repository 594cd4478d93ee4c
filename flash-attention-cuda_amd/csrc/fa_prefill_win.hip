// fa_prefill_win.hip -- prefill attention over a contiguous 16-bit K/V cache
// with a sliding window: fa_prefill_win_f16 / _bf16 of include/fa_mi355x.h,
// stamped by FA_PREFILL_ENTRIES next to the host body in
// csrc/fa_prefill_host.hpp; the kernel is csrc/fa_prefill_kernel.hpp
// (DESIGN.md §3.0m).  A unit of its own so that the build stays parallel.
#include "fa_prefill_host.hpp"

FA_PREFILL_ENTRIES(fa_prefill_win, false, CONTIG, WIN, KV16)
