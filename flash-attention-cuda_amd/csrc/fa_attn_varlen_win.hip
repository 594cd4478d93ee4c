// fa_attn_varlen_win.hip -- attention over token-major Q, K and V with no
// cache with a sliding window: fa_attn_varlen_win_f16 / _bf16 of
// include/fa_mi355x.h, stamped by FA_ATTN_VARLEN_ENTRIES next to the host body
// in csrc/fa_attn_varlen_host.hpp; the kernel is csrc/fa_prefill_kernel.hpp
// (DESIGN.md §3.0p).  A unit of its own so that the build stays parallel.
#include "fa_attn_varlen_host.hpp"

FA_ATTN_VARLEN_ENTRIES(fa_attn_varlen_win, WIN)
