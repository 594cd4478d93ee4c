// fa_prefill_varlen.hip -- packed (cu_seqlens, token-major Q) prefill
// attention over a contiguous 16-bit K/V cache: fa_prefill_varlen_f16 / _bf16
// of include/fa_mi355x.h, stamped by FA_PREFILL_ENTRIES next to the host body
// in csrc/fa_prefill_host.hpp; the kernel is csrc/fa_prefill_kernel.hpp
// (DESIGN.md §3.0l).  A unit of its own so that the build stays parallel.
#include "fa_prefill_host.hpp"

FA_PREFILL_ENTRIES(fa_prefill_varlen, true, CONTIG, PLAIN, KV16)
