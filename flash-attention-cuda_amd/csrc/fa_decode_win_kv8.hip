// fa_decode_win_kv8.hip -- decode attention over a contiguous FP8 (E4M3) K/V
// cache with a sliding window: fa_decode_win_kv8_f16 / _bf16 of
// include/fa_mi355x.h, stamped by FA_DECODE_ENTRIES next to the host body in
// csrc/fa_decode_host.hpp; the kernel is csrc/fa_decode_kernel.hpp (DESIGN.md
// §3.0m).  A unit of its own so that the build stays parallel.
#include "fa_decode_host.hpp"

FA_DECODE_ENTRIES(fa_decode_win_kv8, CONTIG, WIN, KV8)
