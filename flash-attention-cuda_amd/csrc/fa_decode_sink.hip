// fa_decode_sink.hip -- decode attention over a contiguous 16-bit K/V cache
// with a sliding window and attention sinks: fa_decode_sink_f16 / _bf16 of
// include/fa_mi355x.h, stamped by FA_DECODE_ENTRIES next to the host body in
// csrc/fa_decode_host.hpp; the kernel is csrc/fa_decode_kernel.hpp (DESIGN.md
// §3.0n).  A unit of its own so that the build stays parallel.
#include "fa_decode_host.hpp"

FA_DECODE_ENTRIES(fa_decode_sink, CONTIG, SINK, KV16)
