// fa_decode_tree_kv8.hip -- tree-masked decode attention (speculative-decoding
// verification) over a contiguous FP8 (E4M3) K/V cache, with a
// sliding window and attention sinks: fa_decode_tree_kv8_f16 / _bf16 of
// include/fa_mi355x_tree.h, stamped by FA_DECODE_ENTRIES next to the host body
// in csrc/fa_decode_host.hpp; the kernel is csrc/fa_decode_kernel.hpp
// (DESIGN.md §3.0s).  A unit of its own so that the build stays parallel.
#include "fa_mi355x_tree.h"

#include "fa_decode_host.hpp"

FA_DECODE_ENTRIES(fa_decode_tree_kv8, CONTIG, TREE, KV8)
