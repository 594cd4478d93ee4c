// fa_mla_decode_kv8.hip -- MLA decode over a contiguous FP8 (E4M3) latent
// cache: fa_mla_decode_kv8_f16 / _bf16 of include/fa_mi355x_mla_kv8.h.  The
// host body is csrc/fa_mla_decode_host.hpp, the kernel
// csrc/fa_mla_decode_kv8_kernel.hpp.
#include "fa_mla_decode_kv8_host.hpp"

FA_MLA_ENTRIES(fa_mla_decode_kv8, CONTIG, false, KV8)
