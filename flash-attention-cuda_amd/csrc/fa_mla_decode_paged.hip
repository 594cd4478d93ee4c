// fa_mla_decode_paged.hip -- MLA decode over a paged latent cache (page pool +
// block table): fa_mla_decode_paged_f16 / _bf16 of include/fa_mi355x_mla.h.
// The host body is csrc/fa_mla_decode_host.hpp, the kernel
// csrc/fa_mla_decode_kernel.hpp.  A unit of its own so that
// the build stays parallel.
#include "fa_mla_decode_host.hpp"

FA_MLA_ENTRIES(fa_mla_decode_paged, PAGED, true, KV16)
