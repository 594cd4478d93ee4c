// fa_rope_append_varlen.hip -- the packed (cu_seqlens, token-major) fused RoPE +
// cache-append entries of include/fa_mi355x.h over the four cache forms: the
// host body of fa_rope_append.hip (csrc/fa_rope_append_host.hpp) with VARLEN =
// true (seqlen_new is total_new, new_lens is cu_seqlens), launching the packed
// twin of csrc/fa_rope_append_kernel.hpp.
#include "fa_rope_append_host.hpp"

using namespace fa;

FA_ROPE_APPEND_ENTRIES(fa_rope_append_varlen, true, f16, FA_DTYPE_F16)
FA_ROPE_APPEND_ENTRIES(fa_rope_append_varlen, true, bf16, FA_DTYPE_BF16)
