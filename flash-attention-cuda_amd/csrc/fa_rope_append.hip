// fa_rope_append.hip -- the fused RoPE + cache-append entries of
// include/fa_mi355x.h over the four cache forms (contiguous / paged, 16-bit /
// FP8 E4M3), new tokens as padded [B][H][Sn][D] with new_lens: Q and K rotated,
// K and V appended, one launch.  The host body (rope_append_entry) is
// csrc/fa_rope_append_host.hpp, the kernel csrc/fa_rope_append_kernel.hpp
// (DESIGN.md §3.0o).
#include "fa_rope_append_host.hpp"

using namespace fa;

FA_ROPE_APPEND_ENTRIES(fa_rope_append, false, f16, FA_DTYPE_F16)
FA_ROPE_APPEND_ENTRIES(fa_rope_append, false, bf16, FA_DTYPE_BF16)
