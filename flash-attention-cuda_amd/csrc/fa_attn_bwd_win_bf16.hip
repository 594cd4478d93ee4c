// fa_attn_bwd_win_bf16.hip -- backward pass of the attention over token-major Q,
// K and V through the sliding window and the attention sinks, bf16:
// fa_attn_bwd_win_bf16 and fa_attn_bwd_sink_bf16 of include/fa_mi355x.h, stamped
// by FA_ATTN_BWD_ENTRY next to the host body in csrc/fa_attn_bwd_host.hpp.  Both
// run the windowed dK/dV and dQ kernels of csrc/fa_attn_bwd_kernel.hpp, so they
// share a unit; the sink entry adds the dsinks launch.
#include "fa_attn_bwd_host.hpp"

FA_ATTN_BWD_ENTRY(fa_attn_bwd_win_bf16, __bf16, WIN)
FA_ATTN_BWD_ENTRY(fa_attn_bwd_sink_bf16, __bf16, SINK)
