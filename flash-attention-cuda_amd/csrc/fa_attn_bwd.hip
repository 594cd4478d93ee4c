// fa_attn_bwd.hip -- backward pass (dQ, dK, dV) of the attention over token-major
// Q, K and V (fa_attn_varlen_bwd_f16 of include/fa_mi355x.h), stamped by
// FA_ATTN_BWD_ENTRY next to the host body in csrc/fa_attn_bwd_host.hpp, which
// launches the three kernels of csrc/fa_attn_bwd_kernel.hpp.
#include "fa_attn_bwd_host.hpp"

FA_ATTN_BWD_ENTRY(fa_attn_varlen_bwd_f16, fa::f16, PLAIN)
