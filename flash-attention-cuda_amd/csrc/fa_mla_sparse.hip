// fa_mla_sparse.hip -- MLA sparse attention: every query token attends to the
// latent rows its index list names (fa_mla_sparse_f16 / _bf16 of
// include/fa_mi355x_mla_sparse.h).  The host body is
// csrc/fa_mla_sparse_host.hpp, the kernel csrc/fa_mla_sparse_kernel.hpp
// (DESIGN.md §3.0w).
#include "fa_mla_sparse_host.hpp"

FA_MLA_SPARSE_ENTRY(fa_mla_sparse_f16, FA_DTYPE_F16)
FA_MLA_SPARSE_ENTRY(fa_mla_sparse_bf16, FA_DTYPE_BF16)
