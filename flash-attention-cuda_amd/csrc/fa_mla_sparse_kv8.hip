// fa_mla_sparse_kv8.hip -- MLA sparse attention over an FP8 (E4M3) latent pool:
// every query token attends to the rows of a pool of bytes its index list names
// (fa_mla_sparse_kv8_f16 / _bf16 of include/fa_mi355x_mla_sparse_kv8.h).  The
// host body is csrc/fa_mla_sparse_kv8_host.hpp, the kernel
// csrc/fa_mla_sparse_kv8_kernel.hpp.
#include "fa_mla_sparse_kv8_host.hpp"

FA_MLA_SPARSE_KV8_ENTRY(fa_mla_sparse_kv8_f16, FA_DTYPE_F16)
FA_MLA_SPARSE_KV8_ENTRY(fa_mla_sparse_kv8_bf16, FA_DTYPE_BF16)
