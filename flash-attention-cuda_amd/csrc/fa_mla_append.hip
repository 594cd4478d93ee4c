// fa_mla_append.hip -- the writers of the MLA caches
// (include/fa_mi355x_mla_append.h): the latent append with fused RoPE into the
// four latent cache forms and the quantising writer of the indexer's FP8 key
// pool.  The host bodies are csrc/fa_mla_append_host.hpp, the kernels
// csrc/fa_mla_append_kernel.hpp.
#include "fa_mla_append_host.hpp"

FA_MLA_APPEND_ENTRIES(fa_mla_append, CONTIG, KV16)
FA_MLA_APPEND_ENTRIES(fa_mla_append_paged, PAGED, KV16)
FA_MLA_APPEND_ENTRIES(fa_mla_append_kv8, CONTIG, KV8)
FA_MLA_APPEND_ENTRIES(fa_mla_append_paged_kv8, PAGED, KV8)

FA_MLA_INDEXER_APPEND_ENTRY(fa_mla_indexer_append_k8_f16, fa::f16, CONTIG)
FA_MLA_INDEXER_APPEND_ENTRY(fa_mla_indexer_append_k8_bf16, __bf16, CONTIG)
FA_MLA_INDEXER_APPEND_ENTRY(fa_mla_indexer_append_k8_paged_f16, fa::f16, PAGED)
FA_MLA_INDEXER_APPEND_ENTRY(fa_mla_indexer_append_k8_paged_bf16, __bf16, PAGED)
