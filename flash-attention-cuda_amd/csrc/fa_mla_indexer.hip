// fa_mla_indexer.hip -- the MLA sparse indexer: index logits over a flat pool
// of index keys and the top-k row selection that feeds fa_mla_sparse_*
// (include/fa_mi355x_mla_indexer.h).  The host bodies are
// csrc/fa_mla_indexer_host.hpp, the kernels csrc/fa_mla_indexer_kernel.hpp
// (DESIGN.md §3.0x).
#include "fa_mla_indexer_host.hpp"

FA_MLA_INDEXER_ENTRY(fa_mla_indexer_logits_f16, fa::f16, false, )
FA_MLA_INDEXER_ENTRY(fa_mla_indexer_logits_bf16, __bf16, false, )
FA_MLA_INDEXER_ENTRY(fa_mla_indexer_logits_k8_f16, fa::f16, true, , const float* k_scale)
FA_MLA_INDEXER_ENTRY(fa_mla_indexer_logits_k8_bf16, __bf16, true, , const float* k_scale)

extern "C" int fa_mla_indexer_topk(const float* logits, const int* ks, const int* ke, int* indices, int num_tokens,
                                   int num_rows, int max_len, long long logits_stride, int topk,
                                   void* hip_stream) {
  return fa::mla_indexer_topk_entry(logits, ks, ke, indices, num_tokens, num_rows, max_len, logits_stride, topk,
                                    hip_stream);
}
