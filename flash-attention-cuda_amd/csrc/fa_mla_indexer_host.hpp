// Host side of the MLA indexer entries of include/fa_mi355x_mla_indexer.h: the
// two entry bodies (the checks in the header's order), the parameters and the
// launches.  Neither kernel has a workspace or a dynamic LDS size.
#pragma once

#include <hip/hip_runtime.h>

#include "fa_mi355x_mla_indexer.h"
#include "fa_mla_indexer_kernel.hpp"

namespace fa {

// the checks both entries share, up to the NULL pointers (which differ)
static int mla_indexer_sizes(int num_tokens, int heads, int num_rows, int max_len, long long logits_stride,
                             int topk) {
  if (num_tokens < 0 || heads < 0 || num_rows < 0 || max_len < 0 || topk < 0 || logits_stride < max_len)
    return FA_ERR_BAD_SHAPE;
  if (heads != kIdxHeads) return FA_ERR_BAD_SHAPE;
  return FA_OK;
}

template <class T, bool K8>
static int mla_indexer_logits_entry(const void* q, const void* k, const float* k_scale, const float* weights,
                                    const int* ks, const int* ke, float* logits, int num_tokens, int heads,
                                    int num_rows, int max_len, long long logits_stride, void* hip_stream) {
  if (const int rc = mla_indexer_sizes(num_tokens, heads, num_rows, max_len, logits_stride, 0)) return rc;
  if (num_tokens == 0) return FA_OK;
  if (!q || !k || !weights || !ks || !ke || !logits || (K8 && !k_scale)) return FA_ERR_NULL_POINTER;
  if (max_len == 0 || num_rows == 0) return FA_OK;  // every range is empty: no logit is written
  MlaIndexerParams p = {};
  p.q = q;
  p.k = k;
  p.k_scale = k_scale;
  p.weights = weights;
  p.ks = ks;
  p.ke = ke;
  p.logits = logits;
  p.logits_stride = logits_stride;
  p.num_tokens = num_tokens;
  p.num_rows = num_rows;
  p.max_len = max_len;
  // chunks of 32 tiles, more where the pool would need more than 65535 of them
  const long long tiles = ((long long)num_rows + 63) / 64;
  const long long per = std::max(32ll, (tiles + 65534) / 65535);
  p.chunk_rows = (int)(64 * per);
  const dim3 grid((unsigned)((num_tokens + kIdxTokens - 1) / kIdxTokens), (unsigned)((tiles + per - 1) / per));
  hipLaunchKernelGGL((fa_mla_indexer_logits_kernel<T, K8>), grid, dim3(256), 0, (hipStream_t)hip_stream, p);
  return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
}

static int mla_indexer_topk_entry(const float* logits, const int* ks, const int* ke, int* indices, int num_tokens,
                                  int num_rows, int max_len, long long logits_stride, int topk,
                                  void* hip_stream) {
  if (const int rc = mla_indexer_sizes(num_tokens, kIdxHeads, num_rows, max_len, logits_stride, topk)) return rc;
  if (num_tokens == 0) return FA_OK;
  if (!logits || !ks || !ke || !indices) return FA_ERR_NULL_POINTER;
  if (topk == 0) return FA_OK;  // the lists hold nothing
  // (max_len == 0 or num_rows == 0: every clamped range is empty and the kernel pads every list with -1)
  MlaIndexerParams p = {};
  p.ks = ks;
  p.ke = ke;
  p.logits = const_cast<float*>(logits);
  p.indices = indices;
  p.logits_stride = logits_stride;
  p.num_tokens = num_tokens;
  p.num_rows = num_rows;
  p.max_len = max_len;
  p.topk = topk;
  hipLaunchKernelGGL(fa_mla_indexer_topk_kernel, dim3((unsigned)num_tokens), dim3(kIdxTopkThreads), 0,
                     (hipStream_t)hip_stream, p);
  return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
}

}  // namespace fa

// fa_mla_indexer_logits_{f16,bf16} and fa_mla_indexer_logits_k8_{f16,bf16} of
// include/fa_mi355x_mla_indexer.h (the K8 entries take k_scale after the stream)
#define FA_MLA_INDEXER_ARGS                                                                               \
  const void *q, const void *k, const float *weights, const int *ks, const int *ke, float *logits,       \
      int num_tokens, int heads, int num_rows, int max_len, long long logits_stride, void *hip_stream
#define FA_MLA_INDEXER_ENTRY(NAME, T, K8, ...)                                                            \
  extern "C" int NAME(FA_MLA_INDEXER_ARGS __VA_ARGS__) {                                                  \
    return fa::mla_indexer_logits_entry<T, K8>(q, k, FA_MLA_INDEXER_SCALE_##K8, weights, ks, ke, logits,  \
                                               num_tokens, heads, num_rows, max_len, logits_stride,       \
                                               hip_stream);                                               \
  }
#define FA_MLA_INDEXER_SCALE_false nullptr
#define FA_MLA_INDEXER_SCALE_true k_scale
