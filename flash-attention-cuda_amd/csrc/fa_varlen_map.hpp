// The workgroup -> (sequence, block) map of the packed (cu_seqlens) entries:
// prefill (fa_prefill_kernel.hpp, 128-row query blocks) and cache append
// (fa_cache_append_kernel.hpp, append_block_tokens() tokens), DESIGN.md §3.0l.
//
//   T   = rows of the packed tensors, cu = device int32[nseq + 1]
//   s_b = clamp(cu[b], 0, T),  e_b = clamp(cu[b + 1], s_b, T),  n_b = e_b - s_b
//   f(b) = s_b / BT + b                         b in [0, nseq]
//
// Sequence b owns the virtual block ids [f(b), f(b + 1)); block r = id - f(b)
// covers its rows [BT r, BT r + BT), so blocks are aligned to the sequence's
// own start whatever packed row that is.  For monotone cu, f is strictly
// increasing, the range is never shorter than ceil(n_b / BT) (it is s_{b+1} /
// BT - s_b / BT + 1 >= n_b / BT + 1), and f(nseq) <= T / BT + nseq: the host
// launches T / BT + nseq ids from shapes alone, with no pre-pass and no look
// at cu.  A workgroup finds its b by bisection on f: ceil(log2(nseq + 2))
// dependent scalar loads, all wave-uniform.  An id below f(0), at or past
// f(nseq), or with BT r >= n_b has nothing to do.
//
// Every index into cu lies in [0, nseq] and every (s, n) returned satisfies
// 0 <= s, 0 <= n, s + n <= T whatever cu holds: garbage or non-monotone
// values give an unspecified but in-bounds assignment.
#pragma once

namespace fa {

// false: this id has no block.  Otherwise sequence b, its first packed row s,
// its row count n and the block r (BT r < n), all wave-uniform.
template <int BT>
__device__ __forceinline__ bool varlen_block(const int* cu_, int nseq, int total, int id, int& b,
                                             int& s, int& n, int& r) {
  typedef const __attribute__((address_space(4))) int* cu_t;  // scalar loads
  const cu_t cu = (cu_t)cu_;
  // the number of b in [0, nseq] with f(b) <= id (a prefix: f increases)
  int lo = 0, hi = nseq + 1;
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    const int sm = min(max(cu[mid], 0), total);
    if (sm / BT + mid <= id)
      lo = mid + 1;
    else
      hi = mid;
  }
  if (lo == 0 || lo > nseq) return false;
  b = lo - 1;
  s = min(max(cu[b], 0), total);
  n = min(max(cu[b + 1], s), total) - s;
  r = id - (s / BT + b);
  return r < (n + BT - 1) / BT;
}

// The same map where cu may be absent (the uniform mode of the token-major
// attention entries, fa_attn_varlen_*): entry i is then i * S, never a load,
// and the host has checked nseq * S == total.  A twin of varlen_block(), not a
// parameter of it: the packed entries' instantiations stay what they were.
__device__ __forceinline__ int varlen_start(const int* cu_, int S, int total, int i) {
  typedef const __attribute__((address_space(4))) int* cu_t;  // scalar loads
  return cu_ ? min(max(((cu_t)cu_)[i], 0), total) : min(i * S, total);
}
template <int BT>
__device__ __forceinline__ bool varlen_block_u(const int* cu_, int S, int nseq, int total, int id,
                                               int& b, int& s, int& n, int& r) {
  int lo = 0, hi = nseq + 1;
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (varlen_start(cu_, S, total, mid) / BT + mid <= id)
      lo = mid + 1;
    else
      hi = mid;
  }
  if (lo == 0 || lo > nseq) return false;
  b = lo - 1;
  s = varlen_start(cu_, S, total, b);
  n = max(varlen_start(cu_, S, total, b + 1), s) - s;
  r = id - (s / BT + b);
  return r < (n + BT - 1) / BT;
}

}  // namespace fa
