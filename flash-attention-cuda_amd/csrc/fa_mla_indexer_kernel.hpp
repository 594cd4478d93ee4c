// The MLA sparse indexer for gfx950 (DeepSeek-V3.2's DSA): the two kernels that
// produce the index lists fa_mla_sparse_kernel.hpp consumes.
//
//   logits[n][j - ks[n]] = k_scale[j] * sum_h w[n][h] * max(0, sum_d q[n][h][d] k[j][d])   ks[n] <= j < ke[n]
//   indices[n][:]        = the flat rows ks[n] + c of the min(topk, len) largest logits, ascending, then -1
//
// over a flat pool of index keys k [num_rows][128] (16-bit, or E4M3 bytes with
// one fp32 scale per row), 64 index heads of 128 dims per token.
//
// ---- fa_mla_indexer_logits_kernel --------------------------------------------
// Operand orientation.  One wave holds one token.  Its Q, 64 heads x 128 dims,
// is the MFMA A operand and stays in registers for the whole launch (16
// fragments of 8 elements, 64 VGPRs): heads are the M dimension, keys the N
// dimension, so the accumulator of lane (g, r) of v_mfma_f32_16x16x32 holds
// heads 16 hb + 4 g + i (i < 4) of key r.  The ReLU-weighted head sum is then
// sixteen max/FMA pairs in the lane (hb ascending, i ascending, one FMA chain
// from 0) and two cross-lane adds (lanes l ^ 16, then l ^ 32): the four chains
// g = 0..3 are added as (g0 + g1) + (g2 + g3).  That order is fixed, so two
// calls give the same bits.  The four weights a lane needs per head block are
// loaded once.
//
// Key staging.  A workgroup is four waves = four consecutive tokens x one chunk
// of the flat row space (blockIdx.y).  Keys go through a workgroup-shared LDS
// image in 64-key tiles aligned to 64 pool rows, two images, filled by LDS-DMA
// (buffer_load_dwordx4 ... lds, each wave a quarter of the tile) one tile ahead
// of the MFMAs, one barrier per tile.  The image is fa_fwd_kernel.hpp's image B
// (256-B rows, 16-B chunk XOR row & 15) for 16-bit keys and its 128-B twin
// (chunk XOR (row >> 1) & 7) for FP8 keys: the B-operand row reads, sixteen
// lanes = sixteen keys at one chunk, are conflict-free in both.  The tile's
// descriptor starts at the tile's first row (64-bit base) and ends at the
// pool's end, so a pool past 4 GiB is reached and no byte outside it is read.
//
// Tile walk.  ks and ke are read and clamped on the device (indexer_range).
// The workgroup walks the tiles of [min ks, max ke) of its non-empty tokens,
// cut to its chunk; a wave computes a tile only if it meets its own token's
// range, and stores only the keys inside it (lane 16 g + r stores key 16 g + r
// of the tile: 256 contiguous bytes per wave).  A key of another token's range,
// or of none, that shares the tile is multiplied and dropped: it is a column of
// its own in every MFMA and in the head sum, so whatever it holds (NaN
// included) reaches no stored value.  Prefill tokens share almost all their
// tiles; decode tokens share none, their waves idle in each other's tiles, and
// the parallelism is the chunk dimension's.  No workgroup depends on another.
//
// The FP8 variant (K8) stages bytes and converts them in registers (cvt_fp8x8,
// exact).  A lane's 16-B read is dims 64 tt + 16 g .. + 15, which feed k-steps
// 2 tt and 2 tt + 1; Q's fragments are loaded in the same dim order (an MFMA's
// contraction index is free as long as both operands agree).  k_scale[j] is
// multiplied once onto the finished sum.
//
// ---- fa_mla_indexer_topk_kernel ----------------------------------------------
// One workgroup of 1024 threads per token.  A logit maps to a 32-bit key whose
// unsigned order is the IEEE order (-0 first made +0).  Four radix passes of 8
// bits, most significant first, each a 256-bin LDS histogram of the candidates
// that match the digits found so far, find the key K of the topk-th largest
// logit and r, how many logits equal to K belong to the list.  Lanes that share
// a digit are counted by a ballot and added once (up to four rounds) before the
// rest go to vector LDS atomics, so clustered logits do not serialise on one
// bin.  The last pass walks the columns in ascending order, 1024 at a time:
// ballots and per-wave counts through LDS give each column the number of
// greater and of equal logits before it; a column is kept if its key is greater
// than K or equal with fewer than r equal ones before it, and is written at
// (greater before) + min(equal before, r): ascending rows, lowest columns among
// the ties, no sort.  A token with len <= topk writes its whole range and pads
// with -1.  Only integer compares decide, so NaN logits are ordered somewhere
// and every entry stays inside the token's range.
#pragma once

#include "fa_decode_kernel.hpp"

namespace fa {

constexpr int kIdxHeads = 64;    // index heads per token
constexpr int kIdxDim = 128;     // dims per index head
constexpr int kIdxTile = 64;     // keys per LDS tile
constexpr int kIdxTokens = 4;    // tokens per workgroup: one per wave
constexpr int kIdxLdsBytes = 2 * kIdxTile * kIdxDim * 2;  // two tile images of 16-bit keys (FP8: half)
constexpr int kIdxTopkThreads = 1024;

struct MlaIndexerParams {
  const void* q;         // [N][64][128] 16-bit
  const void* k;         // [num_rows][128] 16-bit or E4M3
  const float* k_scale;  // fp32 [num_rows] (K8 only)
  const float* weights;  // fp32 [N][64]
  const int* ks;
  const int* ke;
  float* logits;         // fp32 [N][.], row stride logits_stride elements
  int* indices;          // int32 [N][topk] (the selection)
  long long logits_stride;
  int num_tokens;
  int num_rows;
  int max_len;
  int topk;
  int chunk_rows;        // rows per blockIdx.y, a multiple of 64
};

// token's range after the contract's clamp: 0 <= s <= e <= num_rows, e - s <= max_len
__device__ __forceinline__ void indexer_range(int ks, int ke, int num_rows, int max_len, int& s, int& e) {
  s = min(max(ks, 0), num_rows);
  e = min(max(ke, s), num_rows);
  e = (int)min((long long)e, (long long)s + max_len);
}

// LDS byte offset of 16-B chunk `ch` of key `row` in the FP8 tile image, and
// the source offset (row * 128 + chunk * 16) of image byte o
__device__ __forceinline__ int k8_off16(int row, int ch) { return 128 * row + 16 * (ch ^ ((row >> 1) & 7)); }
__device__ __forceinline__ int k8_off16_src(int o) {
  const int row = o >> 7;
  return 128 * row + 16 * (((o >> 4) & 7) ^ ((row >> 1) & 7));
}

template <class T, bool K8>
__global__ __launch_bounds__(256, 2) void fa_mla_indexer_logits_kernel(MlaIndexerParams p) {
  constexpr int ROWB = K8 ? kIdxDim : 2 * kIdxDim;  // bytes of one key
  constexpr int IMG = kIdxTile * ROWB;              // one tile image
  constexpr int NT = kIdxDim / 32;                  // k-steps
  constexpr int NHB = kIdxHeads / 16;               // head blocks
  static_assert(2 * IMG <= kIdxLdsBytes && kIdxLdsBytes == 32768, "two tile images in 32 KB");
  __shared__ __attribute__((aligned(16))) char smem[2 * IMG];
  typedef typename Elem<T>::x8 tx8;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;

  // the four tokens' ranges (every wave reads all four: the walk is the workgroup's)
  const long long n0 = (long long)blockIdx.x * kIdxTokens;
  int lo = 0x7fffffff, hi = 0, ms = 0, me = 0;
#pragma unroll
  for (int w = 0; w < kIdxTokens; ++w) {
    int s = 0, e = 0;
    if (n0 + w < p.num_tokens) indexer_range(p.ks[n0 + w], p.ke[n0 + w], p.num_rows, p.max_len, s, e);
    s = __builtin_amdgcn_readfirstlane(s);
    e = __builtin_amdgcn_readfirstlane(e);
    if (s < e) {
      lo = min(lo, s);
      hi = max(hi, e);
    }
    if (w == wave) {
      ms = s;
      me = e;
    }
  }
  const long long c0 = (long long)blockIdx.y * p.chunk_rows;
  const long long c1 = c0 + p.chunk_rows;
  if (lo >= hi || c0 >= hi || c1 <= lo) return;
  const int t0 = (int)(max((long long)lo, c0) >> 6);
  const int t1 = (int)((min((long long)hi, c1) + 63) >> 6);
  const long long n = n0 + wave;

  // Q fragments (A operand): qf[hb][s] = Q[16 hb + r16][dims of k-step s, 8 per lane group g]
  tx8 qf[NHB][NT];
  float wt[NHB][4];
  if (ms < me) {
    const __amdgpu_buffer_rsrc_t rq =
        make_rsrc(static_cast<const char*>(p.q) + (size_t)n * (kIdxHeads * kIdxDim * 2), kIdxHeads * kIdxDim * 2);
#pragma unroll
    for (int hb = 0; hb < NHB; ++hb) {
#pragma unroll
      for (int s = 0; s < NT; ++s) {
        const int d0 = K8 ? 64 * (s >> 1) + 16 * g + 8 * (s & 1) : 32 * s + 8 * g;
        qf[hb][s] = __builtin_bit_cast(tx8, buf_load16(rq, (16 * hb + r16) * (kIdxDim * 2) + 2 * d0));
      }
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(p.weights + (size_t)n * kIdxHeads + 16 * hb + 4 * g);
#pragma unroll
      for (int i = 0; i < 4; ++i) wt[hb][i] = w4[i];
    }
  } else {
#pragma unroll
    for (int hb = 0; hb < NHB; ++hb) {
#pragma unroll
      for (int s = 0; s < NT; ++s) qf[hb][s] = tx8{};
#pragma unroll
      for (int i = 0; i < 4; ++i) wt[hb][i] = 0.f;
    }
  }

  // tile t -> image img: this wave's quarter, IMG / 4096 DMA instructions of 1 KB
  auto issue = [&](int t, char* img) {
    const int left = p.num_rows - 64 * t;  // > 0: t < t1 <= ceil(num_rows / 64)
    const __amdgpu_buffer_rsrc_t rk =
        make_rsrc(static_cast<const char*>(p.k) + (size_t)t * IMG, min(left, kIdxTile) * ROWB);
#pragma unroll
    for (int i = 0; i < IMG / 4096; ++i) {
      const int o = 1024 * ((IMG / 4096) * wave + i);
      buf_load16_lds(rk, img + o, K8 ? k8_off16_src(o + 16 * lane) : k_off16_src(o + 16 * lane));
    }
  };

  float* const out = p.logits + (size_t)n * (size_t)p.logits_stride;
  issue(t0, smem);
  for (int t = t0; t < t1; ++t) {
    const char* cur = smem + ((t - t0) & 1) * IMG;
    // this wave's pieces of tile t have landed; after the barrier every wave's
    // have, and every wave is done with the other image (tile t - 1)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t + 1 < t1) issue(t + 1, smem + ((t + 1 - t0) & 1) * IMG);
    if (64 * (long long)t >= me || 64 * (long long)t + 64 <= ms) continue;  // not this token's tile

    float mine = 0.f;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      // B operand: key 16 cb + r16, one 16-B chunk per k-step (FP8: per two)
      tx8 kf[NT];
      if constexpr (K8) {
#pragma unroll
        for (int tt = 0; tt < NT / 2; ++tt) {
          const u32x4 w = *reinterpret_cast<const u32x4*>(cur + k8_off16(16 * cb + r16, 4 * tt + g));
          kf[2 * tt] = cvt_fp8x8<T>(w[0], w[1]);
          kf[2 * tt + 1] = cvt_fp8x8<T>(w[2], w[3]);
        }
      } else {
#pragma unroll
        for (int s = 0; s < NT; ++s) kf[s] = *reinterpret_cast<const tx8*>(cur + k_off16(16 * cb + r16, 4 * s + g));
      }
      f32x4 acc[NHB];
#pragma unroll
      for (int s = 0; s < NT; ++s)
#pragma unroll
        for (int hb = 0; hb < NHB; ++hb) acc[hb] = Elem<T>::mfma(qf[hb][s], kf[s], s == 0 ? f32x4{} : acc[hb]);
      // sum_h w[h] relu(s[h]) of key 16 cb + r16: this lane's sixteen heads, then the four lane groups
      float part = 0.f;
#pragma unroll
      for (int hb = 0; hb < NHB; ++hb)
#pragma unroll
        for (int i = 0; i < 4; ++i) part = __builtin_fmaf(wt[hb][i], fmaxf(acc[hb][i], 0.f), part);
      part = sum_xor32(sum_xor16(part));
      mine = g == cb ? part : mine;
    }
    const long long j = 64 * (long long)t + lane;  // key 16 g + r16 of the tile
    if (j >= ms && j < me) {
      if constexpr (K8) mine *= p.k_scale[j];
      out[j - ms] = mine;
    }
  }
}

// a logit's bits -> a key whose unsigned order is the IEEE order; -0 is +0
__device__ __forceinline__ unsigned indexer_key(unsigned u) {
  u = u == 0x80000000u ? 0u : u;
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

__global__ __launch_bounds__(kIdxTopkThreads) void fa_mla_indexer_topk_kernel(MlaIndexerParams p) {
  constexpr int NW = kIdxTopkThreads / 64;
  __shared__ unsigned hist[256];
  __shared__ unsigned pick[2];         // the pass's digit and what is still needed below it
  __shared__ unsigned counts[2][NW][2];  // per chunk parity and wave: greater, equal

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t n = blockIdx.x;
  int s, e;
  indexer_range(p.ks[n], p.ke[n], p.num_rows, p.max_len, s, e);
  const int len = e - s, topk = p.topk;
  int* const out = p.indices + n * (size_t)topk;
  if (len <= topk) {
    for (int c = tid; c < topk; c += kIdxTopkThreads) out[c] = c < len ? s + c : -1;
    return;
  }
  const unsigned* const row = reinterpret_cast<const unsigned*>(p.logits) + n * (size_t)p.logits_stride;

  // K = the key of the topk-th largest logit, need = how many equal to K are kept
  unsigned prefix = 0, need = (unsigned)topk;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    const unsigned himask = shift == 24 ? 0u : ~0u << (shift + 8);
    for (int c0 = 0; c0 < len; c0 += kIdxTopkThreads) {
      const int c = c0 + tid;
      const unsigned key = c < len ? indexer_key(row[c]) : 0u;
      bool todo = c < len && (key & himask) == prefix;
      const unsigned d = (key >> shift) & 255u;
      for (int round = 0; round < 4; ++round) {
        const unsigned long long left = __builtin_amdgcn_ballot_w64(todo);
        if (left == 0) break;
        const unsigned lead = (unsigned)__builtin_amdgcn_readlane((int)d, (int)__builtin_ctzll(left));
        const unsigned long long same = __builtin_amdgcn_ballot_w64(todo && d == lead);
        if (todo && d == lead) {
          if ((same & ((1ull << lane) - 1)) == 0) atomicAdd(&hist[lead], (unsigned)__builtin_popcountll(same));
          todo = false;
        }
      }
      if (todo) atomicAdd(&hist[d], 1u);
    }
    __syncthreads();
    if (wave == 0) {
      // bins 4 lane .. 4 lane + 3; above = the candidates in higher bins
      unsigned cnt[4], tot = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        cnt[j] = hist[4 * lane + j];
        tot += cnt[j];
      }
      unsigned suf = tot;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned y = (unsigned)__shfl_down((int)suf, off);
        if (lane + off < 64) suf += y;
      }
      unsigned above = suf - tot;
#pragma unroll
      for (int j = 3; j >= 0; --j) {
        if (above < need && above + cnt[j] >= need) {
          pick[0] = 4 * lane + j;
          pick[1] = need - above;
        }
        above += cnt[j];
      }
    }
    __syncthreads();
    prefix |= pick[0] << shift;
    need = pick[1];
    // (the next pass's zeroing of hist is behind this barrier, its reads of pick before the next write)
  }

  // ordered compaction: columns ascending, 1024 at a time
  const unsigned K = prefix, r = need;
  unsigned gt_base = 0, eq_base = 0;
  int par = 0;
  for (int c0 = 0; c0 < len; c0 += kIdxTopkThreads, par ^= 1) {
    const int c = c0 + tid;
    const unsigned key = c < len ? indexer_key(row[c]) : 0u;
    const bool gt = c < len && key > K, eq = c < len && key == K;
    const unsigned long long mg = __builtin_amdgcn_ballot_w64(gt), me = __builtin_amdgcn_ballot_w64(eq);
    if (lane == 0) {
      counts[par][wave][0] = (unsigned)__builtin_popcountll(mg);
      counts[par][wave][1] = (unsigned)__builtin_popcountll(me);
    }
    __syncthreads();
    unsigned gt_before = gt_base, eq_before = eq_base;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const unsigned cg = counts[par][w][0], ce = counts[par][w][1];
      gt_before += w < wave ? cg : 0u;
      eq_before += w < wave ? ce : 0u;
      gt_base += cg;
      eq_base += ce;
    }
    const unsigned long long below = (1ull << lane) - 1;
    gt_before += (unsigned)__builtin_popcountll(mg & below);
    eq_before += (unsigned)__builtin_popcountll(me & below);
    if (gt || (eq && eq_before < r)) {
      const unsigned pos = gt_before + min(eq_before, r);
      if (pos < (unsigned)topk) out[pos] = s + c;
    }
  }
}

}  // namespace fa
