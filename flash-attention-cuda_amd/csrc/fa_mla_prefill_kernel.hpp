// MLA prefill for gfx950: attention over token-major Q, K and V with no cache
// in the non-absorbed form of Multi-head Latent Attention (DeepSeek-V2 / V3 /
// R1, Kimi K2): the score contracts over 192 dims (k = [k_nope 128 | k_pe 64]),
// the value has 128, and the softmax scale is the caller's
// (include/fa_mi355x_mla_prefill.h).
//
//   s[i,j]   = softmax_scale * sum_{d<192} q[i,h,d] k[j,hkv,d],  hkv = h / (Hq / Hkv)
//   O[i,h,:] = sum_j softmax_j(s[i,.]) v[j,hkv,0:128]
//   causal (bottom-right): row i of sequence b sees keys j <= nk_b - nq_b + i
//
// Work split.  A workgroup is (virtual 128-row query block, query head), four
// waves of 32 rows; fa_varlen_map.hpp turns the block id into (sequence, block)
// on the device, causal ids are taken from the top (a sequence's heaviest block
// first) and the `group` query heads of a K/V head are adjacent ids, so they
// stream the same K/V tiles through L2.  Key tiles are 64 keys.
//
// LDS.  Two buffers of one K image (64 x 384 B = 24 KB) and one V image (64 x
// 256 B = 16 KB): 80 KB, two workgroups per CU.
//   K image: packed 384-B rows, three 128-B groups of eight 16-B chunks, the
//     chunk within its group XORed with (row >> 1) & 7:
//       off(row, ch) = 384 row + 128 (ch >> 3) + 16 ((ch & 7) ^ ((row >> 1) & 7))
//     384 row mod 256 = 128 (row & 1), so modulo a 256-B bank row the 16-B slot
//     is 8 ((row & 1) ^ ((ch >> 3) & 1)) + ((ch & 7) ^ ((row >> 1) & 7)).
//     Operand read (ds_read_b128, S^T = K . Q^T): a pass is sixteen lanes = the
//     sixteen rows of a key block at one ch; (row & 1, (row >> 1) & 7) takes
//     sixteen distinct values, so sixteen distinct slots.  Staging write
//     (ds_write_b128): eight consecutive lanes are the eight chunks of one
//     128-B group of one row, the eight distinct slots of a 128-B bank row,
//     and the next eight lanes are the next row, the other half of the 256.
//   V image: image A of fa_fwd_kernel.hpp (lds_off), read with
//     ds_read_b64_tr_b16 for O^T += V^T . P^T, staged by M16's lane map.
//   Staging goes through registers (6 + 4 16-byte loads per lane and tile, K's
//   issued before the tile's score MFMAs and V's after them, both written after
//   the tile's last MFMA, one barrier per tile):
//   a tile's rows past the sequence's keys then arrive as zeros from the
//   descriptor's range check alone, where LDS-DMA needs a zero-fill pass of the
//   image first, and the 40 staging VGPRs fit (below).
//
// Registers per wave (32 rows = two 16-row blocks): Q fragments 2 x 6 x 4 = 48,
// O^T 2 x 8 x 4 = 64, scores 32, P 16, staging 40; no scratch.
//
// Softmax.  Scores leave the MFMA chain unscaled and are multiplied by
// softmax_scale log2(e) in fp32 for both element types; the running maximum is
// exact (per tile), l sums the fp32 exponentials and P is their rounding to T.
// O is rescaled only when some row's maximum moved (x 1.0 is exact).
//
// Tiles wholly above a wave's rows are skipped wave-uniformly (the wave still
// stages and takes the barrier); the mask is applied only to tiles that cross
// the diagonal or the end of the keys.  Tail rows and keys are the descriptors'
// range: zero-filled loads, dropped stores.
#pragma once

#include "fa_decode_kernel.hpp"
#include "fa_varlen_map.hpp"

namespace fa {

constexpr int kMlaPfDqk = 192;                   // dims of a query / key row
constexpr int kMlaPfDv = 128;                    // dims of a value / output row
constexpr int kMlaPfQRow = 2 * kMlaPfDqk;        // bytes per Q / K row
constexpr int kMlaPfVRow = 2 * kMlaPfDv;         // bytes per V / O row
constexpr int kMlaPfBM = 128;                    // query rows per workgroup
constexpr int kMlaPfKImg = 64 * kMlaPfQRow;      // one K image
constexpr int kMlaPfVImg = 64 * kMlaPfVRow;      // one V image
constexpr int kMlaPfLdsBytes = 2 * (kMlaPfKImg + kMlaPfVImg);
static_assert(kMlaPfLdsBytes == 80 * 1024 && 2 * kMlaPfLdsBytes <= 160 * 1024,
              "two workgroups share a CU's 160 KB of LDS");

struct MlaPrefillParams {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  float* lse;            // [Hq][T_q] natural-log LSE, or nullptr
  const int* cu_q;       // device int32[nseq + 1], or nullptr (uniform)
  const int* cu_k;       // device int32[nseq + 1], or nullptr (uniform)
  int useq_q, useq_k;    // the uniform lengths (read where the cu is nullptr)
  int q_sb, k_sb, v_sb;  // bytes between consecutive tokens of Q, K and V
  int hq, hkv, group;    // group = hq / hkv
  int tq, tk, nseq;
  int causal;
  float c;               // softmax_scale * log2(e)
};

// byte offset of 16-B chunk `ch` (0..23) of row `row` (0..63) in a K image
__device__ __forceinline__ int mla_pf_k_off(int row, int ch) {
  return kMlaPfQRow * row + 128 * (ch >> 3) + 16 * ((ch & 7) ^ ((row >> 1) & 7));
}

template <class T>
__global__ __launch_bounds__(256, 2) void fa_mla_prefill_kernel(MlaPrefillParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int BN = 64, BM = kMlaPfBM, RW = 32, QB = 2;
  constexpr int NTQ = kMlaPfDqk / 32;  // 32-wide k-steps of QK^T
  constexpr int NE = kMlaPfDv / 16;    // 16-wide d-blocks of O
  constexpr int NKB = BN / 16, NU = BN / 32;
  constexpr int QROW = kMlaPfQRow, VROW = kMlaPfVRow;
  constexpr int BUF = kMlaPfKImg + kMlaPfVImg;
  constexpr int NK = 6, NV = 4;  // staging loads per lane and tile
  typedef typename Elem<T>::x8 tx8;
  typedef typename Elem<T>::x4 tx4;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  const int sg = ((g & 1) << 1) | (g >> 1);

  // workgroup -> (virtual block id, kv head, head of the group)
  const unsigned gi = blockIdx.x % (unsigned)p.group;
  const unsigned rest = blockIdx.x / (unsigned)p.group;
  const int hk = (int)(rest % (unsigned)p.hkv);
  int id = (int)(rest / (unsigned)p.hkv);
  if (p.causal) id = p.tq / BM + p.nseq - 1 - id;
  int b, s0, nq, qb;
  if (!varlen_block_u<BM>(p.cu_q, p.useq_q, p.nseq, p.tq, id, b, s0, nq, qb)) return;
  b = __builtin_amdgcn_readfirstlane(b);
  s0 = __builtin_amdgcn_readfirstlane(s0);
  nq = __builtin_amdgcn_readfirstlane(nq);
  qb = __builtin_amdgcn_readfirstlane(qb);
  const int hq = hk * p.group + (int)gi;
  const int q0 = qb * BM;
  // the keys' span, clamped to [0, T_k]
  int sk = varlen_start(p.cu_k, p.useq_k, p.tk, b);
  int len = max(varlen_start(p.cu_k, p.useq_k, p.tk, b + 1), sk) - sk;
  sk = __builtin_amdgcn_readfirstlane(sk);
  len = __builtin_amdgcn_readfirstlane(len);
  const int off = len - nq;  // keys before the first row's diagonal (negative: leading rows see nothing)
  const int kv_hi = p.causal ? max(0, min(len, off + q0 + BM)) : len;
  const int ntiles = (kv_hi + BN - 1) / BN;
  const int qwl = wave * RW;                                     // the wave's first row in the block
  const int qwm = p.causal ? off + q0 + qwl : 0x3fffffff;        // ... as the mask sees it

  // Q, O, LSE: the block's valid rows; the range ends with the last one's own bytes
  const int qrows = min(nq - q0, BM);
  const int qsq = p.q_sb, qso = p.hq * VROW;
  const __amdgpu_buffer_rsrc_t rq =
      make_rsrc(static_cast<const char*>(p.q) + ((size_t)s0 + q0) * (size_t)qsq + (size_t)hq * QROW,
                (qrows - 1) * qsq + QROW);
  const __amdgpu_buffer_rsrc_t ro =
      make_rsrc(static_cast<char*>(p.o) + (((size_t)s0 + q0) * (size_t)p.hq + hq) * VROW,
                (qrows - 1) * qso + VROW);

  // Q fragments (B operand): qf[bb][t] = Q[qwl + 16 bb + r16][32 t + 8 g .. +7]
  tx8 qf[QB][NTQ];
#pragma unroll
  for (int bb = 0; bb < QB; ++bb)
#pragma unroll
    for (int t = 0; t < NTQ; ++t)
      qf[bb][t] = __builtin_bit_cast(tx8, buf_load16(rq, (qwl + 16 * bb + r16) * qsq + (4 * t + g) * 16));

  // Staging lanes.  K: pass i = 3 h + grp loads chunk 8 grp + (tid & 7) of row
  // 32 h + (tid >> 3).  V: M16's map (two rows of opposite parity x 4 chunks
  // per 8 lanes), pass i rows 16 i further.
  const int ksb = p.k_sb, vsb = p.v_sb;
  const int kr = tid >> 3, kc = tid & 7;
  const int kvo = kr * ksb + kc * 16;
  const int klo = QROW * kr + 16 * (kc ^ ((kr >> 1) & 7));
  const int vr = 4 * wave + 2 * ((lane >> 5) & 1) + ((lane >> 2) & 1);
  const int vc = 4 * ((lane >> 3) & 3) + (lane & 3);
  const int vvo = vr * vsb + vc * 16;
  const int vlo = lds_off(vr, vc);  // + 4096 i: 16 rows further
  const char* Kh = static_cast<const char*>(p.k) + (size_t)sk * (size_t)ksb + (size_t)hk * QROW;
  const char* Vh = static_cast<const char*>(p.v) + (size_t)sk * (size_t)vsb + (size_t)hk * VROW;
  u32x4 kst[NK], vst[NV];
  // tile tl's loads: its descriptors start at its first row and end with its
  // last visible row's own bytes, so a lane's 16 bytes of row r are inside iff
  // r is visible (the strides are >= a token's heads); a tile past kv_hi has
  // zero bytes and moves nothing
  auto issue_k = [&](int tl) {
    const int live = max(0, min(kv_hi - BN * tl, BN));
    const size_t r0 = (size_t)min(BN * tl, kv_hi);
    const __amdgpu_buffer_rsrc_t rk = make_rsrc(Kh + r0 * (size_t)ksb, live > 0 ? (live - 1) * ksb + QROW : 0);
#pragma unroll
    for (int i = 0; i < NK; ++i)
      kst[i] = __builtin_amdgcn_raw_buffer_load_b128(rk, kvo + 32 * (i / 3) * ksb + 128 * (i % 3), 0, 0);
  };
  auto issue_v = [&](int tl) {
    const int live = max(0, min(kv_hi - BN * tl, BN));
    const size_t r0 = (size_t)min(BN * tl, kv_hi);
    const __amdgpu_buffer_rsrc_t rv = make_rsrc(Vh + r0 * (size_t)vsb, live > 0 ? (live - 1) * vsb + VROW : 0);
#pragma unroll
    for (int i = 0; i < NV; ++i) vst[i] = __builtin_amdgcn_raw_buffer_load_b128(rv, vvo + 16 * i * vsb, 0, 0);
  };
  auto write_lds = [&](char* kb) {
    char* vb = kb + kMlaPfKImg;
#pragma unroll
    for (int i = 0; i < NK; ++i)
      *reinterpret_cast<u32x4*>(kb + klo + 32 * QROW * (i / 3) + 128 * (i % 3)) = kst[i];
#pragma unroll
    for (int i = 0; i < NV; ++i) *reinterpret_cast<u32x4*>(vb + vlo + 4096 * i) = vst[i];
  };

  // A-operand addresses.  QK^T: A row r16 of key block cb is key 16 cb +
  // sigma(r16), so the S^T accumulator of lane (g, r16) holds keys 16 cb + 4 sg
  // + i, the order the transposed V reads deliver (fa_decode_kernel.hpp); chunk
  // 4 t + g of that row: + 6144 cb + 128 (t >> 1) on ka[t & 1]
  const int krow = 4 * ((((r16 >> 2) & 1) << 1) | (r16 >> 3)) + (r16 & 3);
  int ka[2], vaddr[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) ka[h] = mla_pf_k_off(krow, 4 * h + g);
  {
    const int qq = r16 >> 2, pp = r16 & 3;
#pragma unroll
    for (int ep = 0; ep < 2; ++ep)
      vaddr[ep] = 2048 * (sg >> 1) + 64 * (4 * (sg & 1) + qq) + 16 * ((2 * ep + (pp >> 1)) ^ sg) + 8 * (pp & 1);
  }

  f32x4 acc[QB][NE];
  float m[QB], lsum[QB];
#pragma unroll
  for (int bb = 0; bb < QB; ++bb) {
#pragma unroll
    for (int e = 0; e < NE; ++e) acc[bb][e] = f32x4{};
    m[bb] = ninf();
    lsum[bb] = 0.f;
  }

  // prologue: tile 0 (every load, Q's included, has retired before the loop)
  issue_k(0);
  issue_v(0);
  write_lds(smem);
#pragma unroll
  for (int bb = 0; bb < QB; ++bb)
#pragma unroll
    for (int t = 0; t < NTQ; ++t) asm volatile("" : "+v"(qf[bb][t]));
  __syncthreads();

  for (int j = 0; j < ntiles; ++j) {
    const char* kb = smem + (j & 1) * BUF;
    const char* vb = kb + kMlaPfKImg;
    const int kv0 = j * BN;
    // wave-uniform: does any key of this tile lie at or below some row of this wave?
    const bool active = kv0 <= qwm + RW - 1;
    // the next tile's loads, past kv_hi zero bytes and no memory traffic: K's
    // before the score MFMAs, V's after them (its four staging registers are
    // not live beside the score chain's operands)
    issue_k(j + 1);
    f32x4 s[QB][NKB];
    if (active) {
      // S^T = K . Q^T: six k-steps over the tile's four 16-key blocks
#pragma unroll
      for (int t = 0; t < NTQ; ++t)
#pragma unroll
        for (int cb = 0; cb < NKB; ++cb) {
          const tx8 kf = *reinterpret_cast<const tx8*>(kb + ka[t & 1] + 16 * QROW * cb + 128 * (t >> 1));
#pragma unroll
          for (int bb = 0; bb < QB; ++bb)
            s[bb][cb] = Elem<T>::mfma(kf, qf[bb][t], t == 0 ? f32x4{} : s[bb][cb]);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    issue_v(j + 1);
    __builtin_amdgcn_sched_barrier(0);
    if (active) {
      const bool need_mask = (kv0 + BN > kv_hi) || (kv0 + BN - 1 > qwm);
      tx8 pf[QB][NU];
#pragma unroll
      for (int bb = 0; bb < QB; ++bb) {
#pragma unroll
        for (int cb = 0; cb < NKB; ++cb) s[bb][cb] *= p.c;
        if (need_mask) {
          const int qrow = qwm + 16 * bb + r16;
#pragma unroll
          for (int cb = 0; cb < NKB; ++cb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int kv = kv0 + 16 * cb + 4 * sg + i;
              s[bb][cb][i] = (kv < kv_hi && kv <= qrow) ? s[bb][cb][i] : ninf();
            }
        }
        float mx = s[bb][0][0];
#pragma unroll
        for (int cb = 0; cb < NKB; ++cb)
#pragma unroll
          for (int i = (cb == 0 ? 1 : 0); i < 4; ++i) mx = fmaxf(mx, s[bb][cb][i]);
        mx = max_xor32(max_xor16(mx));
        const float mnew = fmaxf(m[bb], mx);
        const float msafe = mnew == ninf() ? 0.f : mnew;  // a row that has seen no key yet
        const float alpha = __builtin_amdgcn_exp2f(m[bb] - msafe);
        m[bb] = mnew;
        lsum[bb] *= alpha;
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {  // (x 1.0 is exact: the same bits either way)
#pragma unroll
          for (int e = 0; e < NE; ++e) acc[bb][e] *= alpha;
        }
        // l takes the fp32 exponentials, P their rounding to T
#pragma unroll
        for (int cb = 0; cb < NKB; ++cb)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float ex = __builtin_amdgcn_exp2f(s[bb][cb][i] - msafe);
            pf[bb][cb >> 1][4 * (cb & 1) + i] = (T)ex;
            lsum[bb] += ex;
          }
      }
      // O^T += V^T . P^T
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int e = 0; e < NE; ++e) {
          const int base = 8192 * u + 512 * (e >> 1) + vaddr[e & 1];
          const tx4 lo = __builtin_bit_cast(tx4, lds_read_tr(vb, base));
          const tx4 hi = __builtin_bit_cast(tx4, lds_read_tr(vb, base + 4096));
          const tx8 vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
          for (int bb = 0; bb < QB; ++bb) acc[bb][e] = Elem<T>::mfma(vf, pf[bb][u], acc[bb][e]);
        }
    }
    write_lds(smem + ((j + 1) & 1) * BUF);
    __syncthreads();
  }

  // Epilogue: lane (g, r16) holds d = 16 e + 4 g + 0..3 of row r16 for every e;
  // one permlane16 swap per dword of a d-block pair leaves each lane 8
  // contiguous d of one row (M16::store_o), rows past the block's last dropped
  const __amdgpu_buffer_rsrc_t rl =
      make_rsrc(p.lse ? p.lse + (size_t)hq * (size_t)p.tq + s0 + q0 : nullptr, p.lse ? qrows * 4 : 0);
#pragma unroll
  for (int bb = 0; bb < QB; ++bb) {
    const float L = sum_xor32(sum_xor16(lsum[bb]));
    const float inv = L > 0.f ? 1.0f / L : 0.f;
    const int row = qwl + 16 * bb + r16;
    const int dlane = 16 * (g & 1) + 8 * (g >> 1);
#pragma unroll
    for (int ep = 0; ep < NE / 2; ++ep) {
      tx4 wx, wy;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        wx[x] = (T)(acc[bb][2 * ep][x] * inv);
        wy[x] = (T)(acc[bb][2 * ep + 1][x] * inv);
      }
      u32x2 X = __builtin_bit_cast(u32x2, wx), Y = __builtin_bit_cast(u32x2, wy);
#pragma unroll
      for (int dw = 0; dw < 2; ++dw) {
        const auto r = __builtin_amdgcn_permlane16_swap(X[dw], Y[dw], false, false);
        X[dw] = r[0];
        Y[dw] = r[1];
      }
      __builtin_amdgcn_raw_buffer_store_b128(u32x4{X[0], X[1], Y[0], Y[1]}, ro,
                                             row * qso + 2 * (32 * ep + dlane), 0, kOStoreAux);
    }
    const float lse = L > 0.f ? (m[bb] + __builtin_log2f(L)) * 0.6931471805599453f : ninf();
    if (g == 0) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, lse), rl, row * 4, 0, 0);
  }
}

}  // namespace fa
