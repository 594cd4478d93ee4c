// Backward pass (dQ, dK, dV) of the attention over token-major Q, K and V with
// no cache (the fa_attn_varlen_bwd_* entries), for gfx950.
//
//   c = 1 / sqrt(D),  s_ij = c q_i . k_j,  P_ij = exp(s_ij - LSE_i) on the keys
//   row i sees (the forward's: its own sequence, causal j <= nk_b - nq_b + i),
//   delta_i = sum_d dO_id O_id,  dP_ij = dO_i . v_j,  dS_ij = P_ij (dP_ij - delta_i)
//   dV_j = sum_i P_ij dO_i,  dK_j = c sum_i dS_ij q_i,  dQ_i = c sum_j dS_ij k_j
//
// Three kernels, no sum across workgroups, no atomics, no fp32 buffer but
// delta: S and dP are computed twice (7 matrix products per tile pair where
// the fused form has 5), once with the key on the MFMA lane for dK / dV and
// once with the query row on it for dQ.
//
//  * fa_attn_bwd_delta_kernel: delta[h][t] for the rows of a sequence.
//  * fa_attn_bwd_dkdv_kernel: a workgroup owns 128 keys of one (sequence, K/V
//    head), a wave 32 of them: their K and V rows sit in registers as the B
//    operands of S = Q K^T and dP = dO V^T (v_mfma_f32_16x16x32, key = column
//    = lane & 15), and dK^T, dV^T (d x key) in fp32 accumulators for the whole
//    sweep over the group's query heads x the 64-row query tiles that can see
//    the block.  A tile's Q and dO go through one LDS image each, read by rows
//    (A operand of S / dP) and by columns (ds_read_b64_tr_b16: A operand of
//    dK^T += Q^T dS, dV^T += dO^T P).  The accumulators of two 16-row S tiles
//    are, converted, the B operand of those products over 32 rows: element j
//    of lane group h is row 16 (j >> 2) + 4 h + (j & 3), which is the order
//    the transposed reads deliver.
//  * fa_attn_bwd_dq_kernel: the same body with the roles swapped.  A workgroup
//    owns 128 query rows of one (sequence, query head), a wave 32: Q and dO
//    rows in registers (B operands, row = lane & 15), -LSE and delta one
//    value per lane, dQ^T in accumulators; K and V tiles of 64 keys through
//    the LDS images (rows: S^T = K Q^T, dP^T = V dO^T; columns: dQ^T += K^T dS^T).
//
// Rows and keys outside a sequence are never read (every descriptor ends with
// the last owned row's bytes, so they come as zeros) nor written (the store
// descriptors end the same way).  A masked element is selected to 0, never
// multiplied; a row whose LSE is -inf takes -inf as its exponent offset, so
// exp(-inf - (-inf)) is never formed.
//
// The sliding window and the sinks (fa_attn_bwd_win_* / fa_attn_bwd_sink_*,
// DESIGN.md §3.0r).  The dK/dV and dQ kernels take WIN from their parameter
// type, Windowed<AttnBwdParams>, as the forward's kernels do, and every line
// of it stands under `if constexpr (WIN)`: the instantiations of the entries
// without a window keep their device code, instruction for instruction.
// Row t of a sequence then sees the keys lo <= j with lo = off + t - W + 1 (off
// = nk - nq); the host gives W = total_k where there is no window, which
// excludes no key, and has checked that total_q + total_k fits an int.  WIN
// adds one comparison to the mask and bounds the sweeps: the dK/dV sweep ends
// at the tile of the last row whose window reaches the block, the dQ sweep
// starts at the tile of the first key its block's first row sees, and a wave
// skips a 32-row (32-key) sub-block that lies wholly outside.  The sinks need
// nothing there: the forward's LSE holds them.  Their own gradient is
// fa_attn_bwd_dsinks_kernel, a fourth launch.
#pragma once

#include "fa_prefill_kernel.hpp"

namespace fa {

constexpr int kBwdBN = 128;   // keys per dK/dV workgroup
constexpr int kBwdBM = 128;   // query rows per dQ workgroup (the forward's block)
constexpr int kBwdTile = 64;  // rows of the swept tiles (queries for dK/dV, keys for dQ)
// two images of 64 rows in 256-B slots, then 64 floats of -LSE log2(e) and 64 of delta
constexpr int kBwdLdsBytes = 2 * kBwdTile * 256 + 2 * kBwdTile * 4;

struct AttnBwdParams {
  const void* dout;
  const void* q;
  const void* k;
  const void* v;
  const void* out;
  const float* lse;  // [Hq][T_q] natural log
  void* dq;
  void* dk;
  void* dv;
  float* delta;      // [Hq][T_q]
  const int* cu_q;   // device int32[B + 1], or nullptr (uniform)
  const int* cu_k;
  int useq_q, useq_k;
  int do_sb, q_sb, k_sb, v_sb;  // bytes between consecutive tokens
  int hq, hkv, group;
  int tq, tk, nseq;
  int causal;
  float c;           // 1 / sqrt(D)
};

// LDS image of a [64][D] tile: 256-B row slots, the 16-B chunk XORed so that
// the row reads and the transposed reads both spread over the banks
__device__ __forceinline__ int bwd_off(int row, int ch) {
  return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}
// the address lane l16 = 4 q + p of a 16-lane group gives ds_read_b64_tr_b16
// for the 4-row x 16-column block at (r0, 16-B chunk c0)
__device__ __forceinline__ int bwd_tr_off(int l16, int r0, int c0) {
  return bwd_off(r0 + (l16 >> 2), c0 + ((l16 >> 1) & 1)) + 8 * (l16 & 1);
}

// Two [64][D] tiles (rows sa / sb bytes apart, the descriptors ending at the
// last live row) staged through registers into the two images.
template <int HDIM>
struct BwdStage {
  static constexpr int ROW = 2 * HDIM, CPR = ROW / 16, NCH = kBwdTile * CPR / 256;
  u32x4 a[NCH], b[NCH];
  __device__ __forceinline__ void issue(__amdgpu_buffer_rsrc_t ra, int sa, __amdgpu_buffer_rsrc_t rb,
                                        int sb, int tid) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int ci = tid + 256 * i, row = ci / CPR, ch = ci % CPR;
      a[i] = __builtin_amdgcn_raw_buffer_load_b128(ra, row * sa + ch * 16, 0, 0);
      b[i] = __builtin_amdgcn_raw_buffer_load_b128(rb, row * sb + ch * 16, 0, 0);
    }
  }
  __device__ __forceinline__ void write(char* ia, char* ib, int tid) const {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int ci = tid + 256 * i, row = ci / CPR, ch = ci % CPR;
      *reinterpret_cast<u32x4*>(ia + bwd_off(row, ch)) = a[i];
      *reinterpret_cast<u32x4*>(ib + bwd_off(row, ch)) = b[i];
    }
  }
};

template <class T>
__device__ __forceinline__ typename Elem<T>::x8 bwd_pack(f32x4 lo, f32x4 hi) {
  typename Elem<T>::x8 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = (T)lo[i], r[4 + i] = (T)hi[i];
  return r;
}
template <class T>
__device__ __forceinline__ void bwd_store4(__amdgpu_buffer_rsrc_t r, int off, f32x4 v, float sc) {
  typename Elem<T>::x4 t;
#pragma unroll
  for (int i = 0; i < 4; ++i) t[i] = (T)(v[i] * sc);
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, t), r, off, 0, 0);
}
// the exponent offset of a row: -LSE log2(e); -inf for a row that saw no key
__device__ __forceinline__ float bwd_nl(float lse) {
  return lse == ninf() ? ninf() : -lse * 1.4426950408889634f;
}

// delta[h][t] = sum_d float(dO[t][h][d]) float(O[t][h][d]) for the rows of a
// sequence.  Workgroup = one 128-row block of the packed map; ROW / 16 lanes
// per (token, head), 16 bytes each.
template <class T, int HDIM>
__global__ __launch_bounds__(256) void fa_attn_bwd_delta_kernel(AttnBwdParams p) {
  constexpr int ROW = 2 * HDIM, LPG = ROW / 16, PPW = 256 / LPG;
  typedef typename Elem<T>::x8 tx8;
  int b, s0, nq, qb;
  if (!varlen_block_u<kBwdBM>(p.cu_q, p.useq_q, p.nseq, p.tq, (int)blockIdx.x, b, s0, nq, qb)) return;
  const int q0 = qb * kBwdBM;
  const int rows = min(nq - q0, kBwdBM);
  const int npair = rows * p.hq;
  const int sub = threadIdx.x % LPG, grp = threadIdx.x / LPG;
  for (int base = 0; base < npair; base += PPW) {
    const int idx = base + grp;
    const bool live = idx < npair;
    float acc = 0.f;
    int row = 0, head = 0;
    if (live) {
      row = idx / p.hq, head = idx - row * p.hq;
      const size_t t = (size_t)s0 + q0 + row;
      const tx8 a = *reinterpret_cast<const tx8*>(static_cast<const char*>(p.dout) + t * (size_t)p.do_sb +
                                                  (size_t)head * ROW + sub * 16);
      const tx8 o = *reinterpret_cast<const tx8*>(static_cast<const char*>(p.out) +
                                                  (t * (size_t)p.hq + head) * ROW + sub * 16);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc = __builtin_fmaf((float)a[i], (float)o[i], acc);
    }
#pragma unroll
    for (int m = LPG / 2; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
    if (live && sub == 0) p.delta[(size_t)head * p.tq + s0 + q0 + row] = acc;
  }
}

// WIN: the last row whose window still holds a key, from the first row that
// sees it under the causal mask (key - off; either may lie outside the
// sequence); otherwise unused
template <bool WIN, class P>
__device__ __forceinline__ int bwd_last_row([[maybe_unused]] const P& p, [[maybe_unused]] int first) {
  if constexpr (WIN)
    return first + p.window - 1;
  else
    return 0;
}

// P: AttnBwdParams, or Windowed<AttnBwdParams> (WIN)
template <class T, int HDIM, class P = AttnBwdParams>
__global__ __launch_bounds__(256) void fa_attn_bwd_dkdv_kernel(P p) {
  constexpr bool WIN = ParamsWindowed<P>::value;
  constexpr int BN = kBwdBN, BT = kBwdTile, ROW = 2 * HDIM, NS = HDIM / 32, NE = HDIM / 16;
  constexpr int KB = BN / 64;  // 16-key blocks per wave
  typedef typename Elem<T>::x8 tx8;
  typedef typename Elem<T>::x4 tx4;
  __shared__ __attribute__((aligned(16))) char smem[kBwdLdsBytes];
  char* const qi = smem;
  char* const di = smem + BT * 256;
  float* const nls = reinterpret_cast<float*>(smem + 2 * BT * 256);
  float* const dls = nls + BT;

  const int tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, h = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hk = (int)(blockIdx.x % (unsigned)p.hkv);
  const int id = (int)(blockIdx.x / (unsigned)p.hkv);
  int b, sk, nk, r;
  if (!varlen_block_u<BN>(p.cu_k, p.useq_k, p.nseq, p.tk, id, b, sk, nk, r)) return;
  b = __builtin_amdgcn_readfirstlane(b);
  sk = __builtin_amdgcn_readfirstlane(sk);
  nk = __builtin_amdgcn_readfirstlane(nk);
  r = __builtin_amdgcn_readfirstlane(r);
  int s0 = varlen_start(p.cu_q, p.useq_q, p.tq, b);
  int nq = max(varlen_start(p.cu_q, p.useq_q, p.tq, b + 1), s0) - s0;
  s0 = __builtin_amdgcn_readfirstlane(s0);
  nq = __builtin_amdgcn_readfirstlane(nq);
  const int k0 = r * BN;
  const int live = min(BN, nk - k0);  // > 0: the map's guarantee
  const int off = nk - nq;
  // causal: the first query tile with a row that reaches the block's first key
  const int j0 = p.causal ? max(0, k0 - off) / BT : 0;
  // WIN: ... and the sweep ends with the last row whose window reaches the
  // block (lo <= its last key); no such row: no tile
  const int last = bwd_last_row<WIN>(p, k0 + live - 1 - off);
  const int nt = WIN ? (last < 0 ? 0 : max(0, min((nq + BT - 1) / BT, last / BT + 1) - j0))
                     : max(0, (nq + BT - 1) / BT - j0);
  const int total = nt * p.group;
  const int kw = 32 * wave;  // this wave's first key within the block
  const float c2 = p.c * 1.4426950408889634f;

  // this wave's K and V rows: B operands (key = lane & 15, d = 32 s + 8 h + ..)
  tx8 kf[KB][NS], vf[KB][NS];
  {
    const auto rk = make_rsrc(static_cast<const char*>(p.k) + ((size_t)sk + k0) * (size_t)p.k_sb +
                                  (size_t)hk * ROW, (live - 1) * p.k_sb + ROW);
    const auto rv = make_rsrc(static_cast<const char*>(p.v) + ((size_t)sk + k0) * (size_t)p.v_sb +
                                  (size_t)hk * ROW, (live - 1) * p.v_sb + ROW);
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int n = kw + 16 * kb + l16;
        kf[kb][s] = __builtin_bit_cast(
            tx8, __builtin_amdgcn_raw_buffer_load_b128(rk, n * p.k_sb + 64 * s + 16 * h, 0, 0));
        vf[kb][s] = __builtin_bit_cast(
            tx8, __builtin_amdgcn_raw_buffer_load_b128(rv, n * p.v_sb + 64 * s + 16 * h, 0, 0));
      }
  }
  f32x4 dk[KB][NE], dv[KB][NE];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb)
#pragma unroll
    for (int e = 0; e < NE; ++e) dk[kb][e] = f32x4{0, 0, 0, 0}, dv[kb][e] = f32x4{0, 0, 0, 0};

  // the swept items: (query head of the group, query tile), heads outermost
  BwdStage<HDIM> st;
  float st_f = 0.f;  // tid < 64: LSE of row tid; 64 <= tid < 128: delta of row tid - 64
  auto issue = [&](int it) {
    const int g = it / nt, j = j0 + (it - g * nt);
    const int hq = hk * p.group + g;
    const int rows = min(BT, nq - BT * j);
    const size_t t0 = (size_t)s0 + BT * j;
    const auto rq = make_rsrc(static_cast<const char*>(p.q) + t0 * (size_t)p.q_sb + (size_t)hq * ROW,
                              (rows - 1) * p.q_sb + ROW);
    const auto rd = make_rsrc(static_cast<const char*>(p.dout) + t0 * (size_t)p.do_sb + (size_t)hq * ROW,
                              (rows - 1) * p.do_sb + ROW);
    st.issue(rq, p.q_sb, rd, p.do_sb, tid);
    const size_t l0 = (size_t)hq * (size_t)p.tq + t0;
    const auto rl = make_rsrc(p.lse + l0, rows * 4);
    const auto re = make_rsrc(p.delta + l0, rows * 4);
    // rows past the sequence: offset past the range, so 0
    const float a = __builtin_bit_cast(
        float, __builtin_amdgcn_raw_buffer_load_b32(rl, tid < BT ? tid * 4 : 0x7ffffff0, 0, 0));
    const float d = __builtin_bit_cast(
        float, __builtin_amdgcn_raw_buffer_load_b32(re, (tid >= BT && tid < 2 * BT) ? (tid - BT) * 4 : 0x7ffffff0, 0, 0));
    st_f = tid < BT ? bwd_nl(a) : d;
  };
  auto write = [&]() {
    st.write(qi, di, tid);
    if (tid < 2 * BT) nls[tid] = st_f;  // nls and dls are adjacent
  };

  auto compute = [&](int it) {
    const int j = j0 + it % nt;
    const int i0 = BT * j;
#pragma unroll
    for (int sub = 0; sub < BT / 32; ++sub) {
      const int ib = 32 * sub;
      // wave-uniform: no row of these 32 in the sequence, or none reaches this wave's keys
      if (i0 + ib >= nq) continue;
      if (p.causal && off + i0 + ib + 31 < k0 + kw) continue;
      // ... or the window of the first of them (and so of all) starts past this wave's keys
      if constexpr (WIN)
        if (off + i0 + ib - p.window + 1 > k0 + kw + 31) continue;
      f32x4 s[2][KB], dp[2][KB];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) s[t][kb] = f32x4{0, 0, 0, 0}, dp[t][kb] = f32x4{0, 0, 0, 0};
#pragma unroll
        for (int ss = 0; ss < NS; ++ss) {
          const int o = bwd_off(ib + 16 * t + l16, 4 * ss + h);
          const tx8 aq = *reinterpret_cast<const tx8*>(qi + o);
          const tx8 ad = *reinterpret_cast<const tx8*>(di + o);
#pragma unroll
          for (int kb = 0; kb < KB; ++kb) {
            s[t][kb] = Elem<T>::mfma(aq, kf[kb][ss], s[t][kb]);
            dp[t][kb] = Elem<T>::mfma(ad, vf[kb][ss], dp[t][kb]);
          }
        }
      }
      // P and dS of rows ib + 16 t + 4 h + i, key kw + 16 kb + l16
      tx8 pb[KB], db[KB];
      {
        f32x4 nl[2], de[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          nl[t] = *reinterpret_cast<const f32x4*>(nls + ib + 16 * t + 4 * h);
          de[t] = *reinterpret_cast<const f32x4*>(dls + ib + 16 * t + 4 * h);
        }
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
          const int key = k0 + kw + 16 * kb + l16;
          f32x4 pv[2], ds[2];
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int row = i0 + ib + 16 * t + 4 * h + i;
              bool ok = row < nq && key < nk && (!p.causal || key <= off + row);
              if constexpr (WIN) ok = ok && key > off + row - p.window;
              const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(s[t][kb][i], c2, nl[t][i]));
              pv[t][i] = ok ? e : 0.f;
              ds[t][i] = ok ? e * (dp[t][kb][i] - de[t][i]) : 0.f;
            }
          pb[kb] = bwd_pack<T>(pv[0], pv[1]);
          db[kb] = bwd_pack<T>(ds[0], ds[1]);
        }
      }
      // dV^T += dO^T P, dK^T += Q^T dS over these 32 rows
#pragma unroll
      for (int e = 0; e < NE; ++e) {
        const int o0 = bwd_tr_off(l16, ib + 4 * h, 2 * e), o1 = bwd_tr_off(l16, ib + 16 + 4 * h, 2 * e);
        const tx4 dlo = __builtin_bit_cast(tx4, lds_read_tr(di, o0));
        const tx4 dhi = __builtin_bit_cast(tx4, lds_read_tr(di, o1));
        const tx4 qlo = __builtin_bit_cast(tx4, lds_read_tr(qi, o0));
        const tx4 qhi = __builtin_bit_cast(tx4, lds_read_tr(qi, o1));
        const tx8 ad = __builtin_shufflevector(dlo, dhi, 0, 1, 2, 3, 4, 5, 6, 7);
        const tx8 aq = __builtin_shufflevector(qlo, qhi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
          dv[kb][e] = Elem<T>::mfma(ad, pb[kb], dv[kb][e]);
          dk[kb][e] = Elem<T>::mfma(aq, db[kb], dk[kb][e]);
        }
      }
    }
  };

  if (total > 0) {
    issue(0);
    write();
  }
  __syncthreads();
  for (int it = 0; it < total; ++it) {
    const bool more = it + 1 < total;  // workgroup-uniform
    if (more) issue(it + 1);
    compute(it);
    __syncthreads();
    if (more) write();
    __syncthreads();
  }

  // dK[key][d] = c dK^T[d][key]; a lane holds d = 16 e + 4 h + (0..3) of key l16
  const size_t orow = ((size_t)sk + k0) * (size_t)p.hkv + hk;
  const int os = p.hkv * ROW;
  const auto rdk = make_rsrc(static_cast<char*>(p.dk) + orow * ROW, (live - 1) * os + ROW);
  const auto rdv = make_rsrc(static_cast<char*>(p.dv) + orow * ROW, (live - 1) * os + ROW);
#pragma unroll
  for (int kb = 0; kb < KB; ++kb)
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int o = (kw + 16 * kb + l16) * os + (16 * e + 4 * h) * 2;
      bwd_store4<T>(rdk, o, dk[kb][e], p.c);
      bwd_store4<T>(rdv, o, dv[kb][e], 1.f);
    }
}

// P: as for the dK/dV kernel
template <class T, int HDIM, class P = AttnBwdParams>
__global__ __launch_bounds__(256) void fa_attn_bwd_dq_kernel(P p) {
  constexpr bool WIN = ParamsWindowed<P>::value;
  constexpr int BM = kBwdBM, BT = kBwdTile, ROW = 2 * HDIM, NS = HDIM / 32, NE = HDIM / 16;
  constexpr int IB = BM / 64;  // 16-row blocks per wave
  typedef typename Elem<T>::x8 tx8;
  typedef typename Elem<T>::x4 tx4;
  __shared__ __attribute__((aligned(16))) char smem[2 * BT * 256];
  char* const ki = smem;
  char* const vi = smem + BT * 256;

  const int tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, h = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hq = (int)(blockIdx.x % (unsigned)p.hq);
  int id = (int)(blockIdx.x / (unsigned)p.hq);
  // causal: the ids from the top, so a sequence's heaviest blocks start first
  if (p.causal) id = p.tq / BM + p.nseq - 1 - id;
  int b, s0, nq, qb;
  if (!varlen_block_u<BM>(p.cu_q, p.useq_q, p.nseq, p.tq, id, b, s0, nq, qb)) return;
  b = __builtin_amdgcn_readfirstlane(b);
  s0 = __builtin_amdgcn_readfirstlane(s0);
  nq = __builtin_amdgcn_readfirstlane(nq);
  qb = __builtin_amdgcn_readfirstlane(qb);
  int sk = varlen_start(p.cu_k, p.useq_k, p.tk, b);
  int nk = max(varlen_start(p.cu_k, p.useq_k, p.tk, b + 1), sk) - sk;
  sk = __builtin_amdgcn_readfirstlane(sk);
  nk = __builtin_amdgcn_readfirstlane(nk);
  const int hk = hq / p.group;
  const int q0 = qb * BM;
  const int rows = min(nq - q0, BM);  // > 0: the map's guarantee
  const int off = nk - nq;
  const int kv_hi = p.causal ? max(0, min(nk, off + q0 + BM)) : nk;
  const int ntiles = (kv_hi + BT - 1) / BT;
  // WIN: the tile of the first key the block's first row sees; the tiles below it are never loaded
  int jt0 = 0;
  if constexpr (WIN) jt0 = max(0, off + q0 - p.window + 1) / BT;
  const int qw = 32 * wave;  // this wave's first row within the block
  const float c2 = p.c * 1.4426950408889634f;

  // this wave's Q and dO rows: B operands (row = lane & 15), -LSE log2(e) and delta
  tx8 qf[IB][NS], df[IB][NS];
  float nl[IB], de[IB];
  {
    const size_t t0 = (size_t)s0 + q0;
    const auto rq = make_rsrc(static_cast<const char*>(p.q) + t0 * (size_t)p.q_sb + (size_t)hq * ROW,
                              (rows - 1) * p.q_sb + ROW);
    const auto rd = make_rsrc(static_cast<const char*>(p.dout) + t0 * (size_t)p.do_sb + (size_t)hq * ROW,
                              (rows - 1) * p.do_sb + ROW);
    const size_t l0 = (size_t)hq * (size_t)p.tq + t0;
    const auto rl = make_rsrc(p.lse + l0, rows * 4);
    const auto re = make_rsrc(p.delta + l0, rows * 4);
#pragma unroll
    for (int ib = 0; ib < IB; ++ib) {
      const int n = qw + 16 * ib + l16;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        qf[ib][s] = __builtin_bit_cast(
            tx8, __builtin_amdgcn_raw_buffer_load_b128(rq, n * p.q_sb + 64 * s + 16 * h, 0, 0));
        df[ib][s] = __builtin_bit_cast(
            tx8, __builtin_amdgcn_raw_buffer_load_b128(rd, n * p.do_sb + 64 * s + 16 * h, 0, 0));
      }
      nl[ib] = bwd_nl(__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rl, n * 4, 0, 0)));
      de[ib] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(re, n * 4, 0, 0));
    }
  }
  f32x4 dq[IB][NE];
#pragma unroll
  for (int ib = 0; ib < IB; ++ib)
#pragma unroll
    for (int e = 0; e < NE; ++e) dq[ib][e] = f32x4{0, 0, 0, 0};

  BwdStage<HDIM> st;
  const char* const Kh = static_cast<const char*>(p.k) + (size_t)sk * (size_t)p.k_sb + (size_t)hk * ROW;
  const char* const Vh = static_cast<const char*>(p.v) + (size_t)sk * (size_t)p.v_sb + (size_t)hk * ROW;
  auto issue = [&](int j) {
    const int lv = min(BT, kv_hi - BT * j);
    const auto rk = make_rsrc(Kh + (size_t)(BT * j) * (size_t)p.k_sb, (lv - 1) * p.k_sb + ROW);
    const auto rv = make_rsrc(Vh + (size_t)(BT * j) * (size_t)p.v_sb, (lv - 1) * p.v_sb + ROW);
    st.issue(rk, p.k_sb, rv, p.v_sb, tid);
  };

  auto compute = [&](int j) {
#pragma unroll
    for (int sub = 0; sub < BT / 32; ++sub) {
      const int kb0 = 32 * sub, key0 = BT * j + kb0;
      // wave-uniform: no key of these 32 is seen by a row of this wave
      if (key0 >= kv_hi) continue;
      if (p.causal && key0 > off + q0 + qw + 31) continue;
      // ... or all 32 lie below the window of the wave's first row (and so of all its rows)
      if constexpr (WIN)
        if (key0 + 31 < off + q0 + qw - p.window + 1) continue;
      f32x4 s[2][IB], dp[2][IB];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int ib = 0; ib < IB; ++ib) s[t][ib] = f32x4{0, 0, 0, 0}, dp[t][ib] = f32x4{0, 0, 0, 0};
#pragma unroll
        for (int ss = 0; ss < NS; ++ss) {
          const int o = bwd_off(kb0 + 16 * t + l16, 4 * ss + h);
          const tx8 ak = *reinterpret_cast<const tx8*>(ki + o);
          const tx8 av = *reinterpret_cast<const tx8*>(vi + o);
#pragma unroll
          for (int ib = 0; ib < IB; ++ib) {
            s[t][ib] = Elem<T>::mfma(ak, qf[ib][ss], s[t][ib]);
            dp[t][ib] = Elem<T>::mfma(av, df[ib][ss], dp[t][ib]);
          }
        }
      }
      // dS^T of keys key0 + 16 t + 4 h + i, row qw + 16 ib + l16
      tx8 db[IB];
#pragma unroll
      for (int ib = 0; ib < IB; ++ib) {
        const int row = q0 + qw + 16 * ib + l16;
        f32x4 ds[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int key = key0 + 16 * t + 4 * h + i;
            bool ok = row < nq && key < nk && (!p.causal || key <= off + row);
            if constexpr (WIN) ok = ok && key > off + row - p.window;
            const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(s[t][ib][i], c2, nl[ib]));
            ds[t][i] = ok ? e * (dp[t][ib][i] - de[ib]) : 0.f;
          }
        db[ib] = bwd_pack<T>(ds[0], ds[1]);
      }
      // dQ^T += K^T dS^T over these 32 keys
#pragma unroll
      for (int e = 0; e < NE; ++e) {
        const tx4 lo = __builtin_bit_cast(tx4, lds_read_tr(ki, bwd_tr_off(l16, kb0 + 4 * h, 2 * e)));
        const tx4 hi = __builtin_bit_cast(tx4, lds_read_tr(ki, bwd_tr_off(l16, kb0 + 16 + 4 * h, 2 * e)));
        const tx8 ak = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
        for (int ib = 0; ib < IB; ++ib) dq[ib][e] = Elem<T>::mfma(ak, db[ib], dq[ib][e]);
      }
    }
  };

  if (ntiles > jt0) {
    issue(jt0);
    st.write(ki, vi, tid);
  }
  __syncthreads();
  for (int j = jt0; j < ntiles; ++j) {
    const bool more = j + 1 < ntiles;  // workgroup-uniform
    if (more) issue(j + 1);
    compute(j);
    __syncthreads();
    if (more) st.write(ki, vi, tid);
    __syncthreads();
  }

  // dQ[row][d] = c dQ^T[d][row]; a lane holds d = 16 e + 4 h + (0..3) of row l16
  const int os = p.hq * ROW;
  const auto ro = make_rsrc(static_cast<char*>(p.dq) + (((size_t)s0 + q0) * (size_t)p.hq + hq) * ROW,
                            (rows - 1) * os + ROW);
#pragma unroll
  for (int ib = 0; ib < IB; ++ib)
#pragma unroll
    for (int e = 0; e < NE; ++e)
      bwd_store4<T>(ro, (qw + 16 * ib + l16) * os + (16 * e + 4 * h) * 2, dq[ib][e], p.c);
}

// dsinks[h] = -sum_i exp(sinks[h] - LSE[h][i]) delta[h][i] over the rows of a
// sequence (the sink is one more softmax column whose value is zero, so its dS
// is P_sink (0 - delta)).  Workgroup = one query head.  It walks the sequences
// in order (their spans as the packed map clamps them: the rows whose delta the
// delta kernel wrote, in bounds whatever cu holds), thread t taking the rows t,
// t + NT, .. of each into one fp32 sum; then the butterfly over the lanes and
// the waves' sums in wave order: one fixed order, no atomics.  It is bound by
// the latency of its loads, not their bytes: 1024 threads with both loads of
// eight rows in flight take 8 - 19 us at T_q = 32k where four waves walking
// the 128-row block ids, a bisection each, took 120 us, a tenth of a windowed
// gpt-oss backward.  A row whose LSE is -inf and a head whose
// sink is -inf add nothing, so exp(-inf - (-inf)) is never formed.  NT: the
// workgroup's size (a template so that the units share the kernel).
constexpr int kBwdSinkThreads = 1024;  // the workgroup of fa_attn_bwd_dsinks_kernel

struct AttnBwdSinkParams {
  const float* lse;    // [Hq][T_q]
  const float* delta;  // [Hq][T_q]
  const float* sinks;  // [Hq]
  float* dsinks;       // [Hq]
  const int* cu_q;
  int useq_q, nseq, tq;
};

template <int NT>
__global__ __launch_bounds__(NT) void fa_attn_bwd_dsinks_kernel(AttnBwdSinkParams p) {
  constexpr int NW = NT / 64;
  __shared__ float part[NW];
  const int head = (int)blockIdx.x, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const float sink = p.sinks[head];
  float acc = 0.f;
  if (sink != ninf()) {
    const float* const L = p.lse + (size_t)head * (size_t)p.tq;
    const float* const D = p.delta + (size_t)head * (size_t)p.tq;
    for (int b = 0; b < p.nseq; ++b) {
      const int s0 = varlen_start(p.cu_q, p.useq_q, p.tq, b);
      const int n = max(varlen_start(p.cu_q, p.useq_q, p.tq, b + 1), s0) - s0;
      // both loads whatever the row, so that the unrolled rows' loads are all in flight together
#pragma unroll 8
      for (int r = (int)threadIdx.x; r < n; r += NT) {
        const size_t t = (size_t)s0 + r;
        const float l = L[t], d = D[t];
        const float e = __builtin_amdgcn_exp2f((sink - (l == ninf() ? sink : l)) * 1.4426950408889634f);
        acc = l == ninf() ? acc : __builtin_fmaf(e, d, acc);
      }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) tot += part[w];
    p.dsinks[head] = 0.f - tot;
  }
}

}  // namespace fa
