// MLA decode for gfx950: a few query tokens (1..16) per head against a latent
// K/V cache (DeepSeek-style Multi-head Latent Attention in its weight-absorbed
// form).  Every query head attends to ONE shared row per token,
//   c[j] = [c_kv (512) | k_pe (64)],
// the score contracts over all 576 dims and the value is the row's first 512:
//
//   s[t,j]     = softmax_scale * sum_{d<576} q[b,h,t,d] c[j,d]
//   O[b,h,t,:] = sum_j softmax_j(s[t,.]) c[j,0:512]
//   causal (bottom-right): token t sees keys j <= len_b - Sq + t
//
// Decomposition.  The Hq*Sq query rows of a batch element share the one latent
// head, and row r = h*Sq + t is contiguous in a [B][Hq][Sq][576] tensor, so
// they form the query dimension of the MFMAs.  A workgroup = (batch, row
// group, key piece), four waves; the element's own 64-key tiles are cut into
// num_splits pieces (the decode kernel's plan, hand-off and workspace).
//
// One fetch, two uses.  A 64-key latent tile (64 x 1152 B = 72 KB) goes from
// HBM straight into a workgroup-shared LDS image by LDS-DMA (no registers),
// once, and feeds both contractions from there:
//   S^T = C . Q^T          A operand = 16 keys x 32 dims, one ds_read_b128 per
//                          lane from the key's row (all 18 k-steps of 576);
//   O^T += C[:, :512]^T . P^T   A operand = 16 dims x 32 keys, the transposed
//                          read ds_read_b64_tr_b16 of the same image.
// The image is fa_fwd_kernel.hpp's image A widened to 576 columns: 8-row x
// 32-column subtiles of 512 B, eighteen per 8 rows (9216 B), the 16-B chunk of
// a row XORed with (row >> 2) & 3.  Both reads are bank-conflict-free in it.
// Two images (144 KB of gfx950's 160 KB) double-buffer the stream: tile i+1's
// DMA is issued before tile i's MFMAs and waited for after them, one
// workgroup barrier per tile.
//
// Two regimes, chosen from rows = Hq*Sq on the host:
//   WIDE (rows > 16): a row group is 64 rows, wave w owns 16-row block w over
//     every key of the piece: Q fragments 18 x 4 = 72 VGPRs, O^T 16 x 512 fp32
//     = 128 VGPRs, its own (m, l); no in-CU merge.
//   narrow (rows <= 16): the four waves share the one 16-row block and split
//     each tile's keys, wave w the 16-key slice w (its PV MFMAs carry 16 live
//     keys and 16 zeros); the four (m, l, O) are merged once through LDS, as
//     the decode kernel's in-CU merge does.
#pragma once

#include "fa_decode_kernel.hpp"

namespace fa {

constexpr int kMlaDqk = 576;               // dims of a latent row and of a query row
constexpr int kMlaDv = 512;                // leading dims of the row that are the value
constexpr int kMlaRow = 2 * kMlaDqk;       // bytes per latent / query row
constexpr int kMlaSub8 = 8 * kMlaRow;      // bytes of 8 rows, in memory and in the image
constexpr int kMlaTile = 8 * kMlaSub8;     // one 64-key tile image
constexpr int kMlaLdsBytes = 2 * kMlaTile; // two images; the narrow merge (130 KB) reuses them

// byte offset of 16-B chunk `ch` (0..71) of row `row` (0..63) in a tile image
__device__ __forceinline__ int mla_lds_off(int row, int ch) {
  return kMlaSub8 * (row >> 3) + 512 * (ch >> 2) + 64 * (row & 7) + 16 * ((ch & 3) ^ ((row >> 2) & 3));
}

// rows but no keys (kv_capacity == 0): O = 0, LSE = -inf.  A kernel, not
// memsets, so that a captured graph holds no memset node.
template <int UNUSED = 0>
__global__ void fa_mla_fill_empty_kernel(unsigned* o_words, float* lse, size_t nwords, size_t nrow) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nwords) o_words[i] = 0u;
  if (lse && i < nrow) lse[i] = ninf();
}

// P = DecodeParams (contiguous: k = the cache [B][cap][576]) or
// DecodePagedParams (k = the pool [num_pages][page_size][576], page_bytes =
// page_size * 1152); hkv = 1, group = hq, c = softmax_scale * log2(e); v is
// not looked at.  Paged code sits under `if constexpr`.
template <class T, bool WIDE, bool PAGED = false, class P = DecodeParams>
__global__ __launch_bounds__(256, 1) void fa_mla_decode_kernel(P p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NB = WIDE ? 4 : 1;   // 16-row blocks per workgroup
  constexpr int RW = 16 * NB;        // query rows per workgroup
  constexpr int NTQ = kMlaDqk / 32;  // 32-wide k-steps of QK^T
  constexpr int NE = kMlaDv / 16;    // 16-wide d-blocks of O
  constexpr int HDIM = kMlaDv;
  constexpr int QROW = kMlaRow, OROW = 2 * kMlaDv;
  constexpr int SUB8 = kMlaSub8;
  typedef typename Elem<T>::x8 tx8;
  typedef typename Elem<T>::x4 tx4;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  const int sg = ((g & 1) << 1) | (g >> 1);

  // workgroup -> (batch, row group, piece)
  const int ns = p.num_splits;
  const unsigned unit = blockIdx.x / (unsigned)ns;
  const int piece = (int)(blockIdx.x - unit * (unsigned)ns);
  const int rg = (int)(unit % (unsigned)p.rgroups);
  const int b = (int)(unit / (unsigned)p.rgroups);
  int len = p.kv_lens ? p.kv_lens[b] : p.cap;
  len = __builtin_amdgcn_readfirstlane(min(max(len, 0), p.cap));
  const int ntiles = (len + 63) >> 6;
  const int t0 = (int)((long long)ntiles * piece / ns);
  const int t1 = (int)((long long)ntiles * (piece + 1) / ns);

  const int row0 = rg * RW;
  const size_t qrow = (size_t)b * p.hq * p.sq;  // [B*Hq*Sq] row of r = 0
  const int nrows = max(0, min(RW, p.rows - row0));
  const __amdgpu_buffer_rsrc_t rq =
      make_rsrc(static_cast<const char*>(p.q) + (qrow + row0) * QROW, nrows * QROW);
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(static_cast<char*>(p.o) + (qrow + row0) * OROW, nrows * OROW);
  // contiguous: one descriptor for the element's rows below its length.
  // Paged: one per tile, built in issue()
  [[maybe_unused]] const __amdgpu_buffer_rsrc_t rcontig =
      make_rsrc(static_cast<const char*>(p.k) + (PAGED ? 0 : (size_t)b * (size_t)p.cap * QROW),
                PAGED ? 0 : len * QROW);

  // Q fragments (B operand) of this wave's row block: qf[t] = Q[16 blk + r16][32 t + 8 g .. +7];
  // rows past the group's last read as zeros
  const int blk = WIDE ? wave : 0;
  tx8 qf[NTQ];
#pragma unroll
  for (int t = 0; t < NTQ; ++t)
    qf[t] = __builtin_bit_cast(tx8, buf_load16(rq, (16 * blk + r16) * QROW + (4 * t + g) * 16));

  // first key the lane's row does not see; tiles ending past mask_from need the mask
  const int lim = p.causal ? len - p.sq + 1 + (row0 + 16 * blk + r16) % p.sq : len;
  const int mask_from = p.causal ? len - p.sq + 1 : len;

  // LDS-DMA: instruction i (0..17) of wave w fills the image's 1-KB piece
  // 18 w + i lane-linearly, i.e. 128 B (two subtiles) of the eight rows
  // 16 w + 8 (i / 9) .. + 7: lane = (subtile, row, slot), and the source chunk
  // is the slot un-XORed.  Per lane the source offset is wsrc[i / 9] + 128 (i % 9).
  const int drow = (lane >> 2) & 7;
  unsigned wsrc[2];
  {
    const unsigned l0 = drow * QROW + 64 * (lane >> 5) + 16 * ((lane & 3) ^ ((lane >> 4) & 1));
    wsrc[0] = (unsigned)(2 * wave) * SUB8 + l0;
    wsrc[1] = (unsigned)(2 * wave + 1) * SUB8 + (l0 ^ 32u);
  }
  // tile tl -> image `img`.  pg, r (paged): the tile's pool page and its
  // 64-row block in it; the descriptor ends at the tile's last live row, an id
  // outside the pool gives no rows.  Rows past the live ones are zero-filled
  // here (they are never read from memory: the loads address them past the range)
  auto issue = [&](int tl, [[maybe_unused]] int pg, [[maybe_unused]] int r, char* img) {
    __amdgpu_buffer_rsrc_t rc;
    unsigned base;
    int live = len - 64 * tl;
    if constexpr (PAGED) {
      const bool ok = (unsigned)pg < (unsigned)p.num_pages;
      if (!ok) live = 0;
      rc = make_rsrc(static_cast<const char*>(p.k) + (size_t)(ok ? pg : 0) * p.page_bytes,
                     (64 * r + min(live, 64)) * QROW);
      base = (unsigned)(64 * r) * QROW;
    } else {
      rc = rcontig;
      base = (unsigned)(64 * tl) * QROW;
    }
    if (live < 64) {
#pragma unroll
      for (int i = 0; i < 18; ++i)
        if (16 * wave + 8 * (i / 9) + drow >= live)
          *reinterpret_cast<u32x4*>(img + (18 * wave + i) * 1024 + 16 * lane) = u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int i = 0; i < 18; ++i)
      buf_load16_lds(rc, img + (18 * wave + i) * 1024, (int)(base + wsrc[i / 9] + 128 * (i % 9)));
  };

  // A-operand addresses.  QK^T: row r16 of 16-key block cb is key 16 cb +
  // sigma(r16), so the S^T accumulator of lane (g, r16) holds keys 16 cb + 4 sg
  // + i, the order the transposed reads deliver (fa_decode_kernel.hpp)
  const int krow = 4 * ((((r16 >> 2) & 1) << 1) | (r16 >> 3)) + (r16 & 3);
  const int kaddr = mla_lds_off(krow, g);  // + 2 SUB8 cb + 512 t
  int vaddr[2];
  {
    const int qq = r16 >> 2, pp = r16 & 3;
#pragma unroll
    for (int ep = 0; ep < 2; ++ep)
      vaddr[ep] = SUB8 * (sg >> 1) + 64 * (4 * (sg & 1) + qq) + 16 * ((2 * ep + (pp >> 1)) ^ sg) + 8 * (pp & 1);
  }

  f32x4 acc[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) acc[e] = f32x4{};
  float m = ninf(), lsum = 0.f;

  // Paged: the page id of the tile after next is fetched (a vector load, so
  // that it rides on the wait the DMA needs anyway) while the next tile's
  // descriptor is built from the id fetched one iteration earlier.  Only
  // entries of tiles below t1 (pages holding a key below len) are read.
  [[maybe_unused]] int j0 = 0, jf = 0, rf = 0, pgn = 0, rn = 0;
  [[maybe_unused]] __amdgpu_buffer_rsrc_t rtab = rcontig;  // (paged: the element's table row)
  if constexpr (PAGED) rtab = make_rsrc(p.table + (size_t)b * p.max_pages, p.max_pages * 4);
  [[maybe_unused]] auto page_id = [&](int j) { return (int)__builtin_amdgcn_raw_buffer_load_b32(rtab, 4 * j, 0, 0); };
  if (t0 < t1) {
    int pg = 0, r = 0;
    if constexpr (PAGED) {
      j0 = t0 / p.tpp;
      r = t0 - j0 * p.tpp;
      pg = __builtin_amdgcn_readfirstlane(page_id(j0));
      jf = j0, rf = r + 1;
      if (rf == p.tpp) rf = 0, ++jf;
      pgn = __builtin_amdgcn_readfirstlane(page_id(t0 + 1 < t1 ? jf : j0));
      rn = rf;
    }
    issue(t0, pg, r, smem);
  }

  for (int tl = t0; tl < t1; ++tl) {
    char* cur = smem + ((tl - t0) & 1) * kMlaTile;
    // this wave's pieces of tile tl have landed; after the barrier every
    // wave's have, and every wave is done with the other image (tile tl - 1)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    [[maybe_unused]] int pgf = 0;
    if (tl + 1 < t1) {
      issue(tl + 1, pgn, rn, smem + ((tl + 1 - t0) & 1) * kMlaTile);
      if constexpr (PAGED) {
        if (++rf == p.tpp) rf = 0, ++jf;
        pgf = page_id(tl + 2 < t1 ? jf : j0);
      }
    }

    const int kv0 = 64 * tl;
    const bool need_mask = kv0 + 64 > mask_from;
    tx8 pf[2];
    if constexpr (WIDE) {
      // S^T = C . Q^T over the tile's four 16-key blocks (four independent chains)
      f32x4 s[4];
#pragma unroll
      for (int t = 0; t < NTQ; ++t)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
          s[cb] = Elem<T>::mfma(*reinterpret_cast<const tx8*>(cur + kaddr + 2 * SUB8 * cb + 512 * t), qf[t],
                                t == 0 ? f32x4{} : s[cb]);
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) s[cb] *= p.c;
      if (need_mask) {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
          for (int i = 0; i < 4; ++i) s[cb][i] = kv0 + 16 * cb + 4 * sg + i < lim ? s[cb][i] : ninf();
      }
      float mx = s[0][0];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int i = (cb == 0 ? 1 : 0); i < 4; ++i) mx = fmaxf(mx, s[cb][i]);
      mx = max_xor32(max_xor16(mx));
      const float mnew = fmaxf(m, mx);
      const float msafe = mnew == ninf() ? 0.f : mnew;  // a row that has seen no key yet
      const float alpha = __builtin_amdgcn_exp2f(m - msafe);
      m = mnew;
      lsum *= alpha;
      if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {  // (x 1.0 is exact: the same bits either way)
#pragma unroll
        for (int e = 0; e < NE; ++e) acc[e] *= alpha;
      }
      // l takes the fp32 exponentials, P their rounding to T
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float ex = __builtin_amdgcn_exp2f(s[cb][i] - msafe);
          pf[cb >> 1][4 * (cb & 1) + i] = (T)ex;
          lsum += ex;
        }
      // O^T += C[:, :512]^T . P^T
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
          const int base = 4 * SUB8 * u + 512 * (e >> 1) + vaddr[e & 1];
          const tx4 lo = __builtin_bit_cast(tx4, lds_read_tr(cur, base));
          const tx4 hi = __builtin_bit_cast(tx4, lds_read_tr(cur, base + 2 * SUB8));
          const tx8 vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          acc[e] = Elem<T>::mfma(vf, pf[u], acc[e]);
        }
      }
    } else {
      // the wave's 16-key slice: keys kv0 + 16 wave + 4 sg + i
      const char* mine = cur + 2 * SUB8 * wave;
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < NTQ; ++t)
        s = Elem<T>::mfma(*reinterpret_cast<const tx8*>(mine + kaddr + 512 * t), qf[t], s);
      s *= p.c;
      if (need_mask) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = kv0 + 16 * wave + 4 * sg + i < lim ? s[i] : ninf();
      }
      float mx = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
      mx = max_xor32(max_xor16(mx));
      const float mnew = fmaxf(m, mx);
      const float msafe = mnew == ninf() ? 0.f : mnew;
      const float alpha = __builtin_amdgcn_exp2f(m - msafe);
      m = mnew;
      lsum *= alpha;
      if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
#pragma unroll
        for (int e = 0; e < NE; ++e) acc[e] *= alpha;
      }
      // the MFMA contracts over 32 keys: the slice's 16 and 16 zeros, in both operands
      pf[0] = tx8{};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float ex = __builtin_amdgcn_exp2f(s[i] - msafe);
        pf[0][i] = (T)ex;
        lsum += ex;
      }
      const tx4 zero = tx4{};
#pragma unroll
      for (int e = 0; e < NE; ++e) {
        const tx4 lo = __builtin_bit_cast(tx4, lds_read_tr(mine, 512 * (e >> 1) + vaddr[e & 1]));
        const tx8 vf = __builtin_shufflevector(lo, zero, 0, 1, 2, 3, 4, 5, 6, 7);
        acc[e] = Elem<T>::mfma(vf, pf[0], acc[e]);
      }
    }
    if constexpr (PAGED) {
      pgn = __builtin_amdgcn_readfirstlane(pgf);
      rn = rf;
    }
  }

  const bool split = ns > 1;
  const size_t slot = (size_t)unit * ns + piece;
  const __amdgpu_buffer_rsrc_t rso =
      make_rsrc(p.ws_o ? p.ws_o + slot * RW * HDIM : nullptr, split ? RW * HDIM * 4 : 0);
  const __amdgpu_buffer_rsrc_t rsl = make_rsrc(p.ws_lse ? p.ws_lse + slot * RW : nullptr, split ? RW * 4 : 0);
  float* lse_out = p.lse ? p.lse + qrow + row0 : nullptr;

  if constexpr (WIDE) {
    // the wave's rows are its own over the whole piece: normalise and store
    const float L = sum_xor32(sum_xor16(lsum));
    const float inv = L > 0.f ? 1.0f / L : 0.f;
    const float lse2 = L > 0.f ? m + __builtin_log2f(L) : ninf();
    const int row = 16 * wave + r16;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const f32x4 o = acc[e] * inv;
      if (split) {
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rso,
                                               (row * HDIM + 16 * e + 4 * g) * 4, 0, 16);
      } else {
        tx4 out;
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = (T)o[j];
        buf_store8(ro, row * OROW + (16 * e + 4 * g) * 2, __builtin_bit_cast(f16x4, out));
      }
    }
    if (g == 0) {
      if (split)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, lse2), rsl, row * 4, 0, 16);
      else if (lse_out && row < nrows)
        lse_out[row] = lse2 * 0.6931471805599453f;
    }
  } else {
    // merge the four waves' partials through LDS (wave order: deterministic)
    constexpr int ML_OFF = 4 * NE * 1024, EW = NE / 4;
    __syncthreads();  // every wave is done with the images
#pragma unroll
    for (int e = 0; e < NE; ++e)
      *reinterpret_cast<f32x4*>(smem + ((wave * NE + e) * 64 + lane) * 16) = acc[e];
    *reinterpret_cast<float2*>(smem + ML_OFF + (wave * 64 + lane) * 8) =
        float2{m, sum_xor32(sum_xor16(lsum))};
    __syncthreads();
    float mw[4], lw[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float2 ml = *reinterpret_cast<const float2*>(smem + ML_OFF + (w * 64 + lane) * 8);
      mw[w] = ml.x;
      lw[w] = ml.y;
    }
    const float M = fmaxf(fmaxf(mw[0], mw[1]), fmaxf(mw[2], mw[3]));
    float L = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      mw[w] = M == ninf() ? 0.f : __builtin_amdgcn_exp2f(mw[w] - M);  // now the weight
      L = __builtin_fmaf(mw[w], lw[w], L);
    }
    const float inv = L > 0.f ? 1.0f / L : 0.f;
    const float lse2 = L > 0.f ? M + __builtin_log2f(L) : ninf();
    const int row = r16;
#pragma unroll
    for (int ee = 0; ee < EW; ++ee) {
      const int e = wave * EW + ee;
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(smem + ((w * NE + e) * 64 + lane) * 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = __builtin_fmaf(mw[w], a[j], o[j]);
      }
      o *= inv;
      if (split) {
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rso,
                                               (row * HDIM + 16 * e + 4 * g) * 4, 0, 16);
      } else {
        tx4 out;
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = (T)o[j];
        buf_store8(ro, row * OROW + (16 * e + 4 * g) * 2, __builtin_bit_cast(f16x4, out));
      }
    }
    if (wave == 0 && g == 0) {
      if (split)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, lse2), rsl, row * 4, 0, 16);
      else if (lse_out && row < nrows)
        lse_out[row] = lse2 * 0.6931471805599453f;
    }
  }
  if (!split) return;

  // hand the piece to the last arriver (the decode kernel's protocol: sc1
  // stores, vmcnt(0) + barrier, one lane's agent-scope add, sc1 loads by the
  // workgroup whose add came last, which merges the pieces in piece order)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  volatile int* last = reinterpret_cast<volatile int*>(smem);
  if (tid == 0) {
    const unsigned old = __hip_atomic_fetch_add(p.ws_ctr + unit, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    *last = old == (unsigned)(ns - 1) ? 1 : 0;
  }
  __syncthreads();
  if (!*last) return;
  decode_merge_pieces<T, HDIM, NB>(p, unit, ns, ro, lse_out, row0, tid);
  if (tid == 0) __hip_atomic_store(p.ws_ctr + unit, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace fa
