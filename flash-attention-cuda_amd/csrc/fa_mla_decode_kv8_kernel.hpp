// MLA decode over an FP8 (E4M3) latent cache for gfx950: the contract and the
// decomposition of fa_mla_decode_kernel.hpp -- workgroup = (batch, row group,
// key piece), four waves, WIDE (rows > 16: wave w owns 16-row block w) and
// narrow (rows <= 16: the waves split a tile's keys and merge once through
// LDS), the decode plan, hand-off and workspace -- over a cache of bytes,
//   c[j, d] = ckv_scale * float(E4M3 byte ckv8[b][j][d]),   d < 576.
// The scale never meets a byte: it is folded into the score scale (and so into
// the LSE) and into the final 1 / l, as fa_decode_kernel.hpp folds k_scale and
// v_scale.  Q, P and the MFMAs stay 16-bit; E4M3 -> f16 / bf16 is exact.
//
// One fetch of raw bytes.  A 64-key tile is 64 x 576 B = 36 KB, contiguous in
// memory.  It goes HBM -> LDS by LDS-DMA once, as bytes, and both contractions
// convert in registers on the way into the MFMA.
//
// The image (1-byte elements).  A 16-key block is 9216 B = nine 1-KB pieces,
// piece i = the i-th 128-B line of each of the block's eight row PAIRS (a row
// pair, 1152 B = 9 lines, starts on a line; a single 576-B row does not).  With
// p = (row >> 1) & 7 and m = 36 (row & 1) + ch the chunk's index in its pair,
//   off(row, ch) = 9216 (row >> 4) + 1024 (m >> 3) + 128 p + 16 ((m & 7) ^ (p >> 1)).
// A DMA instruction's lane-linear destination is one piece: lane l = 8 p + slot
// fetches chunk (slot ^ (p >> 1)) of line i of pair p, eight whole lines per
// instruction.  off mod 256 = 128 (p & 1) + 16 ((ch & 7) ^ (p >> 1) ^ 4 (row & 1)):
// sixteen rows that differ mod 16 land, for any fixed ch, in the sixteen 16-B
// slots of a 256-B bank row.  Both reads are of that kind:
//   S^T = C . Q^T   one ds_read_b128 per lane and PAIR of k-steps: chunk 4 tt +
//     g of the lane's key is dims 64 tt + 16 g .. +15, bytes 0..7 feed k-step
//     2 tt and bytes 8..15 k-step 2 tt + 1, and Q's fragments are loaded under
//     the same permutation of d (the sum over d has no order; nine LDS reads
//     per key block where a ds_read_b64 per k-step takes eighteen).  A pass is
//     sixteen lanes = the sixteen rows of a key block.
//   O^T += C[:, :512]^T . P^T   one ds_read_b64_tr_b8 per MFMA.  In a group of
//     sixteen lanes, lanes 2 j and 2 j + 1 address the two 8-B halves of a
//     16-B chunk of row j (j < 8), and lane i receives byte i of the eight
//     rows: dim 16 e + i of eight keys, one whole A operand after cvt_fp8x8.
//     Lane group g takes the keys whose P it holds, S^T rows 4 g .. 4 g + 3 of
//     blocks 2 u and 2 u + 1.  A pass is 32 lanes = two groups = sixteen rows:
//     A-row r of an odd block is key r ^ 8, so that the two groups' rows
//     {0..7} of the even and {8..15} of the odd block differ mod 16.
//
// The queue.  Four 36-KB images (144 KB) form a ring: while tile i is consumed,
// tiles i + 1 .. i + 3 are in flight.  Per tile: a counted wait (a wave issues
// nine DMA instructions per tile, so vmcnt(18) leaves two tiles flying; 9 and 0
// in the last two iterations), ONE barrier, which publishes tile i and retires
// tile i - 1 in every wave, then the issue of tile i + 3 into tile i - 1's
// image.  Page ids (paged) are scalar loads: they count in lgkmcnt and never
// touch the DMA queue's vmcnt.  The narrow merge (130 KB) reuses the ring.
#pragma once

#include "fa_mla_decode_kernel.hpp"

namespace fa {

constexpr int kMla8Row = kMlaDqk;            // bytes per latent row
constexpr int kMla8Blk = 16 * kMla8Row;      // a 16-key block, in memory and in the image
constexpr int kMla8Tile = 4 * kMla8Blk;      // one 64-key tile image
constexpr int kMla8Ring = 4;                 // images: one consumed, three in flight
constexpr int kMla8LdsBytes = kMla8Ring * kMla8Tile;

// byte offset of 16-B chunk `ch` (0..35) of row `row` (0..63) in a tile image
__device__ __forceinline__ int mla8_lds_off(int row, int ch) {
  const int p = (row >> 1) & 7, m = 36 * (row & 1) + ch;
  return kMla8Blk * (row >> 4) + 1024 * (m >> 3) + 128 * p + 16 * ((m & 7) ^ (p >> 1));
}

__device__ __forceinline__ u32x2 lds_read_tr8(const char* base, int off) {
  typedef int i32x2 __attribute__((ext_vector_type(2)));
  typedef __attribute__((address_space(3))) i32x2 lds_i32x2;
  return __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2*)(base + off)));
}

// P = DecodeKv8Params (contiguous: k = the cache [B][cap][576] bytes) or
// DecodePagedKv8Params (k = the pool, page_bytes = page_size * 576); k_scale =
// the one ckv_scale (device float[1] or nullptr), v_scale is not looked at;
// hkv = 1, group = hq, c = softmax_scale * log2(e).
template <class T, bool WIDE, bool PAGED = false, class P = DecodeKv8Params>
__global__ __launch_bounds__(256, 1) void fa_mla_decode_kv8_kernel(P p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NB = WIDE ? 4 : 1;   // 16-row blocks per workgroup
  constexpr int RW = 16 * NB;        // query rows per workgroup
  constexpr int NTP = kMlaDqk / 64;  // pairs of 32-wide k-steps of QK^T
  constexpr int NE = kMlaDv / 16;    // 16-wide d-blocks of O
  constexpr int HDIM = kMlaDv;
  constexpr int QROW = 2 * kMlaDqk, OROW = 2 * kMlaDv;
  constexpr int CROW = kMla8Row, BLK = kMla8Blk;
  typedef typename Elem<T>::x8 tx8;
  typedef typename Elem<T>::x4 tx4;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;

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
  const float ksc = p.k_scale ? p.k_scale[0] : 1.0f;
  const float csc = p.c * ksc;

  const int row0 = rg * RW;
  const size_t qrow = (size_t)b * p.hq * p.sq;  // [B*Hq*Sq] row of r = 0
  const int nrows = __builtin_amdgcn_readfirstlane(max(0, min(RW, p.rows - row0)));
  const __amdgpu_buffer_rsrc_t rq =
      make_rsrc(static_cast<const char*>(p.q) + (qrow + row0) * QROW, nrows * QROW);
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(static_cast<char*>(p.o) + (qrow + row0) * OROW, nrows * OROW);
  // contiguous: one descriptor for the element's rows below its length.
  // Paged: one per tile, built in issue()
  [[maybe_unused]] const __amdgpu_buffer_rsrc_t rcontig =
      make_rsrc(static_cast<const char*>(p.k) + (PAGED ? 0 : (size_t)b * (size_t)p.cap * CROW),
                PAGED ? 0 : len * CROW);

  // first key the lane's row does not see; tiles ending past mask_from need the mask
  const int blk = WIDE ? wave : 0;
  const int lim = p.causal ? len - p.sq + 1 + (row0 + 16 * blk + r16) % p.sq : len;
  const int mask_from = p.causal ? len - p.sq + 1 : len;

  // LDS-DMA: instruction i (0..8) of wave w fills piece 9 w + i of the image
  // lane-linearly: lane = (pair p, slot), the source chunk is the slot un-XORed,
  // 16 m into the pair with m = 8 i + chunk.  Row of the chunk: 16 w + 2 p + (m >= 36)
  const int dpair = lane >> 3, dch = (lane & 7) ^ (lane >> 4);
  const unsigned wsrc = (unsigned)wave * BLK + (unsigned)dpair * (2 * CROW) + 16u * dch;
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
                     (64 * r + min(live, 64)) * CROW);
      base = (unsigned)(64 * r) * CROW;
    } else {
      rc = rcontig;
      base = (unsigned)(64 * tl) * CROW;
    }
    if (live < 64) {
#pragma unroll
      for (int i = 0; i < 9; ++i)
        if (16 * wave + 2 * dpair + (8 * i + dch >= 36 ? 1 : 0) >= live)
          *reinterpret_cast<u32x4*>(img + (9 * wave + i) * 1024 + 16 * lane) = u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) buf_load16_lds(rc, img + (9 * wave + i) * 1024, (int)(base + wsrc + 128 * i));
  };

  // Paged: the tile's (pool page, 64-row block in the page).  The id is read
  // through the constant address space (nothing writes the table during the
  // launch), which makes it a scalar load whatever the DMA's asm clobbers: it
  // counts in lgkmcnt and stays out of the DMA queue's vmcnt.  Only entries of
  // tiles below t1 (pages holding a key below len) are read.
  typedef const __attribute__((address_space(4))) int* const_int_p;
  [[maybe_unused]] const_int_p trow = nullptr;
  if constexpr (PAGED) trow = (const_int_p)(uintptr_t)(p.table + (size_t)b * p.max_pages);
  [[maybe_unused]] auto page_of = [&](int tl, int& r) {
    int pg = 0;
    r = 0;
    if constexpr (PAGED) {
      if (tl < t1) {
        const int j = tl / p.tpp;
        r = tl - j * p.tpp;
        pg = trow[j];
      }
    }
    return pg;
  };

  // prologue: tile t0's DMA, the Q fragments (B operand) of this wave's row
  // block, qf[2 tt + h] = Q[16 blk + r16][64 tt + 16 g + 8 h .. +7] (rows past
  // the group's last read as zeros), then tiles t0 + 1 and t0 + 2.  The Q
  // loads are waited for before the later DMAs are issued, so that no wait on
  // them reaches into the queue.
  int rr = 0;
  if (t0 < t1) {
    const int pg = page_of(t0, rr);
    issue(t0, pg, rr, smem);
  }
  tx8 qf[2 * NTP];
#pragma unroll
  for (int t = 0; t < 2 * NTP; ++t)
    qf[t] = __builtin_bit_cast(
        tx8, buf_load16(rq, (16 * blk + r16) * QROW + 128 * (t >> 1) + 32 * g + 16 * (t & 1)));
#pragma unroll
  for (int t = 0; t < 2 * NTP; ++t) asm volatile("" : "+v"(qf[t]));
#pragma unroll
  for (int d = 1; d < kMla8Ring - 1; ++d)
    if (t0 + d < t1) {
      const int pg = page_of(t0 + d, rr);
      issue(t0 + d, pg, rr, smem + d * kMla8Tile);
    }
  [[maybe_unused]] int rn = 0;
  [[maybe_unused]] int pgn = page_of(t0 + kMla8Ring - 1, rn);  // of the tile issued in iteration t0

  // A-operand addresses.  A-row r of key block cb is key 16 cb + (r ^ 8 (cb & 1)).
  // QK^T: chunk 4 tt + g of that row: kaddr[cb & 1][tt & 1] + 512 (tt & ~1).
  // Narrow: the wave's one block, kaddr[0] only
  constexpr int NPAR = WIDE ? 2 : 1;
  int kaddr[NPAR][2];
#pragma unroll
  for (int par = 0; par < NPAR; ++par) {
    const int row = r16 ^ (8 * (WIDE ? par : (wave & 1))), pr = row >> 1, o = row & 1;
    const int base = 128 * pr + 16 * (g ^ (pr >> 1));
    kaddr[par][0] = base + (o ? 4160 : 0);
    kaddr[par][1] = base + (o ? 5120 : 64);
  }
  // PV: lanes 2 j + h of group g address half h of chunk e of the key of P's
  // element j: block (j >> 2) of the pair, A-row 4 g + (j & 3).  Per e & 7,
  // + 1024 (e >> 3).  Narrow: the one block, elements 4..7 are zeros (the
  // lanes re-read elements 0..3 and the words are dropped)
  int vaddr[8];
  {
    const int j = r16 >> 1, h = r16 & 1;
    const int cbp = WIDE ? (j >> 2) : (wave & 1);
    const int row = (4 * g + (j & 3)) ^ (8 * cbp), pr = row >> 1, o = row & 1;
    const int base = (WIDE ? BLK * (j >> 2) : 0) + 128 * pr + 8 * h;
#pragma unroll
    for (int c = 0; c < 8; ++c)
      vaddr[c] = base + 16 * ((c & 3) ^ (pr >> 1)) + (o ? (c < 4 ? 4160 : 5120) : 64 * (c >> 2));
  }

  f32x4 acc[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) acc[e] = f32x4{};
  float m = ninf(), lsum = 0.f;

  for (int tl = t0; tl < t1; ++tl) {
    char* cur = smem + ((tl - t0) & (kMla8Ring - 1)) * kMla8Tile;
    // this wave's pieces of tile tl have landed (the tiles issued after it may
    // still fly); after the barrier every wave's have, and every wave is done
    // with tile tl - 1, whose image tile tl + 3 takes
    const int ahead = t1 - 1 - tl;
    if (ahead >= 2)
      asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
    else if (ahead == 1)
      asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tl + kMla8Ring - 1 < t1) {
      issue(tl + kMla8Ring - 1, pgn, rn, smem + ((tl + kMla8Ring - 1 - t0) & (kMla8Ring - 1)) * kMla8Tile);
      if constexpr (PAGED) pgn = page_of(tl + kMla8Ring, rn);
    }

    const int kv0 = 64 * tl;
    const bool need_mask = kv0 + 64 > mask_from;
    tx8 pf[2];
    if constexpr (WIDE) {
      // S^T = C . Q^T over the tile's four 16-key blocks (four independent chains)
      f32x4 s[4];
#pragma unroll
      for (int tt = 0; tt < NTP; ++tt)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
          const u32x4 kq =
              *reinterpret_cast<const u32x4*>(cur + BLK * cb + kaddr[cb & 1][tt & 1] + 512 * (tt & ~1));
          s[cb] = Elem<T>::mfma(cvt_fp8x8<T>(kq[0], kq[1]), qf[2 * tt], tt == 0 ? f32x4{} : s[cb]);
          s[cb] = Elem<T>::mfma(cvt_fp8x8<T>(kq[2], kq[3]), qf[2 * tt + 1], s[cb]);
        }
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) s[cb] *= csc;
      if (need_mask) {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            s[cb][i] = kv0 + 16 * cb + ((4 * g + i) ^ (8 * (cb & 1))) < lim ? s[cb][i] : ninf();
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
          const u32x2 vq = lds_read_tr8(cur, 2 * BLK * u + vaddr[e & 7] + 1024 * (e >> 3));
          acc[e] = Elem<T>::mfma(cvt_fp8x8<T>(vq[0], vq[1]), pf[u], acc[e]);
        }
      }
    } else {
      // the wave's 16-key slice: S^T row 4 g + i is key kv0 + 16 wave + ((4 g + i) ^ 8 (wave & 1))
      const char* mine = cur + BLK * wave;
      const int par = wave & 1;
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int tt = 0; tt < NTP; ++tt) {
        const u32x4 kq = *reinterpret_cast<const u32x4*>(mine + kaddr[0][tt & 1] + 512 * (tt & ~1));
        s = Elem<T>::mfma(cvt_fp8x8<T>(kq[0], kq[1]), qf[2 * tt], s);
        s = Elem<T>::mfma(cvt_fp8x8<T>(kq[2], kq[3]), qf[2 * tt + 1], s);
      }
      s *= csc;
      if (need_mask) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = kv0 + 16 * wave + ((4 * g + i) ^ (8 * par)) < lim ? s[i] : ninf();
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
#pragma unroll
      for (int e = 0; e < NE; ++e) {
        const u32x2 vq = lds_read_tr8(mine, vaddr[e & 7] + 1024 * (e >> 3));
        acc[e] = Elem<T>::mfma(cvt_fp8x8<T>(vq[0], 0u), pf[0], acc[e]);
      }
    }
  }

  // the value side of the scale joins the normalisation
  const bool split = ns > 1;
  const size_t slot = (size_t)unit * ns + piece;
  const __amdgpu_buffer_rsrc_t rso =
      make_rsrc(p.ws_o ? p.ws_o + slot * RW * HDIM : nullptr, split ? RW * HDIM * 4 : 0);
  const __amdgpu_buffer_rsrc_t rsl = make_rsrc(p.ws_lse ? p.ws_lse + slot * RW : nullptr, split ? RW * 4 : 0);
  float* lse_out = p.lse ? p.lse + qrow + row0 : nullptr;

  if constexpr (WIDE) {
    // the wave's rows are its own over the whole piece: normalise and store
    const float L = sum_xor32(sum_xor16(lsum));
    const float inv = L > 0.f ? ksc / L : 0.f;
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
    static_assert(ML_OFF + 4 * 64 * 8 <= kMla8LdsBytes, "the narrow merge reuses the ring");
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
    const float inv = L > 0.f ? ksc / L : 0.f;
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

  // hand the piece to the last arriver (the 16-bit kernel's protocol)
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
