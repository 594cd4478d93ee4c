// MLA sparse attention over an FP8 (E4M3) latent pool for gfx950 (DeepSeek-V3.2's
// DSA as a server runs it): fa_mla_sparse_kernel.hpp's contract over bytes,
//   c[r, d]   = ckv_scale * float(E4M3 byte ckv8[r][d]),     r < num_rows, d < 576
//   s[n,h,i]  = softmax_scale * sum_{d<576} q[n,h,d] c[idx[n,i], d]
//   O[n,h,:]  = sum_i softmax_i(s[n,h,.]) c[idx[n,i], 0:512]
// idx = indices [N][topk], flat rows of the pool; an entry outside [0, num_rows)
// is a hole: no byte is read for it and it carries no weight.
//
// What it keeps.  From fa_mla_sparse_kernel.hpp: workgroup = (token, row group
// of its heads, piece of its list), WIDE / narrow, the online softmax, the
// ballot of (unsigned) idx < num_rows as the tile's score mask, the index fetch
// two tiles ahead with its ds_bpermute digest, the skip of tiles of holes.
// From fa_mla_decode_kv8_kernel.hpp: the pair-based byte image mla8_lds_off,
// one ds_read_b128 per pair of k-steps of S^T = C . Q^T with Q loaded under the
// same permutation of d, ds_read_b64_tr_b8 for O^T += C[:, :512]^T . P^T with
// A-row r of an odd key block = key r ^ 8, cvt_fp8x8, and the scale folded
// into the score scale and the final 1 / l, never into a byte.  The compute
// half is that kernel's statement for statement, so on a hole-free list the
// result equals fa_mla_decode_kv8 on the gathered rows bit for bit.
//
// What is its own.
//
// Gather into the pair-based image.  Wave w owns key block w of a tile (list
// entries 16 w .. 16 w + 15): nine 1-KB pieces, piece i = line i (128 B) of
// each of the block's eight row pairs.  A pair is two pool rows that are not
// neighbours in memory, and a 576-B row is 4.5 lines: lines 0..3 of a pair are
// its even row's bytes 0..511, line 4 is the even row's last 64 B and the odd
// row's first 64 B, lines 5..8 the odd row's bytes 64..575.  Lane l = 8 p +
// slot of instruction i fetches chunk m = 8 i + (slot ^ (p >> 1)) of pair p:
// row 16 w + 2 p + (m >= 36), byte 16 (m - 36 (m >= 36)) of that pool row.  So a
// lane holds TWO row bases, a = row_even + 16 ch and b = row_odd + 16 ch - 576
// (ch = slot ^ (p >> 1)), the source of piece i is base + 128 i with base = a
// for i < 4, b for i > 4 and, in piece 4, a for the lanes with ch < 4 and b for
// the others: a per-lane choice of the row, which the global LDS-DMA form
// (global_load_lds_dwordx4, a 64-bit address per lane) allows and a buffer
// descriptor does not.  576 = 36 x 16, so every address is 16-byte aligned with
// the pool.  Holes are per row: a lane whose row for piece i is a hole takes no
// part in that load (EXEC) and stores 16 zero bytes in its place -- a stale LDS
// byte may be the NaN code, and 0 x NaN in the PV product is NaN.  In piece 4,
// and in a pair with one hole, lanes of one pair load and zero-fill side by
// side.  A wave whose block is all holes only zero-fills; a tile of holes is
// neither fetched nor computed.
//
// The queue.  The count of DMA instructions a wave issues per tile depends on
// the holes (0..9, and the index fetch is a vector load too), so the kv8 ring's
// counted wait vmcnt(18) has nothing to stand on.  This kernel takes the
// schedule that needs no count: two 36-KB images, vmcnt(0) and ONE barrier per
// tile, tile t + 1 issued behind the barrier while tile t is computed.  A
// deeper ring was not explored (DESIGN.md §3.0y names it as the open item).
// LDS: the two images are 72 KB (WIDE); the narrow kernel's merge through LDS
// needs 130 KB.  The registers allow one workgroup per CU either way.
#pragma once

#include "fa_mla_decode_kv8_kernel.hpp"
#include "fa_mla_sparse_kernel.hpp"

namespace fa {

// MlaSparseParams with k = the pool of bytes and the one ckv_scale (device
// float[1] or nullptr: 1.0)
struct MlaSparseKv8Params : MlaSparseParams {
  const float* k_scale;
};

constexpr int kMlaSparse8Images = 2;
constexpr int kMlaSparse8MergeBytes = 4 * (kMlaDv / 16) * 1024 + 4 * 64 * 8;  // the narrow merge: acc + (m, l)
constexpr int kMlaSparse8LdsWide = kMlaSparse8Images * kMla8Tile;
constexpr int kMlaSparse8LdsNarrow =
    kMlaSparse8MergeBytes > kMlaSparse8LdsWide ? kMlaSparse8MergeBytes : kMlaSparse8LdsWide;

template <class T, bool WIDE>
__global__ __launch_bounds__(256, 1) void fa_mla_sparse_kv8_kernel(MlaSparseKv8Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NB = WIDE ? 4 : 1;   // 16-row blocks per workgroup
  constexpr int RW = 16 * NB;        // query rows (heads) per workgroup
  constexpr int NTP = kMlaDqk / 64;  // pairs of 32-wide k-steps of QK^T
  constexpr int NE = kMlaDv / 16;    // 16-wide d-blocks of O
  constexpr int HDIM = kMlaDv;
  constexpr int QROW = 2 * kMlaDqk, OROW = 2 * kMlaDv;
  constexpr int CROW = kMla8Row, BLK = kMla8Blk;
  typedef typename Elem<T>::x8 tx8;
  typedef typename Elem<T>::x4 tx4;
  typedef unsigned long long u64;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;

  // workgroup -> (token, row group, piece)
  const int ns = p.num_splits;
  const unsigned unit = blockIdx.x / (unsigned)ns;
  const int piece = (int)(blockIdx.x - unit * (unsigned)ns);
  const int rg = (int)(unit % (unsigned)p.rgroups);
  const int n = (int)(unit / (unsigned)p.rgroups);
  const int ntiles = (int)(((long long)p.topk + 63) >> 6);
  const int t0 = (int)((long long)ntiles * piece / ns);
  const int t1 = (int)((long long)ntiles * (piece + 1) / ns);
  const float ksc = p.k_scale ? p.k_scale[0] : 1.0f;
  const float csc = p.c * ksc;

  const int row0 = rg * RW;
  const size_t qrow = (size_t)n * p.hq;  // [N*Hq] row of head 0
  const int nrows = __builtin_amdgcn_readfirstlane(max(0, min(RW, p.rows - row0)));
  const __amdgpu_buffer_rsrc_t rq =
      make_rsrc(static_cast<const char*>(p.q) + (qrow + row0) * QROW, nrows * QROW);
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(static_cast<char*>(p.o) + (qrow + row0) * OROW, nrows * OROW);

  // Q fragments (B operand) of this wave's row block under the image's
  // permutation of d: qf[2 tt + h] = Q[16 blk + r16][64 tt + 16 g + 8 h .. +7];
  // heads past the group's last read as zeros
  const int blk = WIDE ? wave : 0;
  tx8 qf[2 * NTP];
#pragma unroll
  for (int t = 0; t < 2 * NTP; ++t)
    qf[t] = __builtin_bit_cast(
        tx8, buf_load16(rq, (16 * blk + r16) * QROW + 128 * (t >> 1) + 32 * g + 16 * (t & 1)));

  // The token's list.  fetch(tl): entry 64 tl + lane of it, a hole (-1) past
  // its end or past the piece; the address is 64-bit (topk is any int).
  const int* list = p.indices + (size_t)n * (size_t)p.topk;
  auto fetch = [&](int tl) {
    const long long e = 64ll * tl + lane;
    return tl < t1 && e < (long long)p.topk ? list[e] : -1;
  };
  // LDS-DMA lanes: instruction i (0..8) of wave w fills piece 9 w + i of the
  // image lane-linearly; lane = (pair dpair, slot), the chunk is the slot un-XORed
  const int dpair = lane >> 3, dch = (lane & 7) ^ (lane >> 4);
  // digest(idx): the tile's validity mask and the two pool rows of this lane's pair
  auto digest = [&](int idx, u64& mask, int& ra, int& rb) {
    mask = __builtin_amdgcn_ballot_w64((unsigned)idx < (unsigned)p.num_rows);
    ra = __builtin_amdgcn_ds_bpermute(4 * (16 * wave + 2 * dpair), idx);
    rb = __builtin_amdgcn_ds_bpermute(4 * (16 * wave + 2 * dpair + 1), idx);
  };
  // a digested tile -> image `img`: per piece, the lanes whose row is valid load,
  // the others store zeros (no lane of a hole reads memory); nothing at all for
  // a tile of holes only
  const uintptr_t pool = reinterpret_cast<uintptr_t>(p.k) + 16u * (unsigned)dch;
  auto issue = [&](u64 mask, int ra, int rb, char* img) {
    if (mask == 0) return;
    const unsigned lds = (unsigned)__builtin_amdgcn_readfirstlane(lds_addr(img)) + (unsigned)(BLK * wave);
    char* dst = img + BLK * wave + 16 * lane;
    const bool va = (unsigned)ra < (unsigned)p.num_rows, vb = (unsigned)rb < (unsigned)p.num_rows;
    // piece i of the pair comes from base + 128 i: the even row's base for chunks
    // below 36, the odd row's, moved back by the even row's 576 B, for the others
    const uintptr_t a = pool + (uintptr_t)(unsigned)ra * CROW;
    const uintptr_t b = pool + (uintptr_t)(unsigned)rb * CROW - CROW;
    const u32x4 zero = u32x4{0u, 0u, 0u, 0u};
    if (va) {
#pragma unroll
      for (int i = 0; i < 4; ++i) glb_load16_lds(reinterpret_cast<const char*>(a + 128 * i), lds + 1024 * i);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(dst + 1024 * i) = zero;
    }
    // piece 4: chunks 32..35 close the even row, chunks 36..39 open the odd one
    const bool lo = dch < 4;
    if (lo ? va : vb)
      glb_load16_lds(reinterpret_cast<const char*>((lo ? a : b) + 128 * 4), lds + 1024 * 4);
    else
      *reinterpret_cast<u32x4*>(dst + 1024 * 4) = zero;
    if (vb) {
#pragma unroll
      for (int i = 5; i < 9; ++i) glb_load16_lds(reinterpret_cast<const char*>(b + 128 * i), lds + 1024 * i);
    } else {
#pragma unroll
      for (int i = 5; i < 9; ++i) *reinterpret_cast<u32x4*>(dst + 1024 * i) = zero;
    }
  };

  // A-operand addresses (fa_mla_decode_kv8_kernel.hpp's).  A-row r of key block
  // cb is key 16 cb + (r ^ 8 (cb & 1)).  QK^T: chunk 4 tt + g of that row:
  // kaddr[cb & 1][tt & 1] + 512 (tt & ~1).  Narrow: the wave's one block, kaddr[0]
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
  // + 1024 (e >> 3).  Narrow: the one block, elements 4..7 are zeros
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

  // mask_in: the mask of the tile in flight (the next one to compute);
  // (mask_nx, ra_nx, rb_nx): the digest of the tile to issue next
  u64 mask_in = 0, mask_nx = 0;
  int ra_nx = -1, rb_nx = -1;
  if (t0 < t1) {
    const int i0 = fetch(t0), i1 = fetch(t0 + 1);
    digest(i0, mask_in, ra_nx, rb_nx);
    issue(mask_in, ra_nx, rb_nx, smem);
    digest(i1, mask_nx, ra_nx, rb_nx);
  }

  for (int tl = t0; tl < t1; ++tl) {
    char* cur = smem + ((tl - t0) & 1) * kMla8Tile;
    // this wave's pieces of tile tl have landed, however many they were; after
    // the barrier every wave's have and its zero-fills are visible, and every
    // wave is done with the other image (tile tl - 1)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const u64 mask = mask_in;
    int idf = -1;
    if (tl + 1 < t1) {
      issue(mask_nx, ra_nx, rb_nx, smem + ((tl + 1 - t0) & 1) * kMla8Tile);
      mask_in = mask_nx;
      idf = fetch(tl + 2);
    }

    if (mask != 0) {
      const bool need_mask = mask != ~0ull;
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
          // S^T row 4 g + i of block cb is entry 16 cb + ((4 g + i) ^ 8 (cb & 1)) of the tile
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) {
            const unsigned lm = (unsigned)(mask >> (16 * cb + ((4 * g) ^ (8 * (cb & 1)))));
#pragma unroll
            for (int i = 0; i < 4; ++i) s[cb][i] = (lm >> i) & 1 ? s[cb][i] : ninf();
          }
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
        // the wave's 16-key slice: S^T row 4 g + i is entry 16 wave + ((4 g + i) ^ 8 (wave & 1))
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
          const unsigned lm = (unsigned)(mask >> (16 * wave + ((4 * g) ^ (8 * par))));
#pragma unroll
          for (int i = 0; i < 4; ++i) s[i] = (lm >> i) & 1 ? s[i] : ninf();
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
    // tile tl + 2's entries, on the wait tile tl + 1's DMA needs anyway
    digest(idf, mask_nx, ra_nx, rb_nx);
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
    static_assert(ML_OFF + 4 * 64 * 8 <= kMlaSparse8LdsNarrow, "the narrow merge reuses the images");
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
      // now the weight; a wave whose slices were all holes has m = -inf and weighs nothing
      mw[w] = M == ninf() ? 0.f : __builtin_amdgcn_exp2f(mw[w] - M);
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

  // hand the piece to the last arriver (the decode kernel's protocol)
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
