// MLA sparse attention for gfx950 (DeepSeek-V3.2's DSA): the weight-absorbed
// 576/512 attention of fa_mla_decode_kernel.hpp where every query token names
// the latent rows it attends to,
//   s[n,h,i]  = softmax_scale * sum_{d<576} q[n,h,d] ckv[idx[n,i], d]
//   O[n,h,:]  = sum_i softmax_i(s[n,h,.]) ckv[idx[n,i], 0:512]
// idx = indices [N][topk], flat rows of a pool [num_rows][576]; an entry
// outside [0, num_rows) is a hole: no byte is read for it and it carries no
// weight.  There is no prefix, no length and no causal flag.
//
// Decomposition.  A workgroup = (query token, row group of its heads, piece of
// its list), four waves; tokens never share a tile (their lists differ), the
// row groups of one token gather the same rows.  The list's 64-entry tiles are
// cut into num_splits pieces with the decode plan, hand-off and workspace.
// The two regimes, the two 72-KB swizzled images, the one barrier per tile,
// both MFMA contractions off one image and the online softmax are
// fa_mla_decode_kernel.hpp's; what is this kernel's own:
//
// Gather.  The image is filled by the same eighteen 1-KB LDS-DMA pieces per
// wave, lane = (subtile, row, slot), but each of a piece's eight rows comes
// from its own pool row.  A pool passes 4 GiB (num_rows * 1152 B), which no
// buffer descriptor with a 32-bit lane offset spans, so the DMA is the global
// form, global_load_lds_dwordx4 with a 64-bit address per lane:
//   ckv + idx * 1152 + the lane's chunk un-XORed + 128 * (piece % 9).
// A lane whose row is a hole takes no part in the loads (EXEC) and writes
// zeros to its 16 B of each piece instead: P = 0 against stale LDS bytes would
// be NaN in the PV product.  A tile of holes only is neither fetched nor
// computed.
//
// Index pipeline.  Tile t + 1's DMA is issued while tile t is computed, so
// tile t + 2's 64 entries are fetched then (one vector load, lane = entry,
// clamped to the token's list and to the piece) and digested at the end of the
// iteration, on the wait the DMA needs anyway: a ballot of (unsigned) idx <
// num_rows is the tile's wave-uniform validity mask, two ds_bpermutes hand
// each DMA lane the entries of its two rows.  The mask is the score mask (key
// 16 cb + 4 sg + i of S^T is bit 16 cb + 4 sg + i), applied only on tiles whose
// mask is not all ones.
#pragma once

#include "fa_mla_decode_kernel.hpp"

namespace fa {

// DecodeParams with k = the pool, hkv = 1, sq = 1, group = rows = hq, cap =
// topk, batch = tokens; kv_lens, causal and v are not looked at.
struct MlaSparseParams : DecodeParams {
  const int* indices;  // device int32 [N][topk]
  int topk;
  int num_rows;        // pool rows: an entry outside [0, num_rows) is a hole
};

// LDS-DMA with a 64-bit address per lane: 16 B from `src` to LDS byte `lds`
// + 16 * lane (`lds` wave-uniform, in M0).  Inline asm for buf_load16_lds's
// reasons (fa_fwd_kernel.hpp): completion is waited for explicitly.
__device__ __forceinline__ void glb_load16_lds(const char* src, unsigned lds) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %1\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %2, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "s"(lds), "v"(src)
      : "memory");
}

template <class T, bool WIDE>
__global__ __launch_bounds__(256, 1) void fa_mla_sparse_kernel(MlaSparseParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NB = WIDE ? 4 : 1;   // 16-row blocks per workgroup
  constexpr int RW = 16 * NB;        // query rows (heads) per workgroup
  constexpr int NTQ = kMlaDqk / 32;  // 32-wide k-steps of QK^T
  constexpr int NE = kMlaDv / 16;    // 16-wide d-blocks of O
  constexpr int HDIM = kMlaDv;
  constexpr int QROW = kMlaRow, OROW = 2 * kMlaDv;
  constexpr int SUB8 = kMlaSub8;
  typedef typename Elem<T>::x8 tx8;
  typedef typename Elem<T>::x4 tx4;
  typedef unsigned long long u64;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  const int sg = ((g & 1) << 1) | (g >> 1);

  // workgroup -> (token, row group, piece)
  const int ns = p.num_splits;
  const unsigned unit = blockIdx.x / (unsigned)ns;
  const int piece = (int)(blockIdx.x - unit * (unsigned)ns);
  const int rg = (int)(unit % (unsigned)p.rgroups);
  const int n = (int)(unit / (unsigned)p.rgroups);
  const int ntiles = (int)(((long long)p.topk + 63) >> 6);
  const int t0 = (int)((long long)ntiles * piece / ns);
  const int t1 = (int)((long long)ntiles * (piece + 1) / ns);

  const int row0 = rg * RW;
  const size_t qrow = (size_t)n * p.hq;  // [N*Hq] row of head 0
  const int nrows = __builtin_amdgcn_readfirstlane(max(0, min(RW, p.rows - row0)));
  const __amdgpu_buffer_rsrc_t rq =
      make_rsrc(static_cast<const char*>(p.q) + (qrow + row0) * QROW, nrows * QROW);
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(static_cast<char*>(p.o) + (qrow + row0) * OROW, nrows * OROW);

  // Q fragments (B operand) of this wave's row block: qf[t] = Q[16 blk + r16][32 t + 8 g .. +7];
  // heads past the group's last read as zeros
  const int blk = WIDE ? wave : 0;
  tx8 qf[NTQ];
#pragma unroll
  for (int t = 0; t < NTQ; ++t)
    qf[t] = __builtin_bit_cast(tx8, buf_load16(rq, (16 * blk + r16) * QROW + (4 * t + g) * 16));

  // The token's list.  fetch(tl): entry 64 tl + lane of it, a hole (-1) past
  // its end or past the piece; the address is 64-bit (topk is any int).
  const int* list = p.indices + (size_t)n * (size_t)p.topk;
  auto fetch = [&](int tl) {
    const long long e = 64ll * tl + lane;
    return tl < t1 && e < (long long)p.topk ? list[e] : -1;
  };
  // LDS-DMA lanes: instruction i (0..17) of wave w fills the image's 1-KB piece
  // 18 w + i lane-linearly, 128 B (two subtiles) of the eight tile rows 16 w +
  // 8 (i / 9) + drow; the source chunk is the slot un-XORed: csrc ^ 32 (i / 9)
  // + 128 (i % 9) bytes into the row.
  const int drow = (lane >> 2) & 7;
  const unsigned csrc = 64 * (lane >> 5) + 16 * ((lane & 3) ^ ((lane >> 4) & 1));
  // digest(idx): the tile's validity mask and this lane's two pool rows
  auto digest = [&](int idx, u64& mask, int& ra, int& rb) {
    mask = __builtin_amdgcn_ballot_w64((unsigned)idx < (unsigned)p.num_rows);
    ra = __builtin_amdgcn_ds_bpermute(4 * (16 * wave + drow), idx);
    rb = __builtin_amdgcn_ds_bpermute(4 * (16 * wave + 8 + drow), idx);
  };
  // a digested tile -> image `img`: valid rows by DMA, holes zero-filled (no
  // lane of a hole reads memory); nothing at all for a tile of holes only
  auto issue = [&](u64 mask, int ra, int rb, char* img) {
    if (mask == 0) return;
    const unsigned lds = (unsigned)__builtin_amdgcn_readfirstlane(lds_addr(img)) + 18 * 1024 * (unsigned)wave;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int ri = h ? rb : ra;
      if ((unsigned)ri < (unsigned)p.num_rows) {
        const char* src = static_cast<const char*>(p.k) + (size_t)ri * QROW + (csrc ^ (32u * h));
#pragma unroll
        for (int j = 0; j < 9; ++j) glb_load16_lds(src + 128 * j, lds + 1024 * (9 * h + j));
      } else {
#pragma unroll
        for (int j = 0; j < 9; ++j)
          *reinterpret_cast<u32x4*>(img + (18 * wave + 9 * h + j) * 1024 + 16 * lane) = u32x4{0u, 0u, 0u, 0u};
      }
    }
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
    char* cur = smem + ((tl - t0) & 1) * kMlaTile;
    // this wave's pieces of tile tl have landed; after the barrier every
    // wave's have, and every wave is done with the other image (tile tl - 1)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const u64 mask = mask_in;
    int idf = -1;
    if (tl + 1 < t1) {
      issue(mask_nx, ra_nx, rb_nx, smem + ((tl + 1 - t0) & 1) * kMlaTile);
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
        for (int t = 0; t < NTQ; ++t)
#pragma unroll
          for (int cb = 0; cb < 4; ++cb)
            s[cb] = Elem<T>::mfma(*reinterpret_cast<const tx8*>(cur + kaddr + 2 * SUB8 * cb + 512 * t), qf[t],
                                  t == 0 ? f32x4{} : s[cb]);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) s[cb] *= p.c;
        if (need_mask) {
          const u64 lm = mask >> (4 * sg);
#pragma unroll
          for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int i = 0; i < 4; ++i) s[cb][i] = (lm >> (16 * cb + i)) & 1 ? s[cb][i] : ninf();
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
        // the wave's 16-key slice: entries 64 tl + 16 wave + 4 sg + i
        const char* mine = cur + 2 * SUB8 * wave;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NTQ; ++t)
          s = Elem<T>::mfma(*reinterpret_cast<const tx8*>(mine + kaddr + 512 * t), qf[t], s);
        s *= p.c;
        if (need_mask) {
          const unsigned lm = (unsigned)(mask >> (16 * wave + 4 * sg));
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
        const tx4 zero = tx4{};
#pragma unroll
        for (int e = 0; e < NE; ++e) {
          const tx4 lo = __builtin_bit_cast(tx4, lds_read_tr(mine, 512 * (e >> 1) + vaddr[e & 1]));
          const tx8 vf = __builtin_shufflevector(lo, zero, 0, 1, 2, 3, 4, 5, 6, 7);
          acc[e] = Elem<T>::mfma(vf, pf[0], acc[e]);
        }
      }
    }
    // tile tl + 2's entries, on the wait tile tl + 1's DMA needs anyway
    digest(idf, mask_nx, ra_nx, rb_nx);
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
      // now the weight; a wave whose slices were all holes has m = -inf and weighs nothing
      mw[w] = M == ninf() ? 0.f : __builtin_amdgcn_exp2f(mw[w] - M);
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
