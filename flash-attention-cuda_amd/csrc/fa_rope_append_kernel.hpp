// Fused rotary position embedding + cache append for gfx950: rotate the new K
// rows between the load and the store of the cache append
// (fa_cache_append_kernel.hpp), rotate the new Q rows in the same launch, and
// let the FP8 quantisation follow in registers.
//
//   n_b as the append defines it; for t in [0, n_b):
//     pos = kv_lens[b] - n_b + t                 (the cache row the append writes)
//     pairs (a, b), i in [0, R/2):
//       interleaved == 0 (NeoX / rotate_half):  a = x[i],  b = x[i + R/2]
//       interleaved == 1 (GPT-J):               a = x[2i], b = x[2i + 1]
//     c = cos[pos][i], s = sin[pos][i]           (fp32 tables [rope_len][R/2])
//     a' = a c - b s,  b' = b c + a s            each product and each sum one
//                                                IEEE fp32 operation (no fma),
//                                                then ONE rounding to T (RNE)
//     elements at or past R: bit copies
//   K: the rounded 16-bit row is what the append's contract stores (16-bit: as
//      it is; FP8: the reciprocal contract applied to the rounded value), so
//      fused == "rotate, then fa_cache_append_*" byte for byte.  V: unchanged.
//   Q: row t of every query head, same pos, to q_out (may be q: a wave owns
//      whole rows and loads them before it stores them).
//   A K/V row is written iff the append's rule holds AND pos < rope_len; a Q
//   row iff 0 <= pos < rope_len.  No table row outside [0, rope_len) is read.
//
// Lane map: the append's.  A lane holds one 16-byte piece (8 elements) of a
// row, HDIM / 8 lanes per row, kAppendU wave instructions per tensor in
// flight, row loads and stores nontemporal.  The rotated pieces are the first
// R / 8 of a row.  Interleaved pairs sit inside a lane (4 per piece).  NeoX
// pairs sit R / 16 lanes apart in the same row: the partner's piece comes by
// ds_bpermute (four dwords), executed by every lane of the wave outside any
// divergent branch; both lanes of a pair belong to one row, so they are
// written or dropped together.  Loads stand in front of no divergent branch
// either: a row that will not be written is loaded from the nearest token and
// table row that exist (clamped, so nothing outside the tensors or outside
// table rows [0, rope_len) is read) and only its store is skipped -- with a
// branch per load the compiler waits for the first rows before it issues the
// last ones (319 -> 313 us on the prefill append).
// R and `interleaved` are launch parameters: their branches are wave-uniform.
// The cos / sin rows are the same for every head of a token: a workgroup loads
// them once per batch element and keeps them in registers over its head slots
// (four per workgroup when the launch is large enough, fa_rope_append_host.hpp:
// with one slot each the table loads, two to four per row piece, hold the
// vector memory pipe at 82 % of the copy rate; with four, 92 %).  Plain loads
// (no nontemporal hint: other workgroups re-read the rows), 16-byte pieces, so
// the tables must be 16-byte aligned.
//
// Grid: x = token blocks (VARLEN: virtual block ids, fa_varlen_map.hpp), y over
// head SLOTS: [0, kvs) the K/V heads, [kvs, kvs + hq) the query heads (strided,
// so the sum may exceed the grid limit), z over the batch (strided; VARLEN:
// none).  kvs is hkv, or 0 when no cache row exists (capacity 0).
// No LDS, no scratch.
#pragma once

#include "fa_cache_append_kernel.hpp"

namespace fa {

struct RopeAppendParams {
  AppendParams a;    // the append's own
  const void* q;     // [B][Hq][Sn][D], or packed [T][Hq][D]; 16-bit
  void* q_out;       // the same shape; may be q
  const float* cos;  // [rope_len][R / 2]
  const float* sin;
  int hq, kvs;       // query heads; K/V head slots of the grid (hkv or 0)
  int rope_len, rdim, interleaved;
};

// The wave-uniform facts of the rotation and this lane's place in it.
struct RopeLane {
  int half;    // R / 2: floats per table row
  int col;     // this lane's first table column
  int src;     // ds_bpermute byte address of the NeoX partner lane (own lane when not rotated)
  bool rot;    // this lane's piece lies below R
  bool hi;     // NeoX: this lane holds the b halves
  bool inter;  // wave-uniform
};

// The table entries one lane needs for one row: NeoX 8 cos + 8 sin (columns
// col .. col + 7), interleaved 4 + 4 (c[0], s[0] only).
struct RopeCS {
  f32x4 c[2], s[2];
};

// Every lane loads (no divergent branch in front of a load: the compiler then
// keeps all of a wave's loads in flight): `pos` is clamped into the table by
// the caller and a lane that does not rotate reads columns 0 .. 7, which every
// table has (R / 2 >= 8).
__device__ __forceinline__ RopeCS rope_load_cs(const RopeAppendParams& p, const RopeLane& L, int pos) {
  RopeCS t;
  const size_t off = (size_t)pos * L.half + (L.rot ? L.col : 0);
  t.c[0] = *reinterpret_cast<const f32x4*>(p.cos + off);
  t.s[0] = *reinterpret_cast<const f32x4*>(p.sin + off);
  if (!L.inter) {
    t.c[1] = *reinterpret_cast<const f32x4*>(p.cos + off + 4);
    t.s[1] = *reinterpret_cast<const f32x4*>(p.sin + off + 4);
  } else {
    t.c[1] = t.s[1] = f32x4{0, 0, 0, 0};
  }
  return t;
}

// One piece rotated.  Called by every lane of the wave (the NeoX exchange
// needs the partner lane active); lanes with !L.rot get their piece back.
template <class E>
__device__ __forceinline__ u32x4 rope_rotate(u32x4 raw, const RopeCS& t, const RopeLane& L) {
#pragma clang fp contract(off)
  typedef typename Elem<E>::x8 ex8;
  const ex8 x = __builtin_bit_cast(ex8, raw);
  ex8 y = x;
  if (L.inter) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = (float)x[2 * j], b = (float)x[2 * j + 1];
      const float c = t.c[0][j], s = t.s[0][j];
      const float ac = a * c, bs = b * s, bc = b * c, as = a * s;
      y[2 * j] = (E)(ac - bs);
      y[2 * j + 1] = (E)(bc + as);
    }
  } else {
    u32x4 praw;
#pragma unroll
    for (int j = 0; j < 4; ++j) praw[j] = (unsigned)__builtin_amdgcn_ds_bpermute(L.src, (int)raw[j]);
    const ex8 o = __builtin_bit_cast(ex8, praw);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float c = t.c[e >> 2][e & 3], s = t.s[e >> 2][e & 3];
      const float xc = (float)x[e] * c, os = (float)o[e] * s;
      // lo lane: a c - b s; hi lane: b c + a s (x - y is x + (-y), bit for bit)
      y[e] = (E)(xc + (L.hi ? os : -os));
    }
  }
  return L.rot ? __builtin_bit_cast(u32x4, y) : raw;
}

// T as for fa_cache_append_kernel, but always the element type (f16 or __bf16,
// or PackedSrc<> of one): a 16-bit cache is no longer a bit copy.
template <class T, int HDIM, bool PAGED, bool KV8>
__global__ __launch_bounds__(256) void fa_rope_append_kernel(RopeAppendParams rp) {
  constexpr bool VARLEN = AppendSrc<T>::packed;
  using E = typename AppendSrc<T>::elem;
  constexpr int LPR = HDIM / 8;         // lanes per row
  constexpr int RPW = 64 / LPR;         // rows per wave instruction
  constexpr int WROWS = kAppendU * RPW; // consecutive tokens of one wave (16 or 32)
  constexpr int SROW = 2 * HDIM;        // source row bytes
  constexpr int CROW = KV8 ? HDIM : 2 * HDIM;  // cache row bytes
  constexpr int CPIECE = KV8 ? 8 : 16;  // bytes a lane stores
  static_assert(WROWS <= 64, "a wave's rows must fit one minimal page");
  const AppendParams& p = rp.a;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane / LPR, piece = lane % LPR;
  RopeLane L;
  {
    const int h16 = rp.rdim >> 4;  // pieces per half
    L.half = rp.rdim >> 1;
    L.inter = rp.interleaved != 0;
    L.rot = piece < 2 * h16;
    L.hi = piece >= h16;
    L.col = L.inter ? 4 * piece : 8 * (piece - (L.hi ? h16 : 0));
    L.src = 4 * (L.rot && !L.inter ? (L.hi ? lane - h16 : lane + h16) : lane);
  }
  [[maybe_unused]] int vb = 0, seq0 = 0, seqn = 0, vr = 0;
  if constexpr (VARLEN) {
    if (!varlen_block<4 * WROWS>(p.new_lens, p.batch, p.sn, (int)blockIdx.x, vb, seq0, seqn, vr)) return;
    vb = __builtin_amdgcn_readfirstlane(vb);
    seq0 = __builtin_amdgcn_readfirstlane(seq0);
    seqn = __builtin_amdgcn_readfirstlane(seqn);
    vr = __builtin_amdgcn_readfirstlane(vr);
  }
  // the wave's first token
  const long long tw = (VARLEN ? (long long)vr : (long long)blockIdx.x) * (4 * WROWS) + wave * WROWS;
  const int slots = rp.kvs + rp.hq;

  // One pass per batch element (VARLEN: the one sequence of this workgroup):
  // the positions, and so the table rows, are the same for every head, so they
  // are loaded once and kept in registers while the workgroup's head slots
  // (blockIdx.y, + gridDim.y, ...) go by.
  for (int b = VARLEN ? vb : (int)blockIdx.z; VARLEN ? b == vb : b < p.batch;
       b += VARLEN ? 1u : gridDim.z) {
    int len = p.kv_lens[b], n = p.sn;
    if constexpr (VARLEN) {
      n = seqn;  // already in [0, sn - seq0]
    } else {
      if (p.new_lens) n = p.new_lens[b];
    }
    len = __builtin_amdgcn_readfirstlane(len);
    n = __builtin_amdgcn_readfirstlane(min(max(n, 0), p.sn));
    if (tw >= n) continue;
    // position (= cache row) of the wave's first token; its rows are rb .. rb + WROWS - 1
    const long long rb = (long long)len - n + tw;
    if (rb + WROWS <= 0 || rb >= rp.rope_len) continue;  // no position has a table row
    const int r0 = (int)rb + lr, t0 = (int)tw + lr;      // rb > -WROWS and < rope_len, tw < sn: ints

    // K/V: whether any of the wave's rows exists, their page pair and which are written
    const bool kvrows = rb < p.cap;
    bool okk[kAppendU];
    [[maybe_unused]] int id0 = 0, id1 = 0, edge = 0, base0 = 0;
    if constexpr (PAGED) {
      if (kvrows && (int)blockIdx.y < rp.kvs) {
        const int pg = (int)max(rb, 0LL) / p.page_size;
        const int* row = p.table + (size_t)b * p.max_pages;
        id0 = row[pg];
        id1 = row[min(pg + 1, p.max_pages - 1)];
        id0 = __builtin_amdgcn_readfirstlane(id0);
        id1 = pg + 1 < p.max_pages ? __builtin_amdgcn_readfirstlane(id1) : -1;
        base0 = pg * p.page_size;
        edge = base0 + p.page_size;
      }
    }
    // loads without a branch: a row that is not written is loaded from the
    // nearest token and position that exist (tw < n, so n >= 1) and dropped
    bool okq[kAppendU];
    int tc[kAppendU];
    RopeCS cs[kAppendU];
#pragma unroll
    for (int u = 0; u < kAppendU; ++u) {
      const int t = t0 + u * RPW, r = r0 + u * RPW;
      okq[u] = t < n && r >= 0 && r < rp.rope_len;
      tc[u] = min(t, n - 1);
      cs[u] = rope_load_cs(rp, L, min(max(r, 0), rp.rope_len - 1));
    }
#pragma unroll
    for (int u = 0; u < kAppendU; ++u) {
      const int r = r0 + u * RPW;
      okk[u] = okq[u] && r < p.cap;
      if constexpr (PAGED) {
        const int id = r < edge ? id0 : id1;
        okk[u] = okk[u] && id >= 0 && id < p.num_pages;
      }
    }

#pragma clang loop unroll(disable)
    for (int hs = blockIdx.y; hs < slots; hs += gridDim.y) {
      const bool isq = hs >= rp.kvs;  // workgroup-uniform
      const int hk = isq ? hs - rp.kvs : hs;
      if (isq) {
        // ---- a query head: rotate rows t0 + u RPW of q into q_out
        const size_t qstr = VARLEN ? (size_t)rp.hq * SROW : (size_t)SROW;
        // token 0 of this (sequence, head)
        const size_t qoff = VARLEN ? ((size_t)seq0 * rp.hq + hk) * SROW + piece * 16
                                   : ((size_t)b * rp.hq + hk) * p.sn * SROW + piece * 16;
        const char* qs = static_cast<const char*>(rp.q) + qoff;
        char* qd = static_cast<char*>(rp.q_out) + qoff;
        u32x4 qx[kAppendU];
#pragma unroll
        for (int u = 0; u < kAppendU; ++u)
          qx[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(qs + (size_t)tc[u] * qstr));
#pragma unroll
        for (int u = 0; u < kAppendU; ++u) {
          const u32x4 y = rope_rotate<E>(qx[u], cs[u], L);  // every lane: the exchange
          if (okq[u])
            __builtin_nontemporal_store(y, reinterpret_cast<u32x4*>(qd + (size_t)(t0 + u * RPW) * qstr));
        }
        continue;
      }

      // ---- a K/V head: the append, with K rotated between load and store
      if (!kvrows) continue;  // none of the rows exists
      const size_t sstr = VARLEN ? (size_t)p.hkv * SROW : (size_t)SROW;
      [[maybe_unused]] float krcp = 1.0f, vrcp = 1.0f;
      if constexpr (KV8) {
        float ksc = 1.0f, vsc = 1.0f;
        if (p.k_scale) ksc = p.k_scale[hk];
        if (p.v_scale) vsc = p.v_scale[hk];
        krcp = __builtin_bit_cast(
            float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, 1.0f / ksc)));
        vrcp = __builtin_bit_cast(
            float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, 1.0f / vsc)));
      }
      const size_t bh = (size_t)b * p.hkv + hk;
      // token 0 of this (sequence, head)
      const size_t soff = VARLEN ? ((size_t)seq0 * p.hkv + hk) * SROW + piece * 16
                                 : bh * p.sn * SROW + piece * 16;
      const char* ks = static_cast<const char*>(p.k_new) + soff;
      const char* vs = static_cast<const char*>(p.v_new) + soff;
      u32x4 kx[kAppendU], vx[kAppendU];
#pragma unroll
      for (int u = 0; u < kAppendU; ++u) {
        const size_t so = (size_t)tc[u] * sstr;
        kx[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ks + so));
        vx[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(vs + so));
      }
#pragma unroll
      for (int u = 0; u < kAppendU; ++u) {
        const u32x4 ky = rope_rotate<E>(kx[u], cs[u], L);  // every lane: the exchange
        if (!okk[u]) continue;
        const int r = r0 + u * RPW;
        size_t doff;
        if constexpr (PAGED) {
          const bool lo = r < edge;
          doff = (size_t)(lo ? id0 : id1) * p.page_bytes + (size_t)hk * p.head_bytes +
                 (size_t)(r - (lo ? base0 : edge)) * CROW + piece * CPIECE;
        } else {
          doff = (bh * p.cap + r) * CROW + piece * CPIECE;
        }
        char* kd = static_cast<char*>(p.k_cache) + doff;
        char* vd = static_cast<char*>(p.v_cache) + doff;
        if constexpr (KV8) {
          __builtin_nontemporal_store(append_cvt_fp8x8<E>(ky, krcp), reinterpret_cast<u32x2*>(kd));
          __builtin_nontemporal_store(append_cvt_fp8x8<E>(vx[u], vrcp), reinterpret_cast<u32x2*>(vd));
        } else {
          __builtin_nontemporal_store(ky, reinterpret_cast<u32x4*>(kd));
          __builtin_nontemporal_store(vx[u], reinterpret_cast<u32x4*>(vd));
        }
      }
    }
  }
}

}  // namespace fa
