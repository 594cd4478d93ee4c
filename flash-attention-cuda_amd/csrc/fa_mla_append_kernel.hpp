// The writers of the MLA caches for gfx950 (include/fa_mi355x_mla_append.h,
// DESIGN.md §3.0z): the latent append with fused RoPE, into the four latent
// cache forms the MLA readers take, and the quantising writer of the indexer's
// FP8 key pool.
//
// 1. fa_mla_append_kernel
//
//   sequences by fa_varlen_map.hpp (cu_seqlens, or uniform when it is absent);
//   for t in [0, n_b):  pos = kv_lens[b] - n_b + t
//     cache row pos of b <- [c_kv(512) | rope(k_pe)(64)]        (16-bit or E4M3)
//     q_out[(b, t), h, 512:576] <- rope(q_pe[(b, t), h])         every head h
//   The rotation is fa_rope_append_kernel.hpp's at R = 64: every product and
//   sum one IEEE fp32 operation (no fma), one rounding to the 16-bit type; the
//   FP8 byte is fa_cache_append_kernel.hpp's contract applied to that rounded
//   value.  A cache row is written iff 0 <= pos < cap, its page id (paged) is
//   inside the pool and (tables given) pos < rope_len; a q_out row iff t < n_b
//   and 0 <= pos < rope_len.  Nothing else is stored to.
//
// Lane map.  Latent slot: one wave owns a token's row.  The 1024 bytes of c_kv
// are one 16-byte load across the 64 lanes; the 128 bytes of k_pe are eight
// 16-byte pieces, held by lanes 0-7 (the other lanes load the piece of lane &
// 7 again, so no branch stands in front of a load, and drop it).  The 16-bit
// row (1152 bytes) is one 64-lane 16-byte store and one 8-lane store at byte
// 1024; the FP8 row (576 bytes) one 64-lane 8-byte store and one 8-lane store
// at byte 512.  A wave keeps kAppendU tokens in flight, a workgroup of four
// waves covers kMlaAppendTokens consecutive tokens of ONE sequence, so the
// length, the count and the page pair are wave-uniform.
// Query slots: eight lanes take the 64 elements of one (token, head) q_pe row,
// a wave instruction rotates eight heads of one token.  The wave holds the
// cos / sin pieces of its kAppendU tokens in registers over all the head
// groups it walks (blockIdx.y, + gridDim.y - kvs, ...): at 128 heads the query
// side moves 14 times the bytes of the latent side and the tables would
// otherwise be two to four further loads per row piece.
// In both, the eight lanes of a 64-element row are lane & 7 = piece: the NeoX
// partner (element i +- 32) is piece ^ 4, four lanes away, and comes by
// ds_swizzle (xor 4: a cross-lane move, no LDS allocation, no address
// register); GPT-J pairs sit inside a lane.  Every lane of the wave executes
// the exchange, outside any divergent branch.  A row that will not be written
// is loaded from the nearest token, head and table row that exist and only its
// store is skipped.  Row loads and stores are nontemporal, table loads plain.
//
// Grid: x = virtual block ids (fa_varlen_map.hpp at kMlaAppendTokens), y =
// slots: [0, kvs) the latent slot (kvs is 1, or 0 when no cache row exists),
// then the query head groups of eight (strided).  No LDS, no scratch.
//
// 2. fa_mla_indexer_append_kernel
//
//   pool row of (b, pos) <- E4M3(clamp(float(x) * (1.0f / s), +-448)), k_scale[row] <- s
//   a = max(max_d |float(x_d)|, 1e-4f), s = a / 448.0f (IEEE), scale_pow2: the
//   smallest power of two >= s, taken on the exponent and mantissa bits.
// Sixteen lanes take a row of 128 elements (8 each), a wave instruction four
// rows, kAppendU instructions in flight; the amax is a 16-lane DPP reduction
// (quad_perm xor 1, xor 2, row_half_mirror, row_mirror: max is symmetric, so
// every lane of the row ends with the row's value).
#pragma once

#include "fa_cache_append_kernel.hpp"

namespace fa {

constexpr int kMlaAppendTokens = 4 * kAppendU;         // tokens of one workgroup, latent append
constexpr int kMlaIdxAppendTokens = 4 * kAppendU * 4;  // ... indexer key writer

struct MlaAppendParams {
  const void* ckv_new;  // [T][512], token stride ckv_stride elements
  const void* kpe_new;  // [T][64], token stride kpe_stride elements
  void* cache;          // [B][cap][576] or [num_pages][page_size][576]; 16-bit or E4M3
  long long ckv_stride, kpe_stride;
  const void* q_pe;     // rows (token, head) of 64 elements
  void* q_out;          // rows (token, head) of 576 elements; [512, 576) written
  long long qs_t, qs_h, qo_t, qo_h;  // token and head strides, elements
  const float* cos;     // [rope_len][32], or nullptr: no rotation (k_pe a bit copy)
  const float* sin;
  const int* cu;        // device int32[B + 1], or nullptr: uniform, sn tokens each
  const int* kv_lens;   // device int32[B]: the lengths after the append
  const float* scale;   // FP8 only: device float[1], or nullptr (= 1.0)
  const int* table;     // paged only: device int32[B][max_pages]
  int batch, total, sn, cap;
  int max_pages, num_pages, page_size;
  int hq, kvs, rope_len, interleaved;
};

struct MlaIdxAppendParams {
  const void* k_new;    // [T][128], token stride k_stride elements
  void* pool;           // E4M3 bytes [num_rows][128]
  float* k_scale;       // [num_rows]
  long long k_stride;
  const int* cu;
  const int* kv_lens;
  const int* table;
  int batch, total, sn, cap;
  int max_pages, num_pages, page_size;
  int pow2;
};

// the table entries one lane needs for one token: NeoX 8 cos + 8 sin, GPT-J 4 + 4
struct MlaCS {
  f32x4 c[2], s[2];
};

__device__ __forceinline__ MlaCS mla_load_cs(const float* cos, const float* sin, int pos, int col, bool inter) {
  MlaCS t;
  const size_t off = (size_t)pos * 32 + col;
  t.c[0] = *reinterpret_cast<const f32x4*>(cos + off);
  t.s[0] = *reinterpret_cast<const f32x4*>(sin + off);
  if (!inter) {
    t.c[1] = *reinterpret_cast<const f32x4*>(cos + off + 4);
    t.s[1] = *reinterpret_cast<const f32x4*>(sin + off + 4);
  } else {
    t.c[1] = t.s[1] = f32x4{0, 0, 0, 0};
  }
  return t;
}

// One 16-byte piece of a 64-element row rotated; called by every lane of the
// wave (the NeoX exchange needs the partner lane active).  hi: this lane holds
// the b halves (piece >= 4).
template <class E>
__device__ __forceinline__ u32x4 mla_rope_rotate(u32x4 raw, const MlaCS& t, bool inter, bool hi) {
#pragma clang fp contract(off)
  typedef typename Elem<E>::x8 ex8;
  const ex8 x = __builtin_bit_cast(ex8, raw);
  ex8 y = x;
  if (inter) {
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
    for (int j = 0; j < 4; ++j)  // bit-mask mode: and 0x1f, or 0, xor 4
      praw[j] = (unsigned)__builtin_amdgcn_ds_swizzle((int)raw[j], (4 << 10) | 0x1f);
    const ex8 o = __builtin_bit_cast(ex8, praw);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float c = t.c[e >> 2][e & 3], s = t.s[e >> 2][e & 3];
      const float xc = (float)x[e] * c, os = (float)o[e] * s;
      // lo lane: a c - b s; hi lane: b c + a s (x - y is x + (-y), bit for bit)
      y[e] = (E)(xc + (hi ? os : -os));
    }
  }
  return __builtin_bit_cast(u32x4, y);
}

// the two table entries a wave's rows (at most `page_size` of them, from row
// rb on) can fall into: slot pg and, from row `edge` on, slot pg + 1
struct MlaPagePair {
  int id0, id1, base0, edge;
};
__device__ __forceinline__ MlaPagePair mla_page_pair(const int* table, int max_pages, int page_size, int b,
                                                     long long rb) {
  MlaPagePair pp;
  const int pg = (int)max(rb, 0LL) / page_size;  // rb < cap = max_pages * page_size
  const int* row = table + (size_t)b * max_pages;
  const int id0 = row[pg];
  const int id1 = row[min(pg + 1, max_pages - 1)];
  pp.id0 = __builtin_amdgcn_readfirstlane(id0);
  pp.id1 = pg + 1 < max_pages ? __builtin_amdgcn_readfirstlane(id1) : -1;
  pp.base0 = pg * page_size;
  pp.edge = pp.base0 + page_size;
  return pp;
}

template <class E, bool PAGED, bool KV8>
__global__ __launch_bounds__(256) void fa_mla_append_kernel(MlaAppendParams p) {
  constexpr int U = kAppendU;
  constexpr int CROW = KV8 ? 576 : 1152;  // cache row bytes
  constexpr int CPIECE = KV8 ? 8 : 16;    // bytes a lane stores
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int piece = lane & 7, grp = lane >> 3;

  int b = 0, seq0 = 0, n = 0, vr = 0;
  if (!varlen_block_u<kMlaAppendTokens>(p.cu, p.sn, p.batch, p.total, (int)blockIdx.x, b, seq0, n, vr)) return;
  b = __builtin_amdgcn_readfirstlane(b);
  seq0 = __builtin_amdgcn_readfirstlane(seq0);
  n = __builtin_amdgcn_readfirstlane(n);
  vr = __builtin_amdgcn_readfirstlane(vr);
  const int tw = vr * kMlaAppendTokens + wave * U;  // the wave's first token; below n <= total
  if (tw >= n) return;
  const int len = __builtin_amdgcn_readfirstlane(p.kv_lens[b]);
  const bool tables = p.cos != nullptr;  // wave-uniform
  const bool latent = (int)blockIdx.y < p.kvs;
  // position (= cache row) of the wave's first token; its rows are rb .. rb + U - 1
  const long long rb = (long long)len - n + tw;
  if (rb + U <= 0) return;                    // every position is negative
  if (tables && rb >= p.rope_len) return;     // no position has a table row
  if (latent && rb >= p.cap) return;          // no row exists
  if (!tables && !latent) return;             // (the host launches no query slot without tables)
  const int r0 = (int)rb;                     // -U < rb < rope_len or cap: an int

  const bool inter = p.interleaved != 0;
  const bool hi = piece >= 4;
  const int col = inter ? 4 * piece : 8 * (piece & 3);
  // loads without a branch: a row that is not written is loaded from the
  // nearest token and table row that exist (tw < n, so n >= 1) and dropped
  bool okr[U];
  int tc[U];
  MlaCS cs[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int t = tw + u, r = r0 + u;
    okr[u] = t < n && r >= 0 && (!tables || r < p.rope_len);
    tc[u] = min(t, n - 1);
    if (tables) {
      cs[u] = mla_load_cs(p.cos, p.sin, min(max(r, 0), p.rope_len - 1), col, inter);
    } else {
      cs[u].c[0] = cs[u].c[1] = cs[u].s[0] = cs[u].s[1] = f32x4{0, 0, 0, 0};
    }
  }

  if (latent) {
    [[maybe_unused]] MlaPagePair pp = {};
    if constexpr (PAGED) pp = mla_page_pair(p.table, p.max_pages, p.page_size, b, rb);
    [[maybe_unused]] float rcp = 1.0f;
    if constexpr (KV8) {
      float sc = 1.0f;
      if (p.scale) sc = p.scale[0];
      rcp = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, 1.0f / sc)));
    }
    const char* cs_ = static_cast<const char*>(p.ckv_new) + lane * 16;
    const char* ks_ = static_cast<const char*>(p.kpe_new) + piece * 16;
    u32x4 cx[U], kx[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long tok = (long long)seq0 + tc[u];
      cx[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(cs_ + tok * p.ckv_stride * 2));
      kx[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ks_ + tok * p.kpe_stride * 2));
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      u32x4 ky = kx[u];
      if (tables) ky = mla_rope_rotate<E>(kx[u], cs[u], inter, hi);  // every lane: the exchange
      const int r = r0 + u;
      bool ok = okr[u] && r < p.cap;
      size_t row;
      if constexpr (PAGED) {
        const bool lo = r < pp.edge;
        const int id = lo ? pp.id0 : pp.id1;
        ok = ok && id >= 0 && id < p.num_pages;
        row = (size_t)id * p.page_size + (size_t)(r - (lo ? pp.base0 : pp.edge));
      } else {
        row = (size_t)b * p.cap + r;
      }
      if (!ok) continue;  // wave-uniform; decided before any address is used
      char* d = static_cast<char*>(p.cache) + row * CROW;
      if constexpr (KV8) {
        __builtin_nontemporal_store(append_cvt_fp8x8<E>(cx[u], rcp), reinterpret_cast<u32x2*>(d + lane * CPIECE));
        if (lane < 8)
          __builtin_nontemporal_store(append_cvt_fp8x8<E>(ky, rcp),
                                      reinterpret_cast<u32x2*>(d + 512 + lane * CPIECE));
      } else {
        __builtin_nontemporal_store(cx[u], reinterpret_cast<u32x4*>(d + lane * CPIECE));
        if (lane < 8) __builtin_nontemporal_store(ky, reinterpret_cast<u32x4*>(d + 1024 + lane * CPIECE));
      }
    }
    return;
  }

  // ---- query slots: head groups of eight, the tables staying in registers
  const int hgroups = (p.hq + 7) >> 3;
  const int step = (int)gridDim.y - p.kvs;
  const char* qs = static_cast<const char*>(p.q_pe) + piece * 16;
  char* qd = static_cast<char*>(p.q_out) + 1024 + piece * 16;
#pragma clang loop unroll(disable)
  for (int hg = (int)blockIdx.y - p.kvs; hg < hgroups; hg += step) {
    const int h = hg * 8 + grp;
    const bool hok = h < p.hq;
    const long long hc = min(h, p.hq - 1);
    u32x4 qx[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long tok = (long long)seq0 + tc[u];
      qx[u] = __builtin_nontemporal_load(
          reinterpret_cast<const u32x4*>(qs + (tok * p.qs_t + hc * p.qs_h) * 2));
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const u32x4 y = mla_rope_rotate<E>(qx[u], cs[u], inter, hi);  // every lane: the exchange
      if (okr[u] && hok) {
        const long long tok = (long long)seq0 + tw + u;
        __builtin_nontemporal_store(y, reinterpret_cast<u32x4*>(qd + (tok * p.qo_t + hc * p.qo_h) * 2));
      }
    }
  }
}

// max over the 16 lanes of a DPP row, left in every lane of it
__device__ __forceinline__ float mla_row16_max(float m) {
#define FA_MLA_DPP_MAX(CTRL)                                                                        \
  m = fmaxf(m, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, m),    \
                                                                      __builtin_bit_cast(int, m),    \
                                                                      CTRL, 0xf, 0xf, false)))
  FA_MLA_DPP_MAX(0xB1);   // quad_perm [1,0,3,2]
  FA_MLA_DPP_MAX(0x4E);   // quad_perm [2,3,0,1]
  FA_MLA_DPP_MAX(0x141);  // row_half_mirror
  FA_MLA_DPP_MAX(0x140);  // row_mirror
#undef FA_MLA_DPP_MAX
  return m;
}

template <class E, bool PAGED>
__global__ __launch_bounds__(256) void fa_mla_indexer_append_kernel(MlaIdxAppendParams p) {
  constexpr int U = kAppendU, RPW = 4, WROWS = U * RPW;
  static_assert(4 * WROWS == kMlaIdxAppendTokens && WROWS <= 64, "a wave's rows must fit one minimal page");
  typedef typename Elem<E>::x8 ex8;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane >> 4, piece = lane & 15;

  int b = 0, seq0 = 0, n = 0, vr = 0;
  if (!varlen_block_u<kMlaIdxAppendTokens>(p.cu, p.sn, p.batch, p.total, (int)blockIdx.x, b, seq0, n, vr)) return;
  b = __builtin_amdgcn_readfirstlane(b);
  seq0 = __builtin_amdgcn_readfirstlane(seq0);
  n = __builtin_amdgcn_readfirstlane(n);
  vr = __builtin_amdgcn_readfirstlane(vr);
  const int tw = vr * kMlaIdxAppendTokens + wave * WROWS;
  if (tw >= n) return;
  const int len = __builtin_amdgcn_readfirstlane(p.kv_lens[b]);
  const long long rb = (long long)len - n + tw;
  if (rb + WROWS <= 0 || rb >= p.cap) return;  // none of the rows exists
  const int r0 = (int)rb + lr, t0 = tw + lr;
  [[maybe_unused]] MlaPagePair pp = {};
  if constexpr (PAGED) pp = mla_page_pair(p.table, p.max_pages, p.page_size, b, rb);

  const char* ks = static_cast<const char*>(p.k_new) + piece * 16;
  u32x4 x[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long long tok = (long long)seq0 + min(t0 + u * RPW, n - 1);
    x[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ks + tok * p.k_stride * 2));
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const ex8 v = __builtin_bit_cast(ex8, x[u]);
    float m = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) m = fmaxf(m, __builtin_fabsf((float)v[j]));
    m = mla_row16_max(m);  // every lane: the cross-lane moves
    float s = fmaxf(m, 1e-4f) / 448.0f;
    if (p.pow2) {
      // the smallest power of two >= s (a positive normal): exponent + 1 unless the mantissa is zero
      const unsigned bits = __builtin_bit_cast(unsigned, s);
      s = __builtin_bit_cast(float, (bits + 0x7fffffu) & 0x7f800000u);
    }
    const u32x2 bytes = append_cvt_fp8x8<E>(x[u], 1.0f / s);
    const int t = t0 + u * RPW, r = r0 + u * RPW;
    bool ok = t < n && r >= 0 && r < p.cap;
    size_t row;
    if constexpr (PAGED) {
      const bool lo = r < pp.edge;
      const int id = lo ? pp.id0 : pp.id1;
      ok = ok && id >= 0 && id < p.num_pages;
      row = (size_t)id * p.page_size + (size_t)(r - (lo ? pp.base0 : pp.edge));
    } else {
      row = (size_t)b * p.cap + r;
    }
    if (!ok) continue;  // decided before any address is used
    __builtin_nontemporal_store(bytes, reinterpret_cast<u32x2*>(static_cast<char*>(p.pool) + row * 128 + piece * 8));
    if (piece == 0) p.k_scale[row] = s;
  }
}

}  // namespace fa
