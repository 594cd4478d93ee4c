// Cache append for gfx950: write new K/V tokens into the caches the decode
// kernels (fa_decode_kernel.hpp) read -- contiguous or paged, 16-bit or FP8
// E4M3 with one fp32 scale per K/V head.
//
//   n_b = clamp(new_lens[b], 0, Sn)            (new_lens == nullptr: Sn)
//   for t in [0, n_b):  r = kv_lens[b] - n_b + t
//     cache row r of (b, hkv) <- k_new[b, hkv, t, :]      (same for V)
//
// kv_lens[b] is the length AFTER the append (what the following decode call
// takes) and is not clamped: a row is written iff 0 <= r < cap, so a length
// past the capacity drops the rows that do not exist.  Paged: row r lives in
// page table[b][r / page_size] at offset r % page_size and is written iff that
// id is inside [0, num_pages).  Whether a row is written is decided before any
// address is formed from it, and nothing but the rows named above is stored to.
// Two batch elements whose tables map the same page row race: one of them
// wins, unspecified which (the caller's problem).
//
// FP8 cache: the byte stored for a source element x with scale s is
//   y    = float(x) * (1.0f / s)         both in IEEE fp32, 1.0f / s correctly rounded
//   byte = E4M3(clamp(y, -448, 448))     round to nearest even, subnormals down
//                                        to 2^-9, -0.0 keeps its sign
// +-inf saturates to +-448, a NaN stores a NaN code (0x7f or 0xff).  The
// reciprocal form is the contract (for power-of-two scales it equals x / s):
// s is uniform per head, so the division is paid once per wave.
//
// Lane map.  A lane moves one 16-byte piece of a source row: HDIM / 8 lanes
// per row, RPW = 512 / HDIM rows per wave instruction, so every load covers
// 1 KB of consecutive source bytes and every store RPW whole cache rows (1 KB
// of a 16-bit cache, 512 B of an FP8 one: whole 128-byte lines in both).  A
// wave owns kU * RPW consecutive tokens and issues its 2 kU loads (K and V)
// before the first store; a workgroup is four such waves of one (b, hkv).
// Every byte is touched once, so loads and stores carry the nontemporal hint
// (measured: 9-10 % on the contiguous prefill append).
// The length, the new-token count, the reciprocal scales and (paged) the two
// table entries a wave's rows can fall into are wave-uniform: the wave's rows
// are at most 64 <= page_size, so they span at most two pages and ONE division
// by the page size per wave places all of them.  No LDS, no scratch.
#pragma once

#include "fa_fwd_kernel.hpp"
#include "fa_varlen_map.hpp"

namespace fa {

struct AppendParams {
  const void* k_new;    // [B][Hkv][Sn][D], 16-bit
  const void* v_new;
  void* k_cache;        // [B][Hkv][cap][D], or the pool [num_pages][Hkv][page_size][D]
  void* v_cache;
  const int* kv_lens;   // device int32[B]: the lengths after the append
  const int* new_lens;  // device int32[B], or nullptr (= sn)
  int batch, hkv, sn, cap;
  // paged only
  const int* table;     // device int32[B][max_pages]
  int max_pages, num_pages, page_size;
  unsigned long long page_bytes;  // Hkv * page_size * cache row bytes
  unsigned long long head_bytes;  // page_size * cache row bytes
  // FP8 only: device float[Hkv], or nullptr (= 1.0)
  const float* k_scale;
  const float* v_scale;
};

constexpr int kAppendU = 4;  // wave instructions per tensor a wave keeps in flight
// tokens one workgroup (four waves) covers
template <int HDIM>
constexpr int append_block_tokens() {
  return 4 * kAppendU * (512 / HDIM);
}

// 8 elements of T (one 16-byte piece) -> 8 E4M3 bytes by the contract above.
// The library is built with -fno-honor-nans: NaN is found on the bit pattern
// and turned into a NaN code by setting the byte's low seven bits.
template <class T>
__device__ __forceinline__ u32x2 append_cvt_fp8x8(u32x4 raw, float rcp) {
  typedef typename Elem<T>::x8 tx8;
  constexpr unsigned kInf16 = std::is_same<T, __bf16>::value ? 0x7f80u : 0x7c00u;
  const tx8 x = __builtin_bit_cast(tx8, raw);
  float y[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) y[j] = __builtin_amdgcn_fmed3f((float)x[j] * rcp, -448.0f, 448.0f);
  u32x2 w;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    int b = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * h], y[4 * h + 1], 0, false);
    b = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * h + 2], y[4 * h + 3], b, true);
    unsigned nan = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned bits = (raw[2 * h + (j >> 1)] >> (16 * (j & 1))) & 0x7fffu;
      nan |= bits > kInf16 ? 0x7fu << (8 * j) : 0u;
    }
    w[h] = (unsigned)b | nan;
  }
  return w;
}

// T: the source element type when KV8 (f16 or __bf16: what the conversion
// reads); a 16-bit cache takes a bit copy, one instantiation (T = unsigned
// short) for both types.  Grid: x = token blocks, y over K/V heads, z over
// the batch (both strided, so either may exceed the grid limit).
//
// The packed entries (fa_cache_append_varlen_*) name their source PackedSrc<T>:
// the kernel takes VARLEN from that, so the padded entries' instantiations
// (and their symbols) are what they were.  k_new / v_new are then token-major
// [T][Hkv][D] and the fields of p are read as
//   new_lens = cu_seqlens (int32[B + 1], required), sn = T, batch = B
// Grid: x = virtual block ids (fa_varlen_map.hpp at append_block_tokens()
// granularity: a workgroup's tokens, so every wave's, belong to ONE sequence
// and len, n, the page pair and the scales stay wave-uniform), y over K/V
// heads, no z.  Token t of sequence b is packed row s_b + t; source rows are
// Hkv * SROW bytes apart.
template <class T>
struct PackedSrc {};
template <class T>
struct AppendSrc {
  typedef T elem;
  static constexpr bool packed = false;
};
template <class T>
struct AppendSrc<PackedSrc<T>> {
  typedef T elem;
  static constexpr bool packed = true;
};

template <class T, int HDIM, bool PAGED, bool KV8>
__global__ __launch_bounds__(256) void fa_cache_append_kernel(AppendParams p) {
  constexpr bool VARLEN = AppendSrc<T>::packed;
  using E = typename AppendSrc<T>::elem;
  constexpr int LPR = HDIM / 8;         // lanes per row
  constexpr int RPW = 64 / LPR;         // rows per wave instruction
  constexpr int WROWS = kAppendU * RPW; // consecutive tokens of one wave (16 or 32)
  constexpr int SROW = 2 * HDIM;        // source row bytes
  constexpr int CROW = KV8 ? HDIM : 2 * HDIM;  // cache row bytes
  constexpr int CPIECE = KV8 ? 8 : 16;  // bytes a lane stores
  static_assert(WROWS <= 64, "a wave's rows must fit one minimal page");

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane / LPR, piece = lane % LPR;
  // VARLEN: the workgroup's sequence, its first packed row, its tokens and the block within it
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
  // source: bytes between consecutive tokens
  [[maybe_unused]] const size_t sstr = VARLEN ? (size_t)p.hkv * SROW : (size_t)SROW;

  for (int hk = blockIdx.y; hk < p.hkv; hk += gridDim.y) {
    // VARLEN: the one sequence of this workgroup
    for (int b = VARLEN ? vb : (int)blockIdx.z; VARLEN ? b == vb : b < p.batch;
         b += VARLEN ? 1u : gridDim.z) {
      // the wave-uniform loads first, together: one round trip before the
      // rows are known (two when paged: the table entries need the length)
      int len = p.kv_lens[b], n = p.sn;
      [[maybe_unused]] float ksc = 1.0f, vsc = 1.0f;
      if constexpr (VARLEN) {
        n = seqn;  // already in [0, sn - seq0]
      } else {
        if (p.new_lens) n = p.new_lens[b];
      }
      if constexpr (KV8) {
        if (p.k_scale) ksc = p.k_scale[hk];
        if (p.v_scale) vsc = p.v_scale[hk];
      }
      len = __builtin_amdgcn_readfirstlane(len);
      n = __builtin_amdgcn_readfirstlane(min(max(n, 0), p.sn));
      if (tw >= n) continue;
      // row of the wave's first token; the wave's rows are rb .. rb + WROWS - 1
      const long long rb = (long long)len - n + tw;
      if (rb + WROWS <= 0 || rb >= p.cap) continue;  // none of them exists
      const int r0 = (int)rb + lr, t0 = (int)tw + lr;  // rb > -WROWS and < cap, tw < sn: ints

      // paged: the wave's rows lie in page slot pg and, from row `edge` on, in
      // slot pg + 1 (WROWS <= page_size); a slot past the table holds no row
      [[maybe_unused]] int id0 = 0, id1 = 0, edge = 0, base0 = 0;
      if constexpr (PAGED) {
        const int pg = (int)max(rb, 0LL) / p.page_size;
        const int* row = p.table + (size_t)b * p.max_pages;
        id0 = row[pg];
        id1 = row[min(pg + 1, p.max_pages - 1)];
        id0 = __builtin_amdgcn_readfirstlane(id0);
        id1 = pg + 1 < p.max_pages ? __builtin_amdgcn_readfirstlane(id1) : -1;
        base0 = pg * p.page_size;
        edge = base0 + p.page_size;
      }
      [[maybe_unused]] float krcp = 1.0f, vrcp = 1.0f;
      if constexpr (KV8) {
        krcp = __builtin_bit_cast(
            float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, 1.0f / ksc)));
        vrcp = __builtin_bit_cast(
            float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, 1.0f / vsc)));
      }
      const size_t bh = (size_t)b * p.hkv + hk;
      const size_t soff = VARLEN ? (((size_t)seq0 + t0) * p.hkv + hk) * SROW + piece * 16
                                 : (bh * p.sn + t0) * SROW + piece * 16;
      const char* ks = static_cast<const char*>(p.k_new) + soff;
      const char* vs = static_cast<const char*>(p.v_new) + soff;

      bool ok[kAppendU];
      u32x4 kx[kAppendU], vx[kAppendU];
#pragma unroll
      for (int u = 0; u < kAppendU; ++u) {
        const int r = r0 + u * RPW;
        ok[u] = t0 + u * RPW < n && r >= 0 && r < p.cap;
        if constexpr (PAGED) {
          const int id = r < edge ? id0 : id1;
          ok[u] = ok[u] && id >= 0 && id < p.num_pages;
        }
        kx[u] = vx[u] = u32x4{0, 0, 0, 0};
        if (ok[u]) {
          kx[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ks + (size_t)u * RPW * sstr));
          vx[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(vs + (size_t)u * RPW * sstr));
        }
      }
#pragma unroll
      for (int u = 0; u < kAppendU; ++u) {
        if (!ok[u]) continue;
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
          __builtin_nontemporal_store(append_cvt_fp8x8<E>(kx[u], krcp), reinterpret_cast<u32x2*>(kd));
          __builtin_nontemporal_store(append_cvt_fp8x8<E>(vx[u], vrcp), reinterpret_cast<u32x2*>(vd));
        } else {
          __builtin_nontemporal_store(kx[u], reinterpret_cast<u32x4*>(kd));
          __builtin_nontemporal_store(vx[u], reinterpret_cast<u32x4*>(vd));
        }
      }
    }
  }
}

}  // namespace fa
