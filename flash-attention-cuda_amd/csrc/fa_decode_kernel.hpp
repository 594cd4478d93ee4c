// Decode attention over a K/V cache for gfx950: a few query tokens (1..16)
// per head against a long cache whose length differs per batch element, with
// grouped K/V heads (GQA / MQA) and the key range split across workgroups and
// merged in the same launch.
//
//   O[b,hq,t,:] = softmax(Q[b,hq,t,:] . K[b,hkv,0:len_b,:]^T / sqrt(D) [+ mask]) V[b,hkv,0:len_b,:]
//   hkv = hq / (Hq / Hkv);  causal (bottom-right): token t sees keys <= len_b - Sq + t
//
// Decomposition.  The G*Sq query rows that share one K/V head are contiguous
// in a [B][Hq][Sq][D] tensor (row r = (hq - hkv*G)*Sq + t), so they form the
// query dimension of the MFMAs in NB = 1, 2 or 4 blocks of 16 rows; more than
// 64 rows become several row groups.  A workgroup = (batch, kv head, row
// group, key piece), four waves.  The batch element's own 64-key tiles
// (from kv_lens[b], not from the capacity) are cut into num_splits pieces;
// wave w of a piece streams tiles w, w+4, ... with no workgroup barrier in
// the loop and keeps its own (m, l, O) in the exp2 domain.  The four partials
// are merged once through LDS; with num_splits > 1 each piece then hands its
// normalised partial to the last-arriving piece through the workspace (the
// causal split tier's hand-off, fa_w4_kernel.hpp).
//
// Operand movement (the operand is streamed once, so LDS is used only where a
// transpose needs it):
//   K: straight from HBM into the A-operand registers of S^T = K . Q^T, one
//      buffer_load_dwordx4 per lane per 16-key x 32-dim fragment, the next
//      tile's 16 fragments issued right after the current tile's QK^T.
//   V: register-staged into a wave-private 16-KB LDS image (image A of
//      fa_fwd_kernel.hpp) and read back with ds_read_b64_tr_b16 as the A
//      operand of O^T = V^T . P^T.  The next tile's V loads are issued right
//      after the image is written, so they fly during PV, the next QK^T and
//      softmax.  The image is wave-private: no barrier, the wave's own LDS
//      order suffices.
// All loads are plain builtins, so hipcc counts vmcnt itself and each wave
// keeps one K or V tile (16 KB at head_dim 128) in flight at any time.
// The K/V descriptors' range is len_b rows: rows past the length read as
// zeros whatever the capacity padding holds (P = 0 and a finite V).
#pragma once

#include "fa_fwd_kernel.hpp"

namespace fa {

struct DecodeParams {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  float* lse;          // [B][Hq][Sq] natural-log LSE, or nullptr
  const int* kv_lens;  // device int32[B], or nullptr (= cap)
  int hq, hkv, sq, cap;
  int group;           // hq / hkv
  int rows;            // group * sq: query rows per K/V head
  int rgroups;         // row groups (16 * NB rows each) per K/V head
  int num_splits;
  int causal;
  float c;             // log2(e) / sqrt(D)
  unsigned* ws_ctr;    // [unit] arrival counters (the workspace's first 64 KB)
  float* ws_lse;       // [unit][piece][16 NB] log2-sum-exp
  float* ws_o;         // [unit][piece][16 NB][D] normalised partial O
};

// The paged twin (fa_decode_paged.hip): the cache is a pool of fixed-size pages
//   k_pages, v_pages  [num_pages][Hkv][page_size][D]   (page_size % 64 == 0)
// plus a block table int32[B][max_pages]: entry j of row b is the pool page
// that holds keys [j * page_size, (j + 1) * page_size) of batch element b.
// `k` / `v` are the pools and `cap` the logical capacity max_pages * page_size.
//
// It is the same kernel template (fa_decode_kernel<..., PAGED = true>): the
// same (batch, kv head, row group, piece) workgroups, wave w streams the same
// tiles t0 + w, t0 + w + 4, ... with the same operations in the same order,
// the same in-CU merge and the same in-launch piece merge through the
// workspace.  A 64-key tile never straddles a page, so all that differs per
// tile is the K and V buffer descriptor: its base is head hk's rows of the
// tile's page (64-bit arithmetic, pools exceed 4 GiB), its range ends at the
// tile's last live row, (tile % tiles_per_page) * 64 + clamp(len_b - 64 tile,
// 0, 64) rows, and the loads add the tile's offset in the page.  Rows past the
// length and unmapped pages are therefore never read, and a page id outside
// the pool gives a zero range.  Output and LSE are bit-identical to the
// contiguous kernel on the gathered cache with the same num_splits.
struct DecodePagedParams : DecodeParams {
  const int* table;          // device int32[B][max_pages]: pool page of keys [j*page_size, +page_size)
  int max_pages;             // table row length
  int num_pages;             // pool pages: an id outside [0, num_pages) reads as zero rows
  int tpp;                   // 64-key tiles per page (page_size / 64)
  int adv_pages, adv_tiles;  // 4 / tpp, 4 % tpp: a wave's step of four tiles in (page, tile in page)
  unsigned long long page_bytes;  // Hkv * page_size * row bytes
  unsigned long long head_bytes;  // page_size * row bytes
};

// The FP8 cache twins (fa_decode_kv8.hip, fa_decode_paged_kv8.hip): K and V
// are OCP FP8 E4M3 bytes with one fp32 scale per K/V head each (device
// arrays of Hkv floats, nullptr = 1.0); Q and O stay 16-bit.
struct DecodeKv8Params : DecodeParams {
  const float* k_scale;
  const float* v_scale;
};
struct DecodePagedKv8Params : DecodePagedParams {
  const float* k_scale;
  const float* v_scale;
};

// The sliding-window entries (fa_decode_win_*, fa_prefill[_varlen]_win_*) pass
// their parameters as Windowed<one of the structs above / of
// fa_prefill_kernel.hpp>: the kernels take WIN from the type, so the entries
// without a window keep their instantiations and their symbols (DESIGN.md
// §3.0m).  window = W >= 1: a row at position pos sees the keys
//   max(0, pos - W + 1) <= j <= pos
// (its own included: Hugging Face's sliding_window = W, flash-attn's
// window_size = (W - 1, 0)).  The host clamps W to the capacity, past which it
// changes nothing, so pos - W cannot overflow.
template <class Base>
struct Windowed : Base {
  int window;
};
template <class P>
struct ParamsWindowed : std::false_type {};
template <class Base>
struct ParamsWindowed<Windowed<Base>> : std::true_type {};
// The attention-sink entries (fa_decode_sink_*, fa_prefill[_varlen]_sink_*)
// pass Sinked<Windowed<...>>: `sinks` is a device array of Hq floats (nullptr:
// no sinks), one logit per query head in natural-log units that joins the
// softmax denominator and carries no value:
//   den = exp(sinks[h]) + sum_j exp(s_j),  O = sum_j exp(s_j) v_j / den,
//   LSE = log(den);  a row that sees no key: O = 0, LSE = sinks[h].
// The kernels take SINK from the type as they take WIN, and the sink enters
// once, where a row's (m, l) becomes 1 / l and the LSE (sink_fold() of
// fa_fwd_kernel.hpp).
template <class Base>
struct Sinked : Base {
  const float* sinks;
};
template <class P>
struct ParamsSinked : std::false_type {};
template <class Base>
struct ParamsSinked<Sinked<Base>> : std::true_type {};
template <class Base>
struct ParamsWindowed<Sinked<Base>> : ParamsWindowed<Base> {};
// The tree-masked decode entries (fa_decode_tree_*, include/fa_mi355x_tree.h)
// pass Treed<Sinked<Windowed<...>>>: the Sq query tokens are the draft tokens
// of a speculation tree, the last Sq keys of the cache, and `tree` is a device
// int32 [B][Sq] (nullptr: the chain), word t the set of draft tokens row t
// sees, its ancestors and itself.  With base = len - Sq and
// m_t = tree[b][t] & ((1 << Sq) - 1):
//   draft key i (cache row base + i >= 0): seen iff bit i of m_t is set;
//   prefix key j < base: seen iff j > pos_t - W, pos_t = base + depth_t,
//     depth_t = max(popcount(m_t) - 1, 0)  (W = capacity: every prefix key).
// The chain is m_t = (2 << t) - 1.  The kernel takes TREE from the type as it
// takes WIN and SINK; the words are read only in the tiles that hold a draft
// key or a window edge, so any contents are safe: they deselect keys, no more.
template <class Base>
struct Treed : Base {
  const int* tree;
};
template <class P>
struct ParamsTreed : std::false_type {};
template <class Base>
struct ParamsTreed<Treed<Base>> : std::true_type {};
template <class Base>
struct ParamsWindowed<Treed<Base>> : ParamsWindowed<Base> {};
template <class Base>
struct ParamsSinked<Treed<Base>> : ParamsSinked<Base> {};

// Rows but no keys, with sinks: LSE[row] = sinks[head of the row].  Padded
// layouts [B][Hq][Sq] (head = row / sq % hq); PACKED: [Hq][T] (head = row / sq,
// sq = T).
template <bool PACKED>
__global__ void fa_sink_fill_lse_kernel(float* lse, const float* sinks, size_t nrow, int hq, int sq) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nrow) return;
  const size_t h = PACKED ? i / (size_t)sq : i / (size_t)sq % (size_t)hq;
  lse[i] = sinks[h];
}

// an offset no K/V descriptor's range reaches: the load returns zeros and
// moves no memory.  The windowed kernels give it to the lanes whose row of the
// first tile lies below the window, so those rows are not read at all.
constexpr int kBelowWindow = 0x7ffffff0;

// 8 E4M3 bytes (two words) -> 8 elements of T.  Exact: every finite E4M3 code
// is representable in f16 and in bf16, and the scale operand is 1.0.
template <class T>
__device__ __forceinline__ typename Elem<T>::x8 cvt_fp8x8(unsigned w0, unsigned w1) {
  typedef T tx2 __attribute__((ext_vector_type(2)));
  tx2 a, b, c, d;
  if constexpr (std::is_same<T, __bf16>::value) {
    a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false);
    b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true);
    c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false);
    d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true);
  } else {
    a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, false);
    b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, true);
    c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, false);
    d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, true);
  }
  return typename Elem<T>::x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

constexpr int kDecodeVBytes = 4 * 64 * 256;  // four wave-private V images
template <int HDIM, int NB>
constexpr int decode_lds_bytes() {
  // in-CU merge region (reuses the images): four waves' O and (m, l); it
  // also covers the Q image of the 64-row head_dim-128 variant (16 KB)
  constexpr int merge = 4 * NB * (HDIM / 16) * 1024 + 4 * NB * 64 * 8;
  return merge > kDecodeVBytes ? merge : kDecodeVBytes;
}

// The last-arriving piece's merge of a unit's NS partials, in piece order:
//   O = sum_s 2^(lse_s - M) O_s / sum_s 2^(lse_s - M),  M = max_s lse_s.
// Thread = one 16-B chunk (4 fp32) of one row; every slab load is sc1.
// SINK: the row's sink is one more term, with O = 0 and log2-sum-exp sink2 (the
// pieces' partials carry none of it, so it counts once).
template <class T, int HDIM, int NB, bool SINK = false>
__device__ __forceinline__ void decode_merge_pieces(const DecodeParams& p, size_t unit, int ns,
                                                    __amdgpu_buffer_rsrc_t ro, float* lse_out,
                                                    int row0, int tid,
                                                    [[maybe_unused]] const float* sinks = nullptr,
                                                    [[maybe_unused]] int hk = 0) {
  constexpr int kSc1 = 16, RW = 16 * NB, CH = HDIM / 4;
  typedef typename Elem<T>::x4 tx4;
  const __amdgpu_buffer_rsrc_t rs =
      make_rsrc(p.ws_o + unit * (size_t)ns * RW * HDIM, ns * RW * HDIM * 4);
  const __amdgpu_buffer_rsrc_t rls = make_rsrc(p.ws_lse + unit * (size_t)ns * RW, ns * RW * 4);
  for (int idx = tid; idx < RW * CH; idx += 256) {
    const int row = idx / CH, ch = idx - row * CH;
    float M = ninf();
    if constexpr (SINK) {
      // row r of the K/V head's group * Sq rows belongs to head hk * group + r / Sq
      if (sinks)
        M = sinks[hk * p.group + min(row0 + row, p.rows - 1) / p.sq] * 1.4426950408889634f;
    }
    [[maybe_unused]] const float sink2 = M;
#pragma unroll 4
    for (int s = 0; s < ns; ++s)
      M = fmaxf(M, __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                 rls, (s * RW + row) * 4, 0, kSc1)));
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float den = 0.f;
    if constexpr (SINK) den = sink2 == ninf() ? 0.f : __builtin_amdgcn_exp2f(sink2 - M);
#pragma unroll 4
    for (int s = 0; s < ns; ++s) {
      const float l = __builtin_bit_cast(
          float, __builtin_amdgcn_raw_buffer_load_b32(rls, (s * RW + row) * 4, 0, kSc1));
      const f32x4 x = __builtin_bit_cast(
          f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, ((s * RW + row) * HDIM + 4 * ch) * 4, 0,
                                                       kSc1));
      const float w = M == ninf() ? 0.f : __builtin_amdgcn_exp2f(l - M);
      den += w;
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(w, x[j], acc[j]);
    }
    const float inv = den > 0.f ? 1.0f / den : 0.f;
    tx4 out;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = (T)(acc[j] * inv);
    buf_store8(ro, row * (2 * HDIM) + 8 * ch, __builtin_bit_cast(f16x4, out));
    if (lse_out && ch == 0 && row0 + row < p.rows)
      lse_out[row] = den > 0.f ? (M + __builtin_log2f(den)) * 0.6931471805599453f : ninf();
  }
}

// PAGED = false: P = DecodeParams, the contiguous cache (fa_decode.hip).
// PAGED = true: P = DecodePagedParams (fa_decode_paged.hip): the
// decomposition, the order of operations and the merges are the same, only
// where a tile's 64 rows start and how many of them are live comes from the
// block table (tile_at() below), so the result is bit-identical to the
// contiguous kernel on the gathered cache.  Code for PAGED sits under
// `if constexpr`: the PAGED = false instantiations carry none of it
// (DESIGN.md §3.0h).
//
// KV = T: the cache holds T.  KV = unsigned char (P = a Kv8 params struct): the
// cache holds E4M3 bytes, converted to T in registers:
//   K: one 16-B load per lane covers the lane's 8 dims of TWO k-steps (dims
//      64 tt + 16 g + 8 h .. +7 for k-step 2 tt + h), and Q's fragments are
//      loaded under the same permutation of d (the sum over d has no order);
//   V: one 16-B load carries 16 elements of a row and becomes two 16-B writes
//      into the same wave-private image, so the transposed reads and the PV
//      MFMAs are those of the 16-bit kernel;
//   k_scale[hkv] is folded into the score scale c, v_scale[hkv] into the
//      normalisation of the in-CU merge.
// All of it sits under `if constexpr (KV8)`: the KV = T instantiations carry
// none of it.
template <class T, int HDIM, int NB, bool PAGED = false, class P = DecodeParams, class KV = T>
__global__ __launch_bounds__(256, 1) void fa_decode_kernel(P p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool KV8 = !std::is_same<KV, T>::value;
  constexpr bool WIN = ParamsWindowed<P>::value;
  constexpr bool SINK = ParamsSinked<P>::value;
  constexpr bool TREE = ParamsTreed<P>::value;
  static_assert(!TREE || (WIN && SINK), "the tree kernels are instantiated over the sink ones");
  static_assert(!KV8 || std::is_same<KV, unsigned char>::value, "the cache holds T or E4M3 bytes");
  constexpr int ROW = 2 * HDIM;      // bytes per Q/O row
  constexpr int CROW = KV8 ? HDIM : 2 * HDIM;  // bytes per K/V cache row
  constexpr int NTQ = HDIM / 32;     // 32-wide k-steps of QK^T
  constexpr int NE = HDIM / 16;      // 16-wide d-blocks of O
  constexpr int RW = 16 * NB;        // query rows per workgroup
  constexpr int RPW = (KV8 ? 1024 : 512) / HDIM;  // V rows one load instruction of a wave covers
  constexpr int NPASS = 64 / RPW;    // V load instructions per tile
  constexpr int EW = NE / 4;         // d-blocks each wave finishes in the in-CU merge
  // the next tile's K is issued right after QK^T; with 64 rows at head_dim 128
  // the scores and the next K do not fit the register file together (scratch),
  // so there it is issued once the scores are dead (P built)
  constexpr bool kEarlyK = !(NB == 4 && HDIM == 128);
  constexpr bool kQLds = NB == 4 && HDIM == 128;
  typedef typename Elem<T>::x8 tx8;
  typedef typename Elem<T>::x4 tx4;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  const int sg = ((g & 1) << 1) | (g >> 1);

  // workgroup -> (batch, kv head, row group, piece)
  const int ns = p.num_splits;
  const unsigned unit = blockIdx.x / (unsigned)ns;
  const int piece = (int)(blockIdx.x - unit * (unsigned)ns);
  const int rg = (int)(unit % (unsigned)p.rgroups);
  const unsigned bhk = unit / (unsigned)p.rgroups;  // b * Hkv + hkv
  const int b = (int)(bhk / (unsigned)p.hkv), hk = (int)(bhk - (unsigned)b * p.hkv);
  int len = p.kv_lens ? p.kv_lens[b] : p.cap;
  len = __builtin_amdgcn_readfirstlane(min(max(len, 0), p.cap));
  const int ntiles = (len + 63) >> 6;
  // WIN: the first key any row sees is row 0's lower bound; the pieces divide
  // the tiles from its tile on (an empty piece hands off l = 0 like one past
  // ntiles).  lo_in: the rows of tile tlo below that key, which are not read.
  [[maybe_unused]] int win = 0, kv_lo = 0, tlo = 0;
  if constexpr (WIN) {
    win = p.window;
    kv_lo = max(0, len - p.sq + 1 - win);
    tlo = kv_lo >> 6;
  }
  const int t0 = WIN ? tlo + (int)((long long)(ntiles - tlo) * piece / ns)
                     : (int)((long long)ntiles * piece / ns);
  const int t1 = WIN ? tlo + (int)((long long)(ntiles - tlo) * (piece + 1) / ns)
                     : (int)((long long)ntiles * (piece + 1) / ns);

  const int row0 = rg * RW;  // first row of this group among the kv head's rows
  const size_t qrow = ((size_t)b * p.hq + (size_t)hk * p.group) * p.sq;  // [B*Hq*Sq] row of r = 0
  const int nrows = max(0, min(RW, p.rows - row0));
  const char* qb = static_cast<const char*>(p.q) + (qrow + row0) * ROW;
  char* ob = static_cast<char*>(p.o) + (qrow + row0) * ROW;
  const size_t kvoff = PAGED ? 0 : (size_t)bhk * (size_t)p.cap * CROW;
  const __amdgpu_buffer_rsrc_t rq = make_rsrc(qb, nrows * ROW);
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(ob, nrows * ROW);
  // contiguous: one descriptor per operand for the whole head.  Paged: one per
  // tile, rebuilt by tile_at() before the tile's loads are issued
  __amdgpu_buffer_rsrc_t rk =
      make_rsrc(static_cast<const char*>(p.k) + kvoff, PAGED ? 0 : len * CROW);
  __amdgpu_buffer_rsrc_t rv =
      make_rsrc(static_cast<const char*>(p.v) + kvoff, PAGED ? 0 : len * CROW);

  // score scale: the cache's K scale rides on it (a wave-uniform load)
  [[maybe_unused]] float csc = 1.0f;
  if constexpr (KV8) csc = p.k_scale ? p.c * p.k_scale[hk] : p.c;

  // Q fragments (B operand): qf[nb][t] = Q[16 nb + r16][32 t + 8 g .. +7]; rows
  // past the group's last read as zeros.  Held in registers, except with 64
  // rows at head_dim 128 (kQLds: the register file cannot hold them beside
  // the O accumulator and both prefetches): there wave nb parks block nb's
  // fragments lane-linearly behind the V images and every wave re-reads them
  // per tile.  KV8: k-step t holds dims 64 (t >> 1) + 16 g + 8 (t & 1) .. +7,
  // the dims K's 16-byte loads deliver.
  tx8 qf[kQLds ? 1 : NB][NTQ];
  char* qimg = smem + kDecodeVBytes;
  if constexpr (kQLds) {
#pragma unroll
    for (int t = 0; t < NTQ; ++t)
      *reinterpret_cast<u32x4*>(qimg + ((wave * NTQ + t) * 64 + lane) * 16) = __builtin_bit_cast(
          u32x4, buf_load16(rq, (16 * wave + r16) * ROW +
                              (KV8 ? 128 * (t >> 1) + 32 * g + 16 * (t & 1) : (4 * t + g) * 16)));
    __syncthreads();
  } else {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int t = 0; t < NTQ; ++t)
        qf[nb][t] = __builtin_bit_cast(
            tx8, buf_load16(rq, (16 * nb + r16) * ROW +
                                    (KV8 ? 128 * (t >> 1) + 32 * g + 16 * (t & 1) : (4 * t + g) * 16)));
  }
  auto qfrag = [&](int nb, int t) -> tx8 {
    if constexpr (kQLds)
      return *reinterpret_cast<const tx8*>(qimg + ((nb * NTQ + t) * 64 + lane) * 16);
    else
      return qf[nb][t];
  };

  // first key a row does not see
  int lim[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int r = row0 + 16 * nb + r16;
    lim[nb] = p.causal ? len - p.sq + 1 + r % p.sq : len;
  }
  // tiles ending past it need the mask.  TREE: draft key 0 itself (row len -
  // sq) may be hidden from a row; `lim` is unused there (the rows' bounds come
  // from the mask words, read where the mask is applied)
  const int mask_from = TREE ? len - p.sq : p.causal ? len - p.sq + 1 : len;
  // WIN: row r also masks the keys below lim - win; tiles starting below the
  // last row's bound need the mask
  [[maybe_unused]] const int mask_below = WIN ? len - win : 0;

  // K: A-operand row r16 of 16-key block cb is key 16 cb + sigma(r16), so the
  // S^T accumulator of lane (g, r16) holds keys 16 cb + 4 sg + i (the order
  // the transposed V reads deliver)
  const unsigned krow = 4 * ((((r16 >> 2) & 1) << 1) | (r16 >> 3)) + (r16 & 3);
  const unsigned kvo = krow * CROW + g * 16;
  // V staging (conflict-free writes into image A) and transposed reads
  // KV8: lane = (16-B piece vch of cache row vrl); the piece becomes chunks
  // 2 vch and 2 vch + 1 of the image row.  ds_write_b128 banks are 128 B wide
  // per 8 consecutive lanes: lane bits 0..2 = (vch bit 0, row bit 0, row bit
  // 2), which lds_off() turns into the 8 distinct 16-B slots of a bank row
  // (slot bit 0 = row bit 2 ^ j, bit 1 = vch bit 0 ^ row bit 3, + 4 (row & 1)).
  const int vrl = KV8 ? (HDIM == 128 ? ((lane >> 1) & 1) + 2 * ((lane >> 5) & 1) + 4 * ((lane >> 2) & 1)
                                     : ((lane >> 1) & 1) + 2 * ((lane >> 4) & 1) +
                                           4 * ((lane >> 2) & 1) + 8 * ((lane >> 5) & 1))
                      : HDIM == 128 ? 2 * ((lane >> 5) & 1) + ((lane >> 2) & 1)
                                    : 2 * ((lane >> 4) & 3) + ((lane >> 2) & 1);
  const int vch = KV8 ? (HDIM == 128 ? (lane & 1) + 2 * ((lane >> 3) & 3) : (lane & 1) + 2 * ((lane >> 3) & 1))
                      : HDIM == 128 ? 4 * ((lane >> 3) & 3) + (lane & 3) : 4 * ((lane >> 3) & 1) + (lane & 3);
  const unsigned vvo = vrl * CROW + vch * 16;
  char* vimg = smem + 16384 * wave;
  int vaddr[2];
  {
    const int qq = r16 >> 2, pp = r16 & 3;
#pragma unroll
    for (int ep = 0; ep < 2; ++ep)
      vaddr[ep] = 2048 * (sg >> 1) + 64 * (4 * (sg & 1) + qq) + 16 * ((2 * ep + (pp >> 1)) ^ sg) +
                  8 * (pp & 1);
  }

  // lsum: the lane's share of its row's l (its 16 keys of every tile); the four
  // lanes of a row add theirs up once, before the in-CU merge
  f32x4 acc[NB][NE];
  float m[NB], lsum[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
    for (int e = 0; e < NE; ++e) acc[nb][e] = f32x4{};
    lsum[nb] = 0.f;
    m[nb] = ninf();
  }

  tx8 kf[4][NTQ];  // (unused with KV8)
  [[maybe_unused]] u32x4 kq[KV8 ? 4 : 1][KV8 ? NTQ / 2 : 1];  // KV8: 16 bytes = two k-steps
  u32x4 vr[NPASS];
  // tile `tl`'s loads; a tile past the piece is addressed past the
  // descriptor's range (row len): zeros, no memory traffic, no branch
  // (paged: the descriptors and `tofs` are the tile's own, tile_at(), and `tl` is unused)
  [[maybe_unused]] unsigned tofs = 0;  // byte offset of the tile's rows in head hk's part of its page
  auto load_k = [&](int tl) {
    unsigned base;
    if constexpr (PAGED)
      base = tofs + kvo;
    else
      base = (unsigned)min(64 * tl, len) * CROW + kvo;
    if constexpr (KV8) {
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int tt = 0; tt < NTQ / 2; ++tt)
          kq[cb][tt] = __builtin_amdgcn_raw_buffer_load_b128(rk, (int)(base + 16 * cb * CROW + 64 * tt), 0, 0);
    } else {
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int t = 0; t < NTQ; ++t)
          kf[cb][t] = __builtin_bit_cast(tx8, buf_load16(rk, (int)(base + 16 * cb * ROW + 64 * t)));
    }
  };
  auto load_v = [&](int tl) {
    unsigned base;
    if constexpr (PAGED)
      base = tofs + vvo;
    else
      base = (unsigned)min(64 * tl, len) * CROW + vvo;
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps)
      vr[ps] = __builtin_amdgcn_raw_buffer_load_b128(rv, (int)(base + ps * RPW * CROW), 0, 0);
  };

  // WIN: a wave's first tile may be tile tlo, whose rows below kv_lo are
  // addressed past the range (zeros, not read).  (Twins of load_k / load_v, not
  // a flag on them: one generic lambda each changed the register allocation of
  // the kernels without a window, whose device code is to stay what it was.)
  [[maybe_unused]] auto load_k_first = [&](int tl) {
    unsigned base;
    if constexpr (PAGED)
      base = tofs + kvo;
    else
      base = (unsigned)min(64 * tl, len) * CROW + kvo;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const bool in = 64 * tl + 16 * cb + (int)krow >= kv_lo;
      if constexpr (KV8) {
#pragma unroll
        for (int tt = 0; tt < NTQ / 2; ++tt)
          kq[cb][tt] = __builtin_amdgcn_raw_buffer_load_b128(
              rk, in ? (int)(base + 16 * cb * CROW + 64 * tt) : kBelowWindow, 0, 0);
      } else {
#pragma unroll
        for (int t = 0; t < NTQ; ++t)
          kf[cb][t] = __builtin_bit_cast(
              tx8, buf_load16(rk, in ? (int)(base + 16 * cb * ROW + 64 * t) : kBelowWindow));
      }
    }
  };
  [[maybe_unused]] auto load_v_first = [&](int tl) {
    unsigned base;
    if constexpr (PAGED)
      base = tofs + vvo;
    else
      base = (unsigned)min(64 * tl, len) * CROW + vvo;
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps)
      vr[ps] = __builtin_amdgcn_raw_buffer_load_b128(
          rv, 64 * tl + ps * RPW + vrl >= kv_lo ? (int)(base + ps * RPW * CROW) : kBelowWindow, 0, 0);
  };

  int tile = t0 + wave;
  const int tend = tile < t1 ? t1 : tile;  // a wave with no tile loads nothing

  // Paged: tile tl lies in the pool page table[b][tl / tpp], at 64-row block
  // r = tl % tpp of head hk's part of it: tile_at() points the descriptors at
  // that part, with a range that ends at the tile's last live row, and sets
  // the loads' offset `tofs` to block r.  A wave's tiles are four apart, so
  // (page index, block) advance by (adv_pages, adv_tiles) with one carry: no
  // division in the loop.  T = the current tile, A = the next (tile + 4), B =
  // the one after (tile + 8).  B's page id is fetched (a wave-uniform scalar
  // load) while A's descriptors are built from the id fetched one iteration
  // earlier, so kv_lens -> table -> K is a dependent chain only in the
  // prologue.  Only entries of tiles below tend (pages holding a key below
  // len) are read: a tile past the piece re-reads tile T's entry and gets a
  // zero range.
  [[maybe_unused]] int jT = 0, jA = 0, rA = 0, jB = 0, rB = 0, pgA = 0;
  [[maybe_unused]] auto tile_at = [&](bool live, int tl, int pg, int r) {
    if constexpr (PAGED) {
      // a page id outside the pool: zero rows, the base stays inside the pool
      const bool ok = (unsigned)pg < (unsigned)p.num_pages;
      const int rows = live && ok ? 64 * r + min(len - 64 * tl, 64) : 0;
      const size_t off = (size_t)(ok ? pg : 0) * p.page_bytes + (size_t)hk * p.head_bytes;
      rk = make_rsrc(static_cast<const char*>(p.k) + off, rows * CROW);
      rv = make_rsrc(static_cast<const char*>(p.v) + off, rows * CROW);
      tofs = (unsigned)(64 * r) * CROW;
    }
  };
  if constexpr (PAGED) {
    typedef const __attribute__((address_space(4))) int* tab_t;  // scalar loads
    const tab_t tab = (tab_t)(p.table + (size_t)b * p.max_pages);
    int pg = 0, r = 0;
    if (tile < tend) {
      jT = tile / p.tpp;
      r = tile - jT * p.tpp;
      jA = jT + p.adv_pages, rA = r + p.adv_tiles;
      if (rA >= p.tpp) rA -= p.tpp, ++jA;
      jB = jA + p.adv_pages, rB = rA + p.adv_tiles;
      if (rB >= p.tpp) rB -= p.tpp, ++jB;
      pg = tab[jT];
      pgA = tab[tile + 4 < tend ? jA : jT];
    }
    tile_at(tile < tend, tile, pg, r);
  }
  if constexpr (WIN) {
    load_k_first(tile < tend ? tile : ntiles);
    load_v_first(tile < tend ? tile : ntiles);
  } else {
    load_k(tile < tend ? tile : ntiles);
    load_v(tile < tend ? tile : ntiles);
  }
  for (; tile < tend; tile += 4) {
    const int nxt = tile + 4 < tend ? tile + 4 : ntiles;
    if constexpr (PAGED) {
      // this tile's loads are issued: the descriptors move on to the next tile
      typedef const __attribute__((address_space(4))) int* tab_t;
      const tab_t tab = (tab_t)(p.table + (size_t)b * p.max_pages);
      const int pgB = tab[tile + 8 < tend ? jB : jT];
      tile_at(tile + 4 < tend, tile + 4, pgA, rA);
      jT = jA, jA = jB, rA = rB, pgA = pgB;
      jB += p.adv_pages, rB += p.adv_tiles;
      if (rB >= p.tpp) rB -= p.tpp, ++jB;
    }
    // S^T = K . Q^T, then the online softmax in the exp2 domain, P rounded to
    // T in the PV operand layout.  kEarlyK: every block's scores first, so the
    // next K can be issued before the softmax; else block by block (16 score
    // registers live at a time)
    const int kv0 = 64 * tile;
    const bool need_mask = WIN ? kv0 + 64 > mask_from || kv0 < mask_below : kv0 + 64 > mask_from;
    f32x4 s[NB][4];
    tx8 pf[NB][2];
    auto qk = [&](int nb) {
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int t = 0; t < NTQ; ++t)
          if constexpr (KV8)
            s[nb][cb] = Elem<T>::mfma(
                cvt_fp8x8<T>(kq[cb][t >> 1][2 * (t & 1)], kq[cb][t >> 1][2 * (t & 1) + 1]),
                qfrag(nb, t), t == 0 ? f32x4{} : s[nb][cb]);
          else
            s[nb][cb] = Elem<T>::mfma(kf[cb][t], qfrag(nb, t), t == 0 ? f32x4{} : s[nb][cb]);
    };
    auto softmax = [&](int nb) {
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        if constexpr (KV8)
          s[nb][cb] *= csc;
        else
          s[nb][cb] *= p.c;
      }
      if (need_mask) {
        if constexpr (TREE) {
          // the row's mask word, loaded here and not held across the tile loop
          // (at most two tiles of a wave come here, and the words hit in
          // cache): with base = len - sq, a draft key d = key - base >= 0 is
          // seen iff bit d is set (keys from len on have d >= sq), a prefix key
          // iff it lies inside the window of the row's position base + depth.
          // The row's token is row % sq: the block's first row by a scalar
          // division, then u < sq + 16 in fp32 ((u + 1/2) / sq is at least 1 / 32
          // away from an integer, far more than the reciprocal's error).  Nothing
          // of it is computed ahead of the loop: the scalar registers are as
          // scarce as the vector ones
          const int u = (row0 + 16 * nb) % p.sq + (lane & 15);
          const int t = u - p.sq * (int)(((float)u + 0.5f) * __builtin_amdgcn_rcpf((float)p.sq));
          const int mt = p.tree ? p.tree[(size_t)b * p.sq + t] & ((1 << p.sq) - 1) : (2 << t) - 1;
          const int depth = max(__builtin_popcount(mt) - 1, 0);
          // d of the lane's first key, kept one vector register: as a sum of
          // scalars and constants per key the tests spill scalar registers
          int d0 = kv0 + 4 * sg - (len - p.sq);
          asm volatile("" : "+v"(d0));
#pragma unroll
          for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              // pos - key = depth - d; bit 31 of the word is clear (sq <= 16)
              const int d = d0 + 16 * cb + i;
              const bool vis = d < 0 ? (unsigned)(depth - d) < (unsigned)win : (mt >> min(d, 31) & 1) != 0;
              s[nb][cb][i] = vis ? s[nb][cb][i] : ninf();
              // one key at a time: sixteen tests in flight hold thirty-two
              // scalar registers of lane masks and spill the descriptors
              asm volatile("" : "+v"(s[nb][cb][i]));
            }
        } else {
#pragma unroll
          for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if constexpr (WIN)  // lim - win <= key < lim, as one unsigned compare
                s[nb][cb][i] = (unsigned)(lim[nb] - 1 - (kv0 + 16 * cb + 4 * sg + i)) < (unsigned)win
                                   ? s[nb][cb][i]
                                   : ninf();
              else
                s[nb][cb][i] = kv0 + 16 * cb + 4 * sg + i < lim[nb] ? s[nb][cb][i] : ninf();
        }
      }
      float mx = s[nb][0][0];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int i = (cb == 0 ? 1 : 0); i < 4; ++i) mx = fmaxf(mx, s[nb][cb][i]);
      mx = max_xor32(max_xor16(mx));
      const float mnew = fmaxf(m[nb], mx);
      const float msafe = mnew == ninf() ? 0.f : mnew;  // a row that has seen no key yet
      const float alpha = __builtin_amdgcn_exp2f(m[nb] - msafe);
      m[nb] = mnew;
      // l takes the fp32 exponentials, P their rounding to T: a sum of rounded
      // P would put T's rounding (2^-9 relative for bf16) into the LSE of a
      // row with few keys
      lsum[nb] *= alpha;
#pragma unroll
      for (int e = 0; e < NE; ++e) acc[nb][e] *= alpha;
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float ex = __builtin_amdgcn_exp2f(s[nb][cb][i] - msafe);
          pf[nb][cb >> 1][4 * (cb & 1) + i] = (T)ex;
          lsum[nb] += ex;
        }
        // 16 keys at a time (with O rescaled first): this order keeps the 64-row
        // head_dim-128 variant out of scratch
        if constexpr (!kEarlyK) asm volatile("" : "+v"(lsum[nb]));
      }
    };
    if constexpr (kEarlyK) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) qk(nb);
      load_k(nxt);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) softmax(nb);
    } else {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        qk(nb);
        softmax(nb);
        asm volatile("" : "+v"(pf[nb][0]), "+v"(pf[nb][1]));  // keep the blocks apart
      }
    }

    if constexpr (!kEarlyK) load_k(nxt);
    // V tile -> the wave's image, then the next tile's V loads
    if constexpr (KV8) {
#pragma unroll
      for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          *reinterpret_cast<tx8*>(vimg + lds_off(RPW * ps + vrl, 2 * vch + j)) =
              cvt_fp8x8<T>(vr[ps][2 * j], vr[ps][2 * j + 1]);
    } else {
#pragma unroll
      for (int ps = 0; ps < NPASS; ++ps)
        *reinterpret_cast<u32x4*>(vimg + lds_off(RPW * ps + vrl, vch)) = vr[ps];
    }
    load_v(nxt);

    // O^T += V^T . P^T
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int e = 0; e < NE; ++e) {
        const int base = 8192 * u + 512 * (e >> 1) + vaddr[e & 1];
        const tx4 lo = __builtin_bit_cast(tx4, lds_read_tr(vimg, base));
        const tx4 hi = __builtin_bit_cast(tx4, lds_read_tr(vimg, base + 4096));
        const tx8 vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb][e] = Elem<T>::mfma(vf, pf[nb][u], acc[nb][e]);
      }
    }
  }

  // The epilogue's lane indices.  Paged: derived again from the thread id
  // here, not held across the loop (the 64-row head_dim-128 variant has no
  // vector register to spare for them: scratch otherwise)
  int etid = tid;
  if constexpr (PAGED) asm volatile("" : "+v"(etid));
  const int elane = etid & 63, er16 = elane & 15, eg = elane >> 4;

  // ---- merge the four waves' partials through LDS (wave order: deterministic)
  constexpr int ML_OFF = 4 * NB * NE * 1024;
  __syncthreads();  // every wave is done with its V image
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
    for (int e = 0; e < NE; ++e)
      *reinterpret_cast<f32x4*>(smem + (((wave * NB + nb) * NE + e) * 64 + elane) * 16) = acc[nb][e];
    *reinterpret_cast<float2*>(smem + ML_OFF + ((wave * NB + nb) * 64 + elane) * 8) =
        float2{m[nb], sum_xor32(sum_xor16(lsum[nb]))};
  }
  __syncthreads();
  // KV8: the cache's V scale rides on the normalisation (unsplit store and split partials alike)
  [[maybe_unused]] float vsc = 1.0f;
  if constexpr (KV8) {
    if (p.v_scale) vsc = p.v_scale[hk];
  }
  const bool split = ns > 1;
  const size_t slot = (size_t)unit * ns + piece;
  const __amdgpu_buffer_rsrc_t rso =
      make_rsrc(p.ws_o ? p.ws_o + slot * RW * HDIM : nullptr, split ? RW * HDIM * 4 : 0);
  const __amdgpu_buffer_rsrc_t rsl =
      make_rsrc(p.ws_lse ? p.ws_lse + slot * RW : nullptr, split ? RW * 4 : 0);
  float* lse_out = p.lse ? p.lse + qrow + row0 : nullptr;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    float mw[4], lw[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float2 ml = *reinterpret_cast<const float2*>(smem + ML_OFF + ((w * NB + nb) * 64 + elane) * 8);
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
    float inv = KV8 ? (L > 0.f ? 1.0f / L : 0.f) * vsc : L > 0.f ? 1.0f / L : 0.f;
    float lse2 = L > 0.f ? M + __builtin_log2f(L) : ninf();
    const int row = 16 * nb + er16;
    if constexpr (SINK) {
      // the row's sink (rows of one workgroup span several heads), folded in
      // here only when this workgroup's normalisation is the final one; a
      // piece's partial carries none of it (decode_merge_pieces adds it once)
      float sink2 = ninf();
      if (p.sinks && !split)
        sink2 = p.sinks[hk * p.group + min(row0 + row, p.rows - 1) / p.sq] * 1.4426950408889634f;
      float f, Mp;
      const float Lp = sink_fold(M, L, sink2, f, Mp);
      const float invp = Lp > 0.f ? 1.0f / Lp : 0.f;
      inv = f * (KV8 ? invp * vsc : invp);
      lse2 = Lp > 0.f ? Mp + __builtin_log2f(Lp) : ninf();
    }
#pragma unroll
    for (int ee = 0; ee < EW; ++ee) {
      const int e = wave * EW + ee;
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(smem + (((w * NB + nb) * NE + e) * 64 + elane) * 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = __builtin_fmaf(mw[w], a[j], o[j]);
      }
      o *= inv;
      if (split) {
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rso,
                                               (row * HDIM + 16 * e + 4 * eg) * 4, 0, 16);
      } else {
        tx4 out;
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = (T)o[j];
        buf_store8(ro, row * ROW + (16 * e + 4 * eg) * 2, __builtin_bit_cast(f16x4, out));
      }
    }
    if (wave == 0 && eg == 0) {
      if (split)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, lse2), rsl, row * 4, 0, 16);
      else if (lse_out && row < nrows)
        lse_out[row] = lse2 * 0.6931471805599453f;
    }
  }
  if (!split) return;

  // ---- hand the piece to the last arriver (sc1 stores, vmcnt(0) + barrier,
  // one lane's agent-scope add, sc1 loads by the workgroup whose add came last)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // every wave's stores done; the merge region is free
  volatile int* last = reinterpret_cast<volatile int*>(smem);  // the one LDS array
  if (etid == 0) {
    const unsigned old =
        __hip_atomic_fetch_add(p.ws_ctr + unit, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    *last = old == (unsigned)(ns - 1) ? 1 : 0;
  }
  __syncthreads();
  if (!*last) return;
  if constexpr (SINK)
    decode_merge_pieces<T, HDIM, NB, true>(p, unit, ns, ro, lse_out, row0, etid, p.sinks, hk);
  else
    decode_merge_pieces<T, HDIM, NB>(p, unit, ns, ro, lse_out, row0, etid);
  if (etid == 0) __hip_atomic_store(p.ws_ctr + unit, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace fa
