// Prefill attention over a K/V cache for gfx950: any number of query tokens
// per head (a prompt, or a chunk of one behind a cached prefix) against the
// cache decode reads, with grouped K/V heads (GQA / MQA), per-element key and
// query lengths read on the device, bottom-right causal alignment, and the
// four cache forms (contiguous or paged, 16-bit or FP8 E4M3).
//
//   n_b   = q_lens ? clamp(q_lens[b], 0, Sq) : Sq      valid leading query tokens
//   len_b = kv_lens ? clamp(kv_lens[b], 0, cap) : cap  keys, the chunk's own included
//   off_b = len_b - n_b                                 keys that precede the chunk
//   O[b,hq,t,:] = softmax(Q[b,hq,t,:] . K[b,hkv,0:vis,:]^T / sqrt(D)) V[b,hkv,0:vis,:],  t < n_b
//   hkv = hq / (Hq / Hkv);  vis = causal ? clamp(off_b + t + 1, 0, len_b) : len_b
//
// Unlike decode, a key tile is reused by many query rows, so K and V go
// through shared LDS: the kernel is the 4-wave tile loop of fa_fwd_kernel.hpp
// (attention_tile_loop: 128 query rows per workgroup, 32 per wave, 64-key
// tiles, register-staged double buffer, one barrier per tile) around the same
// M16 policy (Q in registers, S^T = K . Q^T and O^T = V^T . P^T on
// v_mfma_f32_16x16x32, image B for K, image A for V read with
// ds_read_b64_tr_b16, exp2-domain softmax with lazy rescale).  What differs:
//  * Workgroup = (batch element, query head, 128-row query block).  A block at
//    or past n_b returns at once; its key range is [0, causal ? min(len_b,
//    off_b + q0 + 128) : len_b).  The policy's mask compares a key with
//    qw + row: it is given qw + off_b (non-causal: a row past every key), the
//    Q loads and O stores the unshifted row.  The wave-uniform "tile lies
//    wholly above this wave's rows" skip is taken against the shifted row.
//  * The Q, O and LSE descriptors start at the block's first row and end at
//    row n_b: rows past it read as zeros and their stores are dropped by the
//    hardware range check, so nothing past n_b is written.
//  * K/V source.  Contiguous: head hkv's rows of element b, the range ending
//    at the block's last visible key.  Paged: a 64-key tile never straddles a
//    page, so the descriptor is rebuilt per tile from the block table as
//    tile_at() of fa_decode_kernel.hpp does (64-bit base, the range ending at
//    the tile's last live row, an out-of-pool id a zero range); the page id of
//    the tile after the one being loaded is fetched one tile ahead (a scalar
//    load), so the table is off the critical path.  Only entries of pages
//    holding a visible key are read.
//  * FP8 cache (KV = unsigned char): converted in staging, between the global
//    load and the LDS write; one 16-byte load is 16 elements and becomes two
//    16-byte writes into the same images (cvt_fp8x8), so the images and every
//    MFMA operand are those of the 16-bit kernel.  k_scale[hkv] rides on the
//    score scale (the policy's c), v_scale[hkv] on the final normalisation.
//    All of it sits under `if constexpr (KV8)`.
//  * bf16 keeps the fp32 score scaling (kScaleS) and takes the row sums from
//    the fp32 exponentials (M16's L32): a sum of bf16-rounded P would put
//    2^-9 relative into the LSE of a row with few keys (as in decode).
//  * Epilogue: O = acc / l (times v_scale), LSE = (m_ref + log2 l) ln 2.
#pragma once

#include "fa_decode_kernel.hpp"
#include "fa_varlen_map.hpp"

namespace fa {

// LDS of every instantiation: two buffers of one K and one V image (64 rows of
// 256-B slots each) -- what the 4-wave loop of fa_fwd_kernel.hpp uses.
constexpr int kPrefillLdsBytes = 65536;
constexpr int kPrefillBM = 128;  // query rows per workgroup

struct PrefillParams {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  float* lse;          // [B][Hq][Sq] natural-log LSE, or nullptr
  const int* kv_lens;  // device int32[B], or nullptr (= cap)
  const int* q_lens;   // device int32[B], or nullptr (= sq)
  int hq, hkv, sq, cap;
  int group;           // hq / hkv
  int nqb;             // 128-row query blocks per head
  unsigned bhk;        // batch * hkv
  int causal;
  float c;             // log2(e) / sqrt(D)
};
// the page pool and block table of fa_decode_kernel.hpp's DecodePagedParams
struct PrefillPagedParams : PrefillParams {
  const int* table;
  int max_pages;
  int num_pages;
  int tpp;                        // 64-key tiles per page
  unsigned long long page_bytes;  // Hkv * page_size * row bytes
  unsigned long long head_bytes;  // page_size * row bytes
};
struct PrefillKv8Params : PrefillParams {
  const float* k_scale;
  const float* v_scale;
};
struct PrefillPagedKv8Params : PrefillPagedParams {
  const float* k_scale;
  const float* v_scale;
};

// The packed entries (fa_prefill_varlen_*) pass their parameters as
// PrefillPacked<one of the four above>: the kernel below takes VARLEN from the
// type, so the padded entries' instantiations (and their symbols) are what
// they were.  q and o are then token-major [T][Hq][D], lse [Hq][T], and the
// fields are read as
//   q_lens = cu_seqlens (int32[B + 1], required), sq = T, nqb = B;  bhk unused
// A workgroup is (virtual block id, query head): fa_varlen_map.hpp gives it
// sequence b, its first packed row s_b and its n_b rows, and block r of b is
// query block qb = r of the padded kernel's element b -- the same tile
// sequence, so the same bits.  Q / O rows are Hq * ROW bytes apart: the
// block's descriptor starts at row s_b + q0 of head hq and ends with the last
// valid row's own ROW bytes, so the range check still zero-fills and drops
// the rows past n_b.  A global heaviest-first order of causal blocks needs the
// lengths before the launch and is not done; causal launches take the ids
// from the top instead, which starts every sequence's blocks last (most keys)
// to first at no cost.
template <class Base>
struct PrefillPacked : Base {};
template <class P>
struct PrefillIsPacked : std::false_type {};
template <class Base>
struct PrefillIsPacked<PrefillPacked<Base>> : std::true_type {};
// the packed windowed entries pass PrefillPacked<Windowed<Base>>
template <class Base>
struct ParamsWindowed<PrefillPacked<Base>> : ParamsWindowed<Base> {};
// ... and the packed sink entries PrefillPacked<Sinked<Windowed<Base>>>
template <class Base>
struct ParamsSinked<PrefillPacked<Base>> : ParamsSinked<Base> {};

// The fifth K/V source (the fa_attn_varlen_* entries): no
// cache at all, K and V token-major [T_k][Hkv][D] as Q is, the three of them
// runtime strides apart (so they may be the slices of one fused QKV buffer).
// Always packed: P = PrefillPacked<[Sinked<Windowed<]PrefillTokenKV[>>]>, and
// the fields of PrefillParams are read as
//   q_lens = cu_seqlens_q or nullptr, sq = T_q, nqb = B, cap = T_k;
//   kv_lens, bhk unused
// Sequence b's queries are the span of cu_seqlens_q (fa_varlen_map.hpp's rule,
// clamped to [0, T_q]) and its keys the span (sk_b, nk_b) of cu_k clamped to
// [0, T_k]; a nullptr stands for i * useq_q / i * useq_k (uniform lengths, the
// [B][S][H][D] layout: no array is read).  len_b := nk_b in the header's
// formulas, so the tile sequence of a block, and with it every bit of O and
// LSE, is that of the packed contiguous-cache kernel on a cache whose rows
// [0, nk_b) are the same keys.  The descriptor of tile tl starts at row
// sk_b + 64 tl of head hkv and ends with the last live row's own ROW bytes
// (as the packed Q descriptor does), the staging loads step by the runtime
// stride, O stays dense.  All of it sits under `if constexpr (TOK)`.
struct PrefillTokenKV : PrefillParams {
  const int* cu_k;           // device int32[B + 1], or nullptr (uniform)
  int useq_q, useq_k;        // the uniform lengths (read where the cu is nullptr)
  int q_sb, k_sb, v_sb;      // bytes between consecutive tokens of Q, K and V
};

// WIN (P = [PrefillPacked<]Windowed<...>[>], the fa_prefill[_varlen]_win_*
// entries; without causal the host admits W = 0 alone and the kernel applies
// no lower bound): row t of the block also masks the keys below
// off_b + t - W + 1.  The block's key range becomes [kv_lo, kv_hi) with
// kv_lo = max(0, off_b + q0 - W + 1), its first row's lower bound: the tile
// loop, the contiguous descriptors and the paged look-ahead start at tile
// tlo = kv_lo / 64, the rows of tile tlo below kv_lo are not loaded, and table
// entries of pages wholly below kv_lo are not read.  A wave skips the MFMAs of
// the tiles wholly below its lowest row's bound as it skips those above its
// rows (it still stages and takes the barrier), and the softmax reference is
// set per row (M16::softmax<.., WIN>).  All of it sits under
// `if constexpr (WIN)`: the other instantiations carry none of it.
//
// SINK (P = [PrefillPacked<]Sinked<Windowed<...>>[>], the
// fa_prefill[_varlen]_sink_* entries): all rows of a workgroup share query
// head hq, so the sink is one scalar, sink2 = sinks[hq] log2(e), folded into
// the epilogue relative to max(m_ref, sink2) (sink_fold(): m_ref is a lazy
// reference, so 2^(sink2 - m_ref) alone overflows).  sinks = nullptr or -inf:
// the factor is 1 and l' = l, the windowed kernel's bits.  fp16: a head with a
// sink takes the fp32 score scaling (M16's RTS_): a sink is compared with the
// scores on their absolute level, which fp16's rounded Q c misses by 2^-11.
template <class T, int HDIM, bool PAGED = false, class P = PrefillParams, class KV = T>
__global__ __launch_bounds__(256, 2) void fa_prefill_kernel(P p) {
  constexpr bool VARLEN = PrefillIsPacked<P>::value;
  constexpr bool WIN = ParamsWindowed<P>::value;
  constexpr bool SINK = ParamsSinked<P>::value;
  constexpr bool TOK = std::is_base_of<PrefillTokenKV, P>::value;
  static_assert(!TOK || (VARLEN && !PAGED && std::is_same<KV, T>::value),
                "token-major K/V: packed, 16-bit, no pages");
  __shared__ __attribute__((aligned(16))) char smem[kPrefillLdsBytes];
  constexpr bool KV8 = !std::is_same<KV, T>::value;
  static_assert(!KV8 || std::is_same<KV, unsigned char>::value, "the cache holds T or E4M3 bytes");
  // fp16 with sinks: whether the scores are scaled in fp32 is decided per
  // workgroup, from its head's sink (RTS, below)
  constexpr bool RTS = SINK && !std::is_same<T, __bf16>::value;
  using Pol = M16<64, T, HDIM, 2, std::is_same<T, __bf16>::value, RTS>;
  constexpr int BN = 64, WAVES = 4, RW = Pol::RW, BM = kPrefillBM;
  static_assert(WAVES * RW == BM, "four waves of 32 rows");
  constexpr int ROW = 2 * HDIM;                // bytes per Q/O row
  constexpr int CROW = KV8 ? HDIM : 2 * HDIM;  // bytes per K/V cache row
  constexpr int TILE_BYTES = BN * 256;         // LDS image: 256-B row slots at any head_dim
  static_assert(4 * TILE_BYTES == kPrefillLdsBytes, "two (K, V) buffers");
  // 16-byte loads per thread per tile (K and V each) and the tile rows the
  // workgroup covers per load instruction
  constexpr int NCH = (BN * CROW / 16) / (WAVES * 64);
  constexpr int RPP = BN / NCH;
  typedef typename Elem<T>::x8 tx8;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // workgroup -> (query block, batch, kv head, head of the group): the G query
  // heads of one K/V head and block are adjacent (they stream the same K/V),
  // causal blocks heaviest first
  const unsigned gi = blockIdx.x % (unsigned)p.group;
  const unsigned rest = blockIdx.x / (unsigned)p.group;
  unsigned bhk;
  int qb, b, hk, hq, nq;
  [[maybe_unused]] int s0 = 0;  // VARLEN: the sequence's first packed row
  if constexpr (VARLEN) {
    // (virtual block id, kv head, head of the group): the id's sequence and
    // block by bisection on cu (wave-uniform scalar loads)
    hk = (int)(rest % (unsigned)p.hkv);
    // causal: the ids are taken from the top, so each sequence's blocks start
    // in the order last (most keys) to first and the launch ends on light
    // blocks; the order BETWEEN sequences stays the packing order
    int id = (int)(rest / (unsigned)p.hkv);
    if (p.causal) id = p.sq / BM + p.nqb - 1 - id;
    if constexpr (TOK) {
      if (!varlen_block_u<BM>(p.q_lens, p.useq_q, p.nqb, p.sq, id, b, s0, nq, qb)) return;
    } else {
      if (!varlen_block<BM>(p.q_lens, p.nqb, p.sq, id, b, s0, nq, qb)) return;
    }
    b = __builtin_amdgcn_readfirstlane(b);
    s0 = __builtin_amdgcn_readfirstlane(s0);
    nq = __builtin_amdgcn_readfirstlane(nq);
    qb = __builtin_amdgcn_readfirstlane(qb);
    bhk = (unsigned)b * (unsigned)p.hkv + (unsigned)hk;
    hq = hk * p.group + (int)gi;
  } else {
    bhk = rest % p.bhk;
    const int qbr = (int)(rest / p.bhk);
    qb = p.causal ? p.nqb - 1 - qbr : qbr;
    b = (int)(bhk / (unsigned)p.hkv), hk = (int)(bhk - (unsigned)b * p.hkv);
    hq = hk * p.group + (int)gi;
    nq = p.q_lens ? p.q_lens[b] : p.sq;
    nq = __builtin_amdgcn_readfirstlane(min(max(nq, 0), p.sq));
  }
  const int q0 = qb * BM;
  if (q0 >= nq) return;  // nothing of this block is valid: nothing is written
  int len;
  [[maybe_unused]] int sk = 0;  // TOK: the sequence's first key row
  if constexpr (TOK) {
    // the keys' span: one more pair of scalar loads (uniform mode: none)
    sk = varlen_start(p.cu_k, p.useq_k, p.cap, b);
    len = max(varlen_start(p.cu_k, p.useq_k, p.cap, b + 1), sk) - sk;
    sk = __builtin_amdgcn_readfirstlane(sk);
    len = __builtin_amdgcn_readfirstlane(len);
  } else {
    len = p.kv_lens ? p.kv_lens[b] : p.cap;
    len = __builtin_amdgcn_readfirstlane(min(max(len, 0), p.cap));
  }
  const int off = len - nq;  // keys before the chunk (negative: the leading rows see nothing)
  const int kv_hi = p.causal ? max(0, min(len, off + q0 + BM)) : len;
  const int ntiles = (kv_hi + BN - 1) / BN;
  // WIN: the first key any row of the block sees (<= kv_hi: off + q0 < len),
  // its tile, and the rows of that tile that lie below it
  [[maybe_unused]] int win = 0, kv_lo = 0, tlo = 0, lo_in = 0;
  if constexpr (WIN) {
    // not causal (the host lets only W = 0 through): no lower bound, as no
    // upper one -- a window past every row - key difference, so the mask,
    // need_mask and the skip below are the plain kernel's
    win = p.causal ? p.window : 0x7fffffff;
    kv_lo = p.causal ? max(0, off + q0 - win + 1) : 0;
    tlo = kv_lo / BN;
    lo_in = kv_lo - BN * tlo;
  }
  // the row the mask compares keys with; non-causal: past every key
  const int qwm = p.causal ? off + q0 + wave * RW : 0x3fffffff;
  const int qwl = wave * RW;  // this wave's first row within the block's descriptors

  // qrow0: the block's first row in units of ROW bytes (Q, O) and, as lrow0,
  // of LSE floats; qs: bytes between its consecutive rows
  size_t qrow0, lrow0;
  int qrows, qs;
  if constexpr (VARLEN) {
    qrow0 = ((size_t)s0 + q0) * (size_t)p.hq + hq;
    lrow0 = (size_t)hq * (size_t)p.sq + s0 + q0;
    qrows = min(nq - q0, BM);
    qs = p.hq * ROW;
  } else {
    qrow0 = lrow0 = ((size_t)b * p.hq + hq) * (size_t)p.sq + q0;
    qrows = nq - q0;  // valid rows from the block's first on (may exceed 128)
    qs = ROW;
  }
  // the range ends with the last valid row's own bytes (VARLEN: <= 127 * Hq *
  // ROW + ROW, which the host checks fits)
  // TOK: Q rows are the runtime stride apart (qsq; <= 127 * qsq + ROW fits, the
  // host's check), O rows stay dense (qs)
  [[maybe_unused]] int qsq = 0;
  __amdgpu_buffer_rsrc_t rq;
  if constexpr (TOK) {
    qsq = p.q_sb;
    rq = make_rsrc(static_cast<const char*>(p.q) + ((size_t)s0 + q0) * (size_t)qsq + (size_t)hq * ROW,
                   (qrows - 1) * qsq + ROW);
  } else {
    rq = make_rsrc(static_cast<const char*>(p.q) + qrow0 * ROW,
                   VARLEN ? (qrows - 1) * qs + ROW : qrows * ROW);
  }
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(static_cast<char*>(p.o) + qrow0 * ROW,
                                              VARLEN ? (qrows - 1) * qs + ROW : qrows * ROW);

  // score scale: the cache's K scale rides on it (a wave-uniform load)
  float csc = p.c;
  [[maybe_unused]] float vsc = 1.0f;
  if constexpr (KV8) {
    if (p.k_scale) csc *= p.k_scale[hk];
    if (p.v_scale) vsc = p.v_scale[hk];
  }

  // SINK: the head's sink in log2 units (a wave-uniform load)
  [[maybe_unused]] float sink2 = ninf();
  if constexpr (SINK) {
    if (p.sinks) sink2 = p.sinks[hq] * 1.4426950408889634f;
  }
  Pol pol;
  pol.init(lane, csc);
  // RTS: a head with a sink scales its fp32 scores by c, as the bf16 kernels
  // do, instead of rounding Q c to fp16 (2^-11 of every score: an offset that
  // cancels in O without a sink and weighs the sink wrongly beside one); a
  // head without one (-inf, or sinks == nullptr) keeps the windowed kernel's
  // arithmetic and so its bits
  if constexpr (RTS) pol.scale_s_rt = sink2 != ninf();
  // scaled once tile 0's loads are in flight
  if constexpr (TOK)
    pol.issue_q(rq, qwl, qsq);
  else
    pol.issue_q(rq, qwl, qs);

  // Staging.  16-bit: the policy's lanes (K natural row-major, V two rows of
  // opposite parity x 4 chunks per 8 lanes).  FP8: a lane holds a 16-byte
  // piece (16 elements) that becomes chunks 2 piece and 2 piece + 1 of its
  // row's slot; per 8 lanes K takes two rows of opposite parity x 4 pieces and
  // V the lanes of fa_decode_kernel.hpp's FP8 V staging, so each of the two
  // writes of 8 consecutive lanes covers the 8 distinct 16-B slots of a bank
  // row in image B / image A.
  int kr0, kc, vr0, vc;
  if constexpr (KV8) {
    if constexpr (HDIM == 128) {
      kr0 = 8 * wave + ((lane >> 2) & 1) + 2 * ((lane >> 4) & 3);
      kc = (lane & 3) + 4 * ((lane >> 3) & 1);
      vr0 = 8 * wave + ((lane >> 1) & 1) + 2 * ((lane >> 5) & 1) + 4 * ((lane >> 2) & 1);
      vc = (lane & 1) + 2 * ((lane >> 3) & 3);
    } else {
      kr0 = 16 * wave + ((lane >> 2) & 1) + 2 * ((lane >> 3) & 7);
      kc = lane & 3;
      vr0 = 16 * wave + ((lane >> 1) & 1) + 2 * ((lane >> 4) & 1) + 4 * ((lane >> 2) & 1) +
            8 * ((lane >> 5) & 1);
      vc = (lane & 1) + 2 * ((lane >> 3) & 1);
    }
  } else {
    kr0 = pol.k_stage_row(wave), kc = pol.k_stage_ch();
    vr0 = pol.v_stage_row(wave), vc = pol.v_stage_ch();
  }
  static_assert(KV8 || RPP == Pol::RPW * WAVES, "the policy's staging covers RPW rows per wave");
  // TOK: the rows of a tile are ksb (K) and vsb (V) bytes apart
  [[maybe_unused]] int ksb = 0, vsb = 0;
  int kvo, vvo;
  if constexpr (TOK) {
    ksb = p.k_sb, vsb = p.v_sb;
    kvo = kr0 * ksb + kc * 16, vvo = vr0 * vsb + vc * 16;
  } else {
    kvo = kr0 * CROW + kc * 16, vvo = vr0 * CROW + vc * 16;
  }

  // The descriptors of the tile whose loads are issued next: its 64 rows start
  // at the base and the range ends at its last visible row (a tile past the
  // range: zero bytes, no memory traffic).
  const char *Kh, *Vh;
  if constexpr (TOK) {
    // head hk's part of the sequence's first key row
    Kh = static_cast<const char*>(p.k) + (size_t)sk * (size_t)ksb + (size_t)hk * ROW;
    Vh = static_cast<const char*>(p.v) + (size_t)sk * (size_t)vsb + (size_t)hk * ROW;
  } else {
    const size_t kvoff = PAGED ? 0 : (size_t)bhk * (size_t)p.cap * CROW;
    Kh = static_cast<const char*>(p.k) + kvoff;
    Vh = static_cast<const char*>(p.v) + kvoff;
  }
  __amdgpu_buffer_rsrc_t rk, rv;
  // pg: the tile's pool page, r: its 64-row block within head hk's part of the page (paged only)
  auto tile_at = [&](int tl, [[maybe_unused]] int pg, [[maybe_unused]] int r) {
    const int live = max(0, min(kv_hi - BN * tl, BN));
    if constexpr (PAGED) {
      // a page id outside the pool: zero rows, the base stays inside the pool
      const bool ok = (unsigned)pg < (unsigned)p.num_pages;
      const size_t o = (size_t)(ok ? pg : 0) * p.page_bytes + (size_t)hk * p.head_bytes +
                       (size_t)(BN * r) * CROW;
      rk = make_rsrc(Kh + o, ok ? live * CROW : 0);
      rv = make_rsrc(Vh + o, ok ? live * CROW : 0);
    } else if constexpr (TOK) {
      // the range ends with the last live row's own ROW bytes: a lane's 16
      // bytes of row r lie inside it iff r < live, whatever the strides (>=
      // Hkv * ROW, the host's check); <= 63 * stride + ROW fits (the same)
      const size_t r0 = (size_t)min(BN * tl, kv_hi);
      rk = make_rsrc(Kh + r0 * (size_t)ksb, live > 0 ? (live - 1) * ksb + ROW : 0);
      rv = make_rsrc(Vh + r0 * (size_t)vsb, live > 0 ? (live - 1) * vsb + ROW : 0);
    } else {
      // a tile past the range keeps the base inside the cache (tl <= ntiles)
      const size_t o = (size_t)min(BN * tl, kv_hi) * CROW;
      rk = make_rsrc(Kh + o, live * CROW);
      rv = make_rsrc(Vh + o, live * CROW);
    }
  };
  u32x4 kst[NCH], vst[NCH];
  auto issue_loads = [&]() {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      if constexpr (TOK) {
        kst[i] = __builtin_amdgcn_raw_buffer_load_b128(rk, kvo + RPP * i * ksb, 0, 0);
        vst[i] = __builtin_amdgcn_raw_buffer_load_b128(rv, vvo + RPP * i * vsb, 0, 0);
      } else {
        kst[i] = __builtin_amdgcn_raw_buffer_load_b128(rk, kvo + RPP * i * CROW, 0, 0);
        vst[i] = __builtin_amdgcn_raw_buffer_load_b128(rv, vvo + RPP * i * CROW, 0, 0);
      }
    }
  };
  // WIN, tile tlo (the prologue's): its rows below kv_lo are addressed past
  // the range, so they come as zeros (a masked P = 0 meets a finite V) and
  // are not read.  (A twin of issue_loads, not a flag on it: folding the two
  // into one generic lambda changed the register allocation of the kernels
  // without a window, whose device code is to stay what it was.)
  [[maybe_unused]] auto issue_loads_first = [&]() {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      if constexpr (TOK) {
        kst[i] = __builtin_amdgcn_raw_buffer_load_b128(
            rk, kr0 + RPP * i >= lo_in ? kvo + RPP * i * ksb : kBelowWindow, 0, 0);
        vst[i] = __builtin_amdgcn_raw_buffer_load_b128(
            rv, vr0 + RPP * i >= lo_in ? vvo + RPP * i * vsb : kBelowWindow, 0, 0);
      } else {
        kst[i] = __builtin_amdgcn_raw_buffer_load_b128(
            rk, kr0 + RPP * i >= lo_in ? kvo + RPP * i * CROW : kBelowWindow, 0, 0);
        vst[i] = __builtin_amdgcn_raw_buffer_load_b128(
            rv, vr0 + RPP * i >= lo_in ? vvo + RPP * i * CROW : kBelowWindow, 0, 0);
      }
    }
  };
  auto write_lds = [&](char* kb) {
    char* vb = kb + TILE_BYTES;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      if constexpr (KV8) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          *reinterpret_cast<tx8*>(kb + Pol::k_lds(kr0 + RPP * i, 2 * kc + j)) =
              cvt_fp8x8<T>(kst[i][2 * j], kst[i][2 * j + 1]);
          *reinterpret_cast<tx8*>(vb + Pol::v_lds(vr0 + RPP * i, 2 * vc + j)) =
              cvt_fp8x8<T>(vst[i][2 * j], vst[i][2 * j + 1]);
        }
      } else {
        *reinterpret_cast<u32x4*>(kb + Pol::k_lds(kr0 + RPP * i, kc)) = kst[i];
        *reinterpret_cast<u32x4*>(vb + Pol::v_lds(vr0 + RPP * i, vc)) = vst[i];
      }
    }
  };

  // Paged: pgN / rN are the page id and block of the tile loaded next, (jF,
  // rF) the table index and block of the tile after it, whose id is fetched
  // while the next tile's loads are in flight.  Only tiles below ntiles
  // (pages holding a visible key) have their entries read.
  [[maybe_unused]] int pgN = 0, rN = 0, jF = 0, rF = 0;
  typedef const __attribute__((address_space(4))) int* tab_t;  // scalar loads
  [[maybe_unused]] tab_t tab = nullptr;
  if constexpr (PAGED) {
    tab = (tab_t)(p.table + (size_t)b * p.max_pages);
    if constexpr (WIN) {
      // the same state, started at tile tlo (any block of its page)
      const int j0 = tlo / p.tpp, j1 = (tlo + 1) / p.tpp;
      const int pg0 = ntiles > tlo ? tab[j0] : 0;
      tile_at(tlo, pg0, tlo - j0 * p.tpp);
      rN = tlo + 1 - j1 * p.tpp;
      pgN = ntiles > tlo + 1 ? tab[j1] : 0;
      jF = (tlo + 2) / p.tpp, rF = tlo + 2 - jF * p.tpp;
    } else {
      const int pg0 = ntiles > 0 ? tab[0] : 0;
      tile_at(0, pg0, 0);
      rN = p.tpp > 1 ? 1 : 0;
      pgN = ntiles > 1 ? tab[p.tpp > 1 ? 0 : 1] : 0;
      jF = 2 / p.tpp, rF = 2 - jF * p.tpp;
    }
  } else {
    tile_at(WIN ? tlo : 0, 0, 0);
  }

  // prologue: unconditional, so every earlier load (Q included) has retired
  // before the loop and no in-loop MFMA waits on the prefetch
  if constexpr (WIN)
    issue_loads_first();
  else
    issue_loads();
  // every prologue load is issued before the first VALU that waits on one
  // (else the scheduler hoists Q's scaling above the K/V loads)
  __builtin_amdgcn_sched_barrier(0);
  pol.scale_q();
  write_lds(smem);
  // vmcnt(0): else the compiler's waitcnt analysis keeps Q "pending" at the
  // loop header and every iteration's first MFMAs wait for the prefetch
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();

  auto step = [&](int j, auto buf_c) {
    constexpr int BUF = decltype(buf_c)::value;
    char* kb = smem + BUF * 2 * TILE_BYTES;
    char* kb_next = smem + (BUF ^ 1) * 2 * TILE_BYTES;
    const int kv0 = j * BN;
    tile_at(j + 1, pgN, rN);
    issue_loads();  // past kv_hi: zero bytes, no memory traffic
    if constexpr (PAGED) {
      if (j + 2 < ntiles) pgN = tab[jF];
      rN = rF;
      if (++rF == p.tpp) rF = 0, ++jF;
    }
    // wave-uniform: does any key of this tile lie at/below some row of this wave?
    if constexpr (WIN) {
      // ... and at/above the lower bound of some row of this wave?  The mask
      // is also needed where a key lies below the wave's highest lower bound
      if (kv0 <= qwm + RW - 1 && kv0 + BN - 1 > qwm - win) {
        const bool need_mask =
            (kv0 + BN > kv_hi) || (kv0 + BN - 1 > qwm) || (kv0 < qwm + RW - win);
        pol.template tile<true, true>(kb, kb + TILE_BYTES, kv0, kv_hi, qwm, csc, need_mask, win);
      }
    } else if (kv0 <= qwm + RW - 1) {
      const bool need_mask = (kv0 + BN > kv_hi) || (kv0 + BN - 1 > qwm);
      pol.template tile<true>(kb, kb + TILE_BYTES, kv0, kv_hi, qwm, csc, need_mask);
    }
    write_lds(kb_next);
    __syncthreads();
  };
  int j = WIN ? tlo : 0;
  for (; j + 1 < ntiles; j += 2) {
    step(j, std::integral_constant<int, 0>{});
    step(j + 1, std::integral_constant<int, 1>{});
  }
  if (j < ntiles) step(j, std::integral_constant<int, 0>{});

  if constexpr (SINK) {
    pol.template store_o<0, Pol::QB, 0, Pol::NE / 2, true>(ro, qwl, vsc, qs, sink2);
  } else {
    pol.store_o(ro, qwl, vsc, qs);
  }
  if (p.lse) {
    const __amdgpu_buffer_rsrc_t rl = make_rsrc(p.lse + lrow0, qrows * 4);
#pragma unroll
    for (int bb = 0; bb < Pol::QB; ++bb) {
      float l = pol.row_sum(bb);
      float mr = pol.m_ref[bb];
      if constexpr (SINK) {
        float f;
        l = sink_fold(pol.m_ref[bb], l, sink2, f, mr);
      }
      const float lse = l > 0.f ? (mr + __builtin_log2f(l)) * 0.6931471805599453f : ninf();
      if (pol.g == 0)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, lse), rl,
                                              (qwl + 16 * bb + pol.r16) * 4, 0, 0);
    }
  }
}

}  // namespace fa
