/*
 * fa_mi355x.h -- C ABI of the MI355X (gfx950) flash-attention forward path.
 *
 * This is the drop-in boundary for the reference's host dispatcher
 *   void flash_attention_v9_dispatch(const half* Q, const half* K,
 *       const half* V, half* Output, float* splitk_buf_O,
 *       float* splitk_buf_ml, int batch_size, int num_heads, int seq_len,
 *       int head_dim, bool causal, cudaStream_t stream = 0)
 * (/root/reference/flash_attention.cu:606-663).  The C++ signature itself is
 * kept in flash_attention_v9.h and forwards here.
 *
 * Conventions shared by every entry point:
 *  - q, k, v, o are DEVICE pointers owned by the caller (the reference
 *    allocates them in main, :772-787), fp16 (IEEE binary16), layout BHSD:
 *    [batch*heads][seq_len][head_dim] contiguous, bh stride seq_len*head_dim
 *    (:119-122, :672-675).
 *  - Stream-ordered and non-blocking: the call enqueues on hip_stream (a
 *    hipStream_t, NULL = default stream) and returns; no allocation, no
 *    synchronisation, safe to capture into a hipGraph.
 *  - Return value: FA_OK (0) or a nonzero fa_status_t.  The reference's
 *    equivalent is CUDA_CHECK(cudaGetLastError()) -> exit (:22-30, :662);
 *    flash_attention_v9_dispatch() keeps that behaviour on top of this ABI.
 */
#ifndef FA_MI355X_H
#define FA_MI355X_H

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  FA_OK = 0,
  FA_ERR_NULL_POINTER = 1,        /* q/k/v/o NULL with a non-empty problem */
  FA_ERR_UNSUPPORTED_HEAD_DIM = 2,/* head_dim not 128 (ref :613 HD=128) or 64 */
  FA_ERR_BAD_SHAPE = 3,           /* negative sizes, int overflow of B*H, or
                                     seq_len*2*head_dim (split-KV: *4) past
                                     INT_MAX: S <= 8388607 at head_dim 128 */
  FA_ERR_LAUNCH = 4,              /* hipGetLastError() after the launch */
  FA_ERR_BAD_CONFIG = 5,          /* config id out of range / wrong causal */
  FA_ERR_HIP = 6,                 /* other HIP runtime failure */
  FA_ERR_WORKSPACE = 7            /* split-KV buffers / workspace missing or short */
} fa_status_t;

/* Tile configuration descriptor (the reference's template switches
 * BLOCK_M/BLOCK_N/NWARPS/IS_CAUSAL, :67-70, re-expressed for 64-wide waves). */
typedef struct {
  int id;
  int block_m;      /* query rows per workgroup */
  int block_n;      /* key/value rows per LDS tile */
  int waves;        /* 64-lane wavefronts per workgroup */
  int causal;       /* 1 = causal instantiation */
  int split_kv;     /* 1 = writes fp32 partials for the LSE merge */
  int lds_bytes;    /* dynamic LDS per workgroup */
  const char* name;
  int dtype;        /* FA_DTYPE_F16 or FA_DTYPE_BF16: element type of Q/K/V/O */
  int head_dim;     /* 128 (the reference's) or 64 */
} fa_config_info_t;

enum { FA_DTYPE_F16 = 0, FA_DTYPE_BF16 = 1 };

/* Per-config compiled resource usage: the reference's register/occupancy
 * report (cudaFuncGetAttributes + cudaOccupancyMaxActiveBlocksPerMultiprocessor,
 * :711-755).  Requires a visible GPU for the occupancy field. */
typedef struct {
  int num_regs;           /* arch VGPRs per lane (hipFuncAttributes.numRegs) */
  int local_size_bytes;   /* scratch (spill) bytes per lane */
  int shared_size_bytes;  /* static LDS */
  int max_threads_per_block;
  int blocks_per_cu;      /* occupancy query at the config's LDS size; -1 if no GPU */
} fa_kernel_attrs_t;

/* Main entry: fused QK^T -> online softmax -> PV forward, fp16 in/out,
 * fp32 accumulate, scale = 1/sqrt(head_dim) (ref :612).  Chooses the tile
 * config with fa_select_config(). Replaces flash_attention_v9_dispatch
 * (flash_attention.cu:606-663). */
int fa_fwd_f16(const void* q, const void* k, const void* v, void* o,
               int batch, int heads, int seq_len, int head_dim, int causal,
               void* hip_stream);

/* Same, forcing one tile config (used to report each (BM,BN,waves) config,
 * as the reference's bench labels its tiers, :905-916).  The config's causal
 * flag must equal `causal`. */
int fa_fwd_f16_config(const void* q, const void* k, const void* v, void* o,
                      int batch, int heads, int seq_len, int head_dim,
                      int causal, int config_id, void* hip_stream);

/* bf16 in/out (fp32 accumulate, P rounded to bf16 before PV): the same
 * kernels on v_mfma_f32_16x16x32_bf16.  Not in the reference (fp16 only,
 * :613); SURVEY.md §8(f) rank 4.  fa_fwd_bf16 uses the bf16 twin of
 * fa_select_config()'s tier; fa_fwd_bf16_config accepts bf16 configs only
 * (fa_config_info().dtype == FA_DTYPE_BF16), fa_fwd_f16_config fp16 only. */
int fa_fwd_bf16(const void* q, const void* k, const void* v, void* o,
                int batch, int heads, int seq_len, int head_dim, int causal,
                void* hip_stream);
int fa_fwd_bf16_config(const void* q, const void* k, const void* v, void* o,
                       int batch, int heads, int seq_len, int head_dim,
                       int causal, int config_id, void* hip_stream);

/* Split-KV (flash-decoding) forward: the reference's dead IS_SPLITK path
 * (:169-180, :460-496) and its merge kernel flash_attention_splitk_merge
 * (:559-598), made live.  Buffers use the reference's layout:
 *   part_o  fp32 [num_splits][batch*heads][seq_len][head_dim]  (unnormalised O)
 *   part_ml fp32 [num_splits][batch*heads][seq_len][2]          (m, l) per row,
 *           m = running max of the scaled scores (natural-log units, as the
 *           reference's m_i), l = running sum; an empty split writes (-inf, 0).
 * num_splits <= 0 uses fa_splitkv_num_splits().  Device buffers are owned by
 * the caller and must hold fa_splitkv_o_bytes()/fa_splitkv_ml_bytes(). */
int fa_fwd_f16_splitkv(const void* q, const void* k, const void* v, void* o,
                       int batch, int heads, int seq_len, int head_dim,
                       int causal, int num_splits, float* part_o,
                       float* part_ml, void* hip_stream);
int fa_splitkv_num_splits(int batch, int heads, int seq_len, int causal);
unsigned long long fa_splitkv_o_bytes(int batch, int heads, int seq_len,
                                      int head_dim, int num_splits);
unsigned long long fa_splitkv_ml_bytes(int batch, int heads, int seq_len,
                                       int head_dim, int num_splits);

/* Workspace forward: fa_fwd_f16 / fa_fwd_bf16 plus a caller-owned device
 * workspace that lets causal launches short of the persistent tier split each
 * 256-row query block's key range into pieces run by separate workgroups and
 * merge them in the same launch (the reference's split-K log-sum-exp merge,
 * :559-598, without its second kernel; fp16 / bf16 normalised partial rows
 * plus an fp32 log2-sum-exp per row).
 *   piece_tiles = 0: the dispatcher's choice -- fa_fwd_split_pieces() is its
 *     piece length in 64-key tiles, 0 when it does not split this shape (the
 *     _ws entries then run the tier fa_fwd_f16 / fa_fwd_bf16 runs; on the
 *     persistent W4 tier with >= 64 rounds of items per XCD (the B=64
 *     headline) the workspace's counter region also carries a cross-XCD tail
 *     pool: the last 1/16 of every XCD's items are claimed at run time, which
 *     evens out XCDs that run a few % slower -- bit-identical output);
 *   piece_tiles > 0: that piece length (causal, head_dim 128, at most 8
 *     pieces per query block, else FA_ERR_BAD_CONFIG).
 * fa_fwd_ws_bytes() is the workspace the call needs (0: neither a split nor
 * a tail pool; 65536: the tail pool's counters only).  Its first 64 KB
 * (counters, the same place for every shape) must be zero before the first
 * use; every launch returns the counters it used to zero, so one buffer of
 * the largest size needed serves any sequence of shapes on ONE stream
 * (launches on different streams need their own).  A counter region that is
 * not zero (a fresh buffer never cleared, or one shared by two streams at
 * once) is not detected: pool items can be skipped and their rows left
 * unwritten, and the split merge can run early.  The workspace must be
 * 16-byte aligned (any hipMalloc / torch allocation is): FA_ERR_WORKSPACE if
 * the call splits and workspace is NULL, misaligned or ws_bytes is short; a
 * tail-pool shape with no, a short or a misaligned (not 8-byte) workspace
 * runs the static item order.  The reference-signature wrapper
 * flash_attention_v9_dispatch (flash_attention_v9.h) owns such a workspace
 * per (device, stream), so it runs the same tiers as these entries. */
unsigned long long fa_fwd_ws_bytes(int batch, int heads, int seq_len, int head_dim,
                                   int causal, int piece_tiles);
int fa_fwd_split_pieces(int batch, int heads, int seq_len, int head_dim, int causal);
int fa_fwd_f16_ws(const void* q, const void* k, const void* v, void* o,
                  int batch, int heads, int seq_len, int head_dim, int causal,
                  int piece_tiles, void* workspace, unsigned long long ws_bytes,
                  void* hip_stream);
int fa_fwd_bf16_ws(const void* q, const void* k, const void* v, void* o,
                   int batch, int heads, int seq_len, int head_dim, int causal,
                   int piece_tiles, void* workspace, unsigned long long ws_bytes,
                   void* hip_stream);

/* Decode attention over a K/V cache: a few query tokens per head (1 for
 * decoding, up to 16 for speculative / multi-token decoding) against a long
 * cache whose length differs per batch element, with grouped K/V heads (GQA /
 * MQA: heads_q % heads_kv == 0, any integer group size).
 *   O[b,hq,t,:] = softmax(Q[b,hq,t,:] . K[b,hkv,0:len_b,:]^T / sqrt(D) [+ mask])
 *                 . V[b,hkv,0:len_b,:],          hkv = hq / (heads_q / heads_kv)
 *   q, o   [batch][heads_q][seqlen_q][head_dim]           (1 <= seqlen_q <= 16)
 *   k, v   [batch][heads_kv][kv_capacity][head_dim]       (the cache, BHSD)
 *   kv_lens DEVICE int32[batch], len_b <= kv_capacity (clamped to it); NULL =
 *           every len_b is kv_capacity.  Read by the kernel, so the call stays
 *           sync-free and a captured graph follows lengths changed between
 *           replays.  Rows past len_b are never read (they may hold anything).
 *   causal = 1: bottom-right aligned, query token t sees keys <= len_b -
 *           seqlen_q + t; 0: all len_b keys.  A row that sees no key writes
 *           zeros and LSE = -inf.
 *   lse    optional fp32 [batch][heads_q][seqlen_q]: natural log of the sum of
 *           exp of the scaled scores; may be NULL.
 * The heads_q / heads_kv * seqlen_q query rows that share a K/V head are one
 * workgroup's rows (64 at most, else several row groups), so each K/V byte is
 * read once per row group.  The key range [0, len_b) is cut into num_splits
 * pieces inside the kernel and the pieces are merged in the same launch, in
 * piece order (bit-deterministic):
 *   num_splits = 0: the plan's choice, fa_decode_num_splits() (from the shape
 *     and the current device's CU count; 256 if the query fails);
 *   num_splits > 0: that many; more than the plan's upper cap (64) is
 *     FA_ERR_BAD_CONFIG.
 * Workspace: same contract as fa_fwd_f16_ws -- the first 64 KB are counters,
 * zero before the first use, and every launch returns the counters it used to
 * zero, so one buffer of the largest size needed serves any sequence of decode
 * AND forward shapes on ONE stream.  fa_decode_ws_bytes() is what the call
 * needs (num_splits as passed to the call; 0 when it does not split: no
 * workspace is touched then and NULL is accepted).  FA_ERR_WORKSPACE if the
 * call splits and workspace is NULL, short or not 16-byte aligned.
 * All argument errors are returned before any launch.  Empty problems (batch
 * or heads of 0) return FA_OK without launching; kv_capacity == 0 with rows
 * present only fills O with zeros and LSE with -inf.  fa_decode_* are not
 * tile configs: fa_config_info() does not list them. */
int fa_decode_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                  int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                  int head_dim, const int* kv_lens, int causal, int num_splits,
                  void* workspace, unsigned long long ws_bytes, void* hip_stream);
int fa_decode_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                   int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                   int head_dim, const int* kv_lens, int causal, int num_splits,
                   void* workspace, unsigned long long ws_bytes, void* hip_stream);
int fa_decode_num_splits(int batch, int heads_q, int heads_kv, int seqlen_q,
                         int kv_capacity, int head_dim);
unsigned long long fa_decode_ws_bytes(int batch, int heads_q, int heads_kv, int seqlen_q,
                                      int kv_capacity, int head_dim, int num_splits);

/* Decode attention over a PAGED K/V cache: fa_decode_* with the cache held as
 * a pool of fixed-size pages plus a per-sequence block table (the layout of
 * the serving stacks), so sequences grow, finish and share prefixes without
 * the cache being gathered first.
 *   q, o      [batch][heads_q][seqlen_q][head_dim]          (1 <= seqlen_q <= 16)
 *   k_pages, v_pages  [num_pages][heads_kv][page_size][head_dim], contiguous:
 *             BHSD inside each page (the serving stacks' "HND" page layout).
 *   page_size any positive multiple of 64 (64, 128, 192, ...: a 64-key tile
 *             never straddles two pages), page_size * 2 * head_dim <= INT_MAX.
 *   block_table DEVICE int32[batch][max_pages_per_seq], row-major: entry j of
 *             row b is the pool page holding keys [j * page_size, (j + 1) *
 *             page_size) of batch element b.  Pages may be shared between
 *             batch elements and listed more than once.
 *   kv_lens   DEVICE int32[batch], clamped to the logical capacity
 *             kv_capacity := max_pages_per_seq * page_size; NULL = that
 *             capacity for every element.
 * Everything else (causal, lse, GQA, row groups, num_splits, the workspace)
 * is as for fa_decode_* with that kv_capacity: num_splits = 0 takes
 * fa_decode_num_splits(batch, heads_q, heads_kv, seqlen_q, kv_capacity,
 * head_dim), the workspace is fa_decode_ws_bytes(..., kv_capacity, head_dim,
 * num_splits), and one per-stream workspace serves paged decode, contiguous
 * decode and forward launches in any order.
 * The kernel is the contiguous one with a per-tile descriptor: the same
 * workgroups, tiles, order of operations and merges.  For the same data and
 * the same num_splits, O and LSE are BIT-IDENTICAL to fa_decode_* run on the
 * gathered [batch][heads_kv][kv_capacity][head_dim] cache.
 * What is read: only the table entries of pages that hold a key below len_b,
 * and of those pages only the rows below len_b.  Entries past that, rows past
 * the length in the last page and unmapped pages may hold anything (NaN bit
 * patterns included); they never reach O.
 * Nothing is validated on the host (the call stays sync-free and
 * graph-capturable: table and lengths may change between replays).  A page id
 * outside [0, num_pages) in an entry that is read touches no memory: that
 * tile reads as zero rows, the batch element's output is unspecified but
 * finite, every other element is unaffected.
 * Argument errors, returned before any launch: page_size not a positive
 * multiple of 64 (or past the byte range above), num_pages <= 0,
 * max_pages_per_seq < 0 or kv_capacity > INT_MAX - 64: FA_ERR_BAD_SHAPE;
 * block_table (or q, k_pages, v_pages, o) NULL with kv_capacity > 0:
 * FA_ERR_NULL_POINTER; head_dim, seqlen_q, heads_q % heads_kv, num_splits and
 * the workspace as for fa_decode_*.  Empty problems (batch or heads of 0)
 * return FA_OK without launching; kv_capacity == 0 (max_pages_per_seq == 0)
 * with rows present only fills O with zeros and LSE with -inf. */
int fa_decode_paged_f16(const void* q, const void* k_pages, const void* v_pages, void* o, float* lse,
                        int batch, int heads_q, int heads_kv, int seqlen_q, int head_dim,
                        int num_pages, int page_size, const int* block_table, int max_pages_per_seq,
                        const int* kv_lens, int causal, int num_splits,
                        void* workspace, unsigned long long ws_bytes, void* hip_stream);
int fa_decode_paged_bf16(const void* q, const void* k_pages, const void* v_pages, void* o, float* lse,
                         int batch, int heads_q, int heads_kv, int seqlen_q, int head_dim,
                         int num_pages, int page_size, const int* block_table, int max_pages_per_seq,
                         const int* kv_lens, int causal, int num_splits,
                         void* workspace, unsigned long long ws_bytes, void* hip_stream);

/* Decode attention over an FP8 K/V cache: fa_decode_* and fa_decode_paged_*
 * with K and V stored as OCP FP8 E4M3 (torch.float8_e4m3fn: one byte per
 * element, no infinities, 0x7f / 0xff = NaN) and one fp32 scale per K/V head
 * for K and one for V.  q and o stay fp16 (_f16) or bf16 (_bf16):
 *   O[b,hq,t,:] = softmax(Q . (k_scale[hkv] * K8)^T / sqrt(D) [+ mask])
 *                 (v_scale[hkv] * V8)
 *   k, v      [batch][heads_kv][kv_capacity][head_dim] bytes, contiguous;
 *   k_pages, v_pages  [num_pages][heads_kv][page_size][head_dim] bytes.
 *   k_scale, v_scale  DEVICE float[heads_kv], or NULL (= 1.0 for every head).
 *             Device arrays so that nothing syncs: a captured graph follows
 *             values rewritten between replays.  A per-tensor scale is the
 *             array filled with one value.
 * Every other argument, the status codes, the order of the argument checks
 * (all before any launch), the accepted capacities and page sizes, the split
 * plan (fa_decode_num_splits) and the workspace (fa_decode_ws_bytes) are those
 * of the 16-bit twin; one per-stream workspace serves all of them.
 * The bytes are converted to the 16-bit type in registers, exactly (every
 * finite E4M3 code is representable in fp16 and in bf16); k_scale enters the
 * score scale (and through it the LSE), v_scale the final normalisation, both
 * in fp32.  Rows past kv_lens[b], unmapped pages and out-of-pool page ids are
 * never read, as for the 16-bit entries.  The paged entry's O and LSE are
 * bit-identical to the contiguous kv8 entry's on the gathered cache with the
 * same num_splits.  fa_cache_append_kv8_* below write (quantise into) these
 * caches. */
int fa_decode_kv8_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                      int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                      int head_dim, const int* kv_lens, int causal, int num_splits,
                      void* workspace, unsigned long long ws_bytes, void* hip_stream,
                      const float* k_scale, const float* v_scale);
int fa_decode_kv8_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                       int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                       int head_dim, const int* kv_lens, int causal, int num_splits,
                       void* workspace, unsigned long long ws_bytes, void* hip_stream,
                       const float* k_scale, const float* v_scale);
int fa_decode_paged_kv8_f16(const void* q, const void* k_pages, const void* v_pages, void* o,
                            float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                            int head_dim, int num_pages, int page_size, const int* block_table,
                            int max_pages_per_seq, const int* kv_lens, int causal, int num_splits,
                            void* workspace, unsigned long long ws_bytes, void* hip_stream,
                            const float* k_scale, const float* v_scale);
int fa_decode_paged_kv8_bf16(const void* q, const void* k_pages, const void* v_pages, void* o,
                             float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                             int head_dim, int num_pages, int page_size, const int* block_table,
                             int max_pages_per_seq, const int* kv_lens, int causal, int num_splits,
                             void* workspace, unsigned long long ws_bytes, void* hip_stream,
                             const float* k_scale, const float* v_scale);

/* Cache append: write new K/V tokens into the caches the decode entries read,
 * K and V in one launch.
 *   k_new, v_new  [batch][heads_kv][seqlen_new][head_dim], fp16 or bf16,
 *             contiguous; seqlen_new >= 1, head_dim 128 or 64.
 *   k_cache, v_cache  [batch][heads_kv][kv_capacity][head_dim], or the pools
 *             k_pages, v_pages [num_pages][heads_kv][page_size][head_dim] with
 *             block_table as for fa_decode_paged_* (kv_capacity :=
 *             max_pages_per_seq * page_size).
 *   kv_lens   DEVICE int32[batch], REQUIRED: each element's length AFTER the
 *             append -- the tensor the following decode call takes.
 *   new_lens  DEVICE int32[batch], or NULL (= seqlen_new for every element).
 *     n_b = clamp(new_lens[b], 0, seqlen_new)
 *     for t in [0, n_b):  r = kv_lens[b] - n_b + t
 *       cache row r of (b, hkv) <- k_new[b][hkv][t][:]        (same for V)
 * Tokens t >= n_b are ignored (right-padded ragged prefill, elements with
 * nothing to append).  A row is written if and only if 0 <= r < kv_capacity;
 * kv_lens[b] is NOT clamped: a length past the capacity drops the rows that do
 * not exist, it does not shift them.  Paged: row r lives in page
 * block_table[b][r / page_size] at offset r % page_size and is written if and
 * only if that id is inside [0, num_pages) -- the write-side twin of "an
 * out-of-pool page id reads as zero rows".  Whether a row is written is decided
 * before any address is formed from it, and no byte of the caches other than
 * the rows named above is ever written.  Two batch elements whose tables map
 * the same page row are the caller's problem: one of them wins, unspecified
 * which.
 * _16: a 16-bit cache of k_new's type; a bit copy, so fp16 and bf16 share the
 * entry.  _kv8_f16 / _kv8_bf16 (the suffix is k_new's type): an FP8 E4M3
 * cache as fa_decode_kv8_* reads it.  The byte stored for a source element x
 * with s = k_scale[hkv] (v_scale[hkv] for V; NULL = 1.0) is
 *     y    = float(x) * (1.0f / s)       both in IEEE fp32, 1.0f / s correctly rounded
 *     byte = E4M3(clamp(y, -448, 448))   round to nearest even, subnormals
 *                                        down to 2^-9, -0.0 keeps its sign
 * +-inf saturates to +-448; a NaN stores a NaN code (0x7f or 0xff).  The
 * reciprocal-multiply form IS the contract (not x / s; the two agree exactly
 * for power-of-two scales).  Any finite scale in [2^-32, 2^32] is covered;
 * outside it, and for non-positive scales, the bytes are unspecified.
 * Lengths, table and scales are read on the device: no host read, no sync, no
 * workspace; everything is enqueued on hip_stream and is graph-capturable, and
 * table, lengths, scales and k_new / v_new contents may change between
 * replays.
 * Argument checks, all before any HIP call, in this order: a negative size:
 * FA_ERR_BAD_SHAPE; head_dim not 64 or 128: FA_ERR_UNSUPPORTED_HEAD_DIM;
 * seqlen_new < 1 (or > INT_MAX - 64), page_size / num_pages /
 * max_pages_per_seq / capacity outside what fa_decode_paged_* accepts:
 * FA_ERR_BAD_SHAPE; batch or heads_kv of 0: FA_OK, nothing enqueued;
 * kv_capacity * 2 * head_dim > INT_MAX (contiguous, as fa_decode_*):
 * FA_ERR_BAD_SHAPE; kv_capacity == 0: FA_OK, nothing enqueued; k_new, v_new, a
 * cache, kv_lens or block_table NULL: FA_ERR_NULL_POINTER. */
int fa_cache_append_16(const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                       int batch, int heads_kv, int seqlen_new, int kv_capacity, int head_dim,
                       const int* kv_lens, const int* new_lens, void* hip_stream);
int fa_cache_append_paged_16(const void* k_new, const void* v_new, void* k_pages, void* v_pages,
                             int batch, int heads_kv, int seqlen_new, int head_dim, int num_pages,
                             int page_size, const int* block_table, int max_pages_per_seq,
                             const int* kv_lens, const int* new_lens, void* hip_stream);
int fa_cache_append_kv8_f16(const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                            int batch, int heads_kv, int seqlen_new, int kv_capacity, int head_dim,
                            const int* kv_lens, const int* new_lens, void* hip_stream,
                            const float* k_scale, const float* v_scale);
int fa_cache_append_kv8_bf16(const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                             int batch, int heads_kv, int seqlen_new, int kv_capacity, int head_dim,
                             const int* kv_lens, const int* new_lens, void* hip_stream,
                             const float* k_scale, const float* v_scale);
int fa_cache_append_paged_kv8_f16(const void* k_new, const void* v_new, void* k_pages,
                                  void* v_pages, int batch, int heads_kv, int seqlen_new,
                                  int head_dim, int num_pages, int page_size,
                                  const int* block_table, int max_pages_per_seq,
                                  const int* kv_lens, const int* new_lens, void* hip_stream,
                                  const float* k_scale, const float* v_scale);
int fa_cache_append_paged_kv8_bf16(const void* k_new, const void* v_new, void* k_pages,
                                   void* v_pages, int batch, int heads_kv, int seqlen_new,
                                   int head_dim, int num_pages, int page_size,
                                   const int* block_table, int max_pages_per_seq,
                                   const int* kv_lens, const int* new_lens, void* hip_stream,
                                   const float* k_scale, const float* v_scale);

/* Prefill attention over the same K/V caches: any number of query tokens per
 * head (a whole prompt, or a chunk of one behind a cached prefix) against the
 * cache fa_cache_append_* wrote and fa_decode_* reads, in all four cache forms
 * (contiguous / paged, 16-bit / FP8 E4M3), with grouped K/V heads.  A prompt's
 * life, append -> prefill -> (append -> decode)*, runs over one cache with the
 * same kv_lens, block table and scales.
 *   q, o   [batch][heads_q][seqlen_q][head_dim]  16-bit, seqlen_q >= 1 (no
 *          upper bound but the 32-bit ranges below), head_dim 128 or 64
 *   k, v   the cache of fa_decode_* / fa_decode_kv8_*; k_pages, v_pages,
 *          block_table, num_pages, page_size, max_pages_per_seq: the pool of
 *          fa_decode_paged_* / fa_decode_paged_kv8_* (kv_capacity :=
 *          max_pages_per_seq * page_size)
 *   n_b   = q_lens ? clamp(q_lens[b], 0, seqlen_q) : seqlen_q
 *          the valid LEADING query tokens of element b: q_lens is the tensor
 *          fa_cache_append_* took as new_lens, with k_new's convention
 *   len_b = kv_lens ? clamp(kv_lens[b], 0, kv_capacity) : kv_capacity
 *          the keys of element b, the chunk's own included (the lengths AFTER
 *          the append)
 *   off_b = len_b - n_b   the keys that precede the chunk
 *   O[b,hq,t,:] = softmax(Q[b,hq,t,:] . K[b,hkv,0:vis,:]^T / sqrt(D))
 *                 . V[b,hkv,0:vis,:]                       for t < n_b
 *   hkv = hq / (heads_q / heads_kv)
 *   vis = causal ? clamp(off_b + t + 1, 0, len_b) : len_b
 * causal is bottom-right aligned, as for decode: with q_lens == NULL and
 * seqlen_q <= 16 the contract is fa_decode_*'s own.  A row that sees no key
 * (vis == 0, e.g. kv_lens[b] < n_b) gives O = 0 exactly and LSE = -inf.
 * Rows t >= n_b of o and lse are NOT WRITTEN (the read-side twin of append's
 * "nothing else is touched").  Cache rows at or past len_b, unmapped table
 * entries and pages past the length are never read (they may hold NaN); a
 * page id outside [0, num_pages) in an entry that is read reads as zero rows,
 * as for fa_decode_paged_*.
 *   lse    optional fp32 [batch][heads_q][seqlen_q], natural log; may be NULL.
 *   kv_lens, q_lens, block_table, k_scale, v_scale are DEVICE arrays read by
 *          the kernel: no host sync, no workspace, graph-capturable; a captured
 *          graph follows values rewritten between replays.  FP8: K is read as
 *          k_scale[hkv] * K8 and V as v_scale[hkv] * V8 (NULL = 1.0), the bytes
 *          converted exactly to the 16-bit type on their way into LDS.
 * A workgroup is (batch element, query head, 128-row query block); a block at
 * or past n_b returns at once.  The paged entries' O and LSE are bit-identical
 * to the contiguous entries' on the gathered cache.
 * Argument errors, all returned before any launch, in fa_decode_*'s order:
 * a negative count: FA_ERR_BAD_SHAPE; head_dim other than 64 / 128:
 * FA_ERR_UNSUPPORTED_HEAD_DIM; seqlen_q < 1, page_size not a positive multiple
 * of 64 (or page_size * 2 * head_dim > INT_MAX), num_pages <= 0,
 * max_pages_per_seq < 0, a logical capacity > INT_MAX - 64, heads_q %
 * heads_kv != 0, batch * heads_q * seqlen_q > INT_MAX, seqlen_q * 2 * head_dim
 * > INT_MAX, kv_capacity * 2 * head_dim > INT_MAX (contiguous; the FP8 entries
 * accept the same capacities) or more workgroups than a grid takes:
 * FA_ERR_BAD_SHAPE; q, k, v, o (or block_table) NULL with kv_capacity > 0:
 * FA_ERR_NULL_POINTER.  batch == 0 or heads_q == 0 return FA_OK with nothing
 * looked at (the page geometry is still checked); kv_capacity == 0 with rows
 * present fills O with zeros and LSE with -inf for ALL rows, as decode does.
 * fa_prefill_* are not tile configs: fa_config_info() does not list them. */
int fa_prefill_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                   int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                   int head_dim, const int* kv_lens, const int* q_lens, int causal,
                   void* hip_stream);
int fa_prefill_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                    int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                    int head_dim, const int* kv_lens, const int* q_lens, int causal,
                    void* hip_stream);
int fa_prefill_paged_f16(const void* q, const void* k_pages, const void* v_pages, void* o, float* lse,
                         int batch, int heads_q, int heads_kv, int seqlen_q, int head_dim,
                         int num_pages, int page_size, const int* block_table, int max_pages_per_seq,
                         const int* kv_lens, const int* q_lens, int causal, void* hip_stream);
int fa_prefill_paged_bf16(const void* q, const void* k_pages, const void* v_pages, void* o, float* lse,
                          int batch, int heads_q, int heads_kv, int seqlen_q, int head_dim,
                          int num_pages, int page_size, const int* block_table, int max_pages_per_seq,
                          const int* kv_lens, const int* q_lens, int causal, void* hip_stream);
int fa_prefill_kv8_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                       int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                       int head_dim, const int* kv_lens, const int* q_lens, int causal,
                       void* hip_stream, const float* k_scale, const float* v_scale);
int fa_prefill_kv8_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                        int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                        int head_dim, const int* kv_lens, const int* q_lens, int causal,
                        void* hip_stream, const float* k_scale, const float* v_scale);
int fa_prefill_paged_kv8_f16(const void* q, const void* k_pages, const void* v_pages, void* o,
                             float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                             int head_dim, int num_pages, int page_size, const int* block_table,
                             int max_pages_per_seq, const int* kv_lens, const int* q_lens, int causal,
                             void* hip_stream, const float* k_scale, const float* v_scale);
int fa_prefill_paged_kv8_bf16(const void* q, const void* k_pages, const void* v_pages, void* o,
                              float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                              int head_dim, int num_pages, int page_size, const int* block_table,
                              int max_pages_per_seq, const int* kv_lens, const int* q_lens, int causal,
                              void* hip_stream, const float* k_scale, const float* v_scale);

/* Packed variable-length (cu_seqlens) forms of the two entries that consume
 * new tokens, prefill and cache append, over the same four cache forms: what a
 * serving stack holds after its QKV projection, one token-major tensor for the
 * whole ragged batch and an int32 prefix sum, taken as it is (no padded copy).
 *   T      total_q / total_new: rows of the packed tensors
 *   batch  the number of sequences B
 *   cu     cu_seqlens_q / cu_seqlens: DEVICE int32[batch + 1], REQUIRED
 *     s_b = clamp(cu[b], 0, T)
 *     e_b = clamp(cu[b + 1], s_b, T)
 *     n_b = e_b - s_b            token t of sequence b is packed row s_b + t
 * The clamps make every cu memory-safe: whatever it holds (garbage, values
 * that decrease), nothing outside the T rows is addressed; for a cu that is
 * not monotone the result is unspecified.  kv_lens (the lengths AFTER the
 * append), len_b, off_b = len_b - n_b, vis, GQA, the bottom-right causal rule,
 * the cache forms, "rows past len_b are never read", "an out-of-pool page id
 * reads as zero rows / drops the row" and the FP8 contracts are those of
 * fa_prefill_* and fa_cache_append_* above, with n_b in q_lens' / new_lens'
 * place.  Everything is read on the device: no host look at cu, no sync, no
 * workspace, graph-capturable; a captured graph follows cu, kv_lens, tables
 * and scales rewritten between replays (T is a launch parameter).
 *
 * fa_prefill_varlen_*:
 *   q, o   [total_q][heads_q][head_dim]  16-bit, token-major, contiguous
 *   lse    optional fp32 [heads_q][total_q], natural log; may be NULL
 * Row s_b + t of o (and lse[hq][s_b + t]) is row t of element b of
 * fa_prefill_* called on the padded copy with q_lens = n, BIT FOR BIT: query
 * blocks are aligned to each sequence's own start, so a workgroup runs the
 * tile sequence the padded entry runs.  Rows below s_0, at or past e_{B-1},
 * and rows that belong to no sequence are NOT WRITTEN.  The launch is
 * heads_q * (total_q / 128 + batch) workgroups whatever the lengths are (a
 * workgroup finds its sequence by bisection on cu and returns if it has no
 * rows).  Causal blocks are not ordered heaviest first across sequences (that
 * needs the lengths on the host); within a sequence they start last to first.
 * Argument errors, all before any launch, in fa_prefill_*'s order: a negative
 * count (total_q included): FA_ERR_BAD_SHAPE; head_dim: as there; the page
 * geometry: as there; batch, heads_q or total_q of 0: FA_OK, nothing enqueued;
 * heads_q % heads_kv != 0, heads_q * total_q > INT_MAX (LSE rows), 128 *
 * heads_q * 2 * head_dim > INT_MAX (the byte range of one block's rows),
 * kv_capacity * 2 * head_dim > INT_MAX (contiguous), heads_q * (total_q / 128
 * + batch) > INT_MAX (the grid): FA_ERR_BAD_SHAPE; kv_capacity == 0 fills O
 * with zeros and LSE with -inf for ALL total_q rows; q, k, v, o, cu_seqlens_q
 * (or block_table) NULL: FA_ERR_NULL_POINTER.
 *
 * fa_cache_append_varlen_*:
 *   k_new, v_new  [total_new][heads_kv][head_dim]  16-bit, token-major
 *   token t of sequence b -> cache row kv_lens[b] - n_b + t, written if and
 *   only if the row exists (fa_cache_append_*'s rule; the FP8 byte is the
 *   reciprocal contract's, byte for byte).
 * Argument errors in fa_cache_append_*'s order, with total_new < 0 (or >
 * INT_MAX - 64) in seqlen_new's place, total_new == 0 returning FA_OK beside
 * batch == 0, total_new / TB + batch > INT_MAX (TB: 64 tokens at head_dim 128,
 * 128 at 64) FA_ERR_BAD_SHAPE before the capacity-0 return, and a NULL
 * cu_seqlens FA_ERR_NULL_POINTER with the other pointers. */
int fa_prefill_varlen_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                          int batch, int heads_q, int heads_kv, int total_q, int kv_capacity,
                          int head_dim, const int* kv_lens, const int* cu_seqlens_q, int causal,
                          void* hip_stream);
int fa_prefill_varlen_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                           int batch, int heads_q, int heads_kv, int total_q, int kv_capacity,
                           int head_dim, const int* kv_lens, const int* cu_seqlens_q, int causal,
                           void* hip_stream);
int fa_prefill_varlen_paged_f16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                float* lse, int batch, int heads_q, int heads_kv, int total_q,
                                int head_dim, int num_pages, int page_size, const int* block_table,
                                int max_pages_per_seq, const int* kv_lens, const int* cu_seqlens_q,
                                int causal, void* hip_stream);
int fa_prefill_varlen_paged_bf16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                 float* lse, int batch, int heads_q, int heads_kv, int total_q,
                                 int head_dim, int num_pages, int page_size, const int* block_table,
                                 int max_pages_per_seq, const int* kv_lens, const int* cu_seqlens_q,
                                 int causal, void* hip_stream);
int fa_prefill_varlen_kv8_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                              int batch, int heads_q, int heads_kv, int total_q, int kv_capacity,
                              int head_dim, const int* kv_lens, const int* cu_seqlens_q, int causal,
                              void* hip_stream, const float* k_scale, const float* v_scale);
int fa_prefill_varlen_kv8_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                               int batch, int heads_q, int heads_kv, int total_q, int kv_capacity,
                               int head_dim, const int* kv_lens, const int* cu_seqlens_q, int causal,
                               void* hip_stream, const float* k_scale, const float* v_scale);
int fa_prefill_varlen_paged_kv8_f16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                    float* lse, int batch, int heads_q, int heads_kv, int total_q,
                                    int head_dim, int num_pages, int page_size,
                                    const int* block_table, int max_pages_per_seq,
                                    const int* kv_lens, const int* cu_seqlens_q, int causal,
                                    void* hip_stream, const float* k_scale, const float* v_scale);
int fa_prefill_varlen_paged_kv8_bf16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                     float* lse, int batch, int heads_q, int heads_kv, int total_q,
                                     int head_dim, int num_pages, int page_size,
                                     const int* block_table, int max_pages_per_seq,
                                     const int* kv_lens, const int* cu_seqlens_q, int causal,
                                     void* hip_stream, const float* k_scale, const float* v_scale);
int fa_cache_append_varlen_16(const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                              int batch, int heads_kv, int total_new, int kv_capacity, int head_dim,
                              const int* kv_lens, const int* cu_seqlens, void* hip_stream);
int fa_cache_append_varlen_paged_16(const void* k_new, const void* v_new, void* k_pages,
                                    void* v_pages, int batch, int heads_kv, int total_new,
                                    int head_dim, int num_pages, int page_size,
                                    const int* block_table, int max_pages_per_seq,
                                    const int* kv_lens, const int* cu_seqlens, void* hip_stream);
int fa_cache_append_varlen_kv8_f16(const void* k_new, const void* v_new, void* k_cache,
                                   void* v_cache, int batch, int heads_kv, int total_new,
                                   int kv_capacity, int head_dim, const int* kv_lens,
                                   const int* cu_seqlens, void* hip_stream, const float* k_scale,
                                   const float* v_scale);
int fa_cache_append_varlen_kv8_bf16(const void* k_new, const void* v_new, void* k_cache,
                                    void* v_cache, int batch, int heads_kv, int total_new,
                                    int kv_capacity, int head_dim, const int* kv_lens,
                                    const int* cu_seqlens, void* hip_stream, const float* k_scale,
                                    const float* v_scale);
int fa_cache_append_varlen_paged_kv8_f16(const void* k_new, const void* v_new, void* k_pages,
                                         void* v_pages, int batch, int heads_kv, int total_new,
                                         int head_dim, int num_pages, int page_size,
                                         const int* block_table, int max_pages_per_seq,
                                         const int* kv_lens, const int* cu_seqlens,
                                         void* hip_stream, const float* k_scale,
                                         const float* v_scale);
int fa_cache_append_varlen_paged_kv8_bf16(const void* k_new, const void* v_new, void* k_pages,
                                          void* v_pages, int batch, int heads_kv, int total_new,
                                          int head_dim, int num_pages, int page_size,
                                          const int* block_table, int max_pages_per_seq,
                                          const int* kv_lens, const int* cu_seqlens,
                                          void* hip_stream, const float* k_scale,
                                          const float* v_scale);

/* Fused rotary position embedding + cache append: Q and K rotated, K and V
 * appended, one launch -- the step between the QKV projection and
 * fa_prefill_* / fa_decode_*.  Each entry takes what the fa_cache_append_* /
 * fa_cache_append_varlen_* entry of its cache form takes (with its meaning:
 * n_b, kv_lens AFTER the append, the cache forms, the FP8 scales), followed by
 *   q, q_out    [batch][heads_q][seqlen_new][head_dim], or packed
 *               [total_new][heads_q][head_dim]; of k_new's 16-bit type,
 *               contiguous.  q_out may be q (in place: a wave owns whole rows
 *               and loads them before it stores them).  heads_q = 0 with
 *               q = q_out = NULL rotates K only.  heads_q need not be a
 *               multiple of heads_kv.
 *   cos, sin    DEVICE float32 [rope_len][rotary_dim / 2], contiguous, 16-byte
 *               aligned
 *   rotary_dim  R, a multiple of 16 in [16, head_dim]
 *   interleaved 0: NeoX / Hugging Face rotate_half pairs; 1: GPT-J pairs
 * For token t < n_b of element b:
 *   pos = kv_lens[b] - n_b + t     the cache row the append writes; no
 *                                  positions tensor is taken
 *   pairs, i in [0, R/2):  interleaved = 0:  a = x[i],  b = x[i + R/2]
 *                          interleaved = 1:  a = x[2i], b = x[2i + 1]
 *   c = cos[pos][i], s = sin[pos][i]
 *   a' = a c - b s,  b' = b c + a s
 * Each product and each sum is an IEEE fp32 operation rounded on its own
 * (nothing is contracted into an fma) and the result is rounded once to the
 * 16-bit type, to nearest even; elements at or past R are bit copies.  This is
 * exactly what the torch expression (a.float() * c - b.float() * s).to(dtype)
 * gives on the CPU, so a caller's result does not change by a bit when they
 * switch over.  The equality is promised for finite inputs and tables whose
 * fp32 products are normal or zero; non-finite inputs give an unspecified
 * value, memory-safely.
 * K: the rotated 16-bit row is what the append's contract then stores: a
 * 16-bit cache takes it as it is, an FP8 cache applies E4M3(clamp(float(y) *
 * (1.0f / s), +-448)) to the ROUNDED 16-bit value y.  Fused equals "rotate,
 * then fa_cache_append_*" byte for byte in all four cache forms.  V is
 * appended unchanged.  A 16-bit cache is no longer a bit copy, so every form
 * has an _f16 and a _bf16 entry (the suffix is the type of k_new, v_new, q).
 * Q: row t of every query head is rotated with the same pos into q_out.
 * Which rows are written: a K/V row if and only if fa_cache_append_*'s rule
 * holds (row in [0, kv_capacity), paged id in the pool) AND pos < rope_len; a
 * q_out row if and only if t < n_b and 0 <= pos < rope_len (whatever the
 * capacity and the page ids are).  Nothing else is stored to, and no table row
 * outside [0, rope_len) is read.  kv_lens, new_lens / cu_seqlens, the block
 * table, the scales and the tables are read on the device: no host read, no
 * sync, no workspace, graph-capturable.
 * Argument errors, all before any launch, in fa_cache_append_*'s order with
 * the rotary ones among them: a negative size (heads_q included):
 * FA_ERR_BAD_SHAPE; head_dim; seqlen_new / total_new; then rotary_dim not a
 * multiple of 16 in [16, head_dim] or rope_len < 1: FA_ERR_BAD_SHAPE; the page
 * geometry; batch == 0, heads_kv == heads_q == 0 (or total_new == 0): FA_OK,
 * nothing enqueued; the capacity and grid ranges; a capacity of 0 leaves no
 * K/V row (FA_OK, nothing enqueued with heads_q == 0; otherwise Q alone is
 * rotated and the K/V pointers are not looked at); k_new, v_new, a cache,
 * block_table, kv_lens (cu_seqlens), then cos or sin, then q or q_out with
 * heads_q > 0 NULL: FA_ERR_NULL_POINTER; a table not 16-byte aligned:
 * FA_ERR_BAD_SHAPE. */
int fa_rope_append_f16(const void* k_new, const void* v_new, void* k_cache, void* v_cache, int batch,
                       int heads_kv, int seqlen_new, int kv_capacity, int head_dim,
                       const int* kv_lens, const int* new_lens, void* hip_stream, const void* q,
                       void* q_out, int heads_q, const float* cos, const float* sin, int rope_len,
                       int rotary_dim, int interleaved);
int fa_rope_append_bf16(const void* k_new, const void* v_new, void* k_cache, void* v_cache, int batch,
                        int heads_kv, int seqlen_new, int kv_capacity, int head_dim,
                        const int* kv_lens, const int* new_lens, void* hip_stream, const void* q,
                        void* q_out, int heads_q, const float* cos, const float* sin, int rope_len,
                        int rotary_dim, int interleaved);
int fa_rope_append_paged_f16(const void* k_new, const void* v_new, void* k_pages, void* v_pages,
                             int batch, int heads_kv, int seqlen_new, int head_dim, int num_pages,
                             int page_size, const int* block_table, int max_pages_per_seq,
                             const int* kv_lens, const int* new_lens, void* hip_stream,
                             const void* q, void* q_out, int heads_q, const float* cos,
                             const float* sin, int rope_len, int rotary_dim, int interleaved);
int fa_rope_append_paged_bf16(const void* k_new, const void* v_new, void* k_pages, void* v_pages,
                              int batch, int heads_kv, int seqlen_new, int head_dim, int num_pages,
                              int page_size, const int* block_table, int max_pages_per_seq,
                              const int* kv_lens, const int* new_lens, void* hip_stream,
                              const void* q, void* q_out, int heads_q, const float* cos,
                              const float* sin, int rope_len, int rotary_dim, int interleaved);
int fa_rope_append_kv8_f16(const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                           int batch, int heads_kv, int seqlen_new, int kv_capacity, int head_dim,
                           const int* kv_lens, const int* new_lens, void* hip_stream,
                           const float* k_scale, const float* v_scale, const void* q, void* q_out,
                           int heads_q, const float* cos, const float* sin, int rope_len,
                           int rotary_dim, int interleaved);
int fa_rope_append_kv8_bf16(const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                            int batch, int heads_kv, int seqlen_new, int kv_capacity, int head_dim,
                            const int* kv_lens, const int* new_lens, void* hip_stream,
                            const float* k_scale, const float* v_scale, const void* q, void* q_out,
                            int heads_q, const float* cos, const float* sin, int rope_len,
                            int rotary_dim, int interleaved);
int fa_rope_append_paged_kv8_f16(const void* k_new, const void* v_new, void* k_pages, void* v_pages,
                                 int batch, int heads_kv, int seqlen_new, int head_dim,
                                 int num_pages, int page_size, const int* block_table,
                                 int max_pages_per_seq, const int* kv_lens, const int* new_lens,
                                 void* hip_stream, const float* k_scale, const float* v_scale,
                                 const void* q, void* q_out, int heads_q, const float* cos,
                                 const float* sin, int rope_len, int rotary_dim, int interleaved);
int fa_rope_append_paged_kv8_bf16(const void* k_new, const void* v_new, void* k_pages, void* v_pages,
                                  int batch, int heads_kv, int seqlen_new, int head_dim,
                                  int num_pages, int page_size, const int* block_table,
                                  int max_pages_per_seq, const int* kv_lens, const int* new_lens,
                                  void* hip_stream, const float* k_scale, const float* v_scale,
                                  const void* q, void* q_out, int heads_q, const float* cos,
                                  const float* sin, int rope_len, int rotary_dim, int interleaved);
int fa_rope_append_varlen_f16(const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                              int batch, int heads_kv, int total_new, int kv_capacity, int head_dim,
                              const int* kv_lens, const int* cu_seqlens, void* hip_stream,
                              const void* q, void* q_out, int heads_q, const float* cos,
                              const float* sin, int rope_len, int rotary_dim, int interleaved);
int fa_rope_append_varlen_bf16(const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                               int batch, int heads_kv, int total_new, int kv_capacity, int head_dim,
                               const int* kv_lens, const int* cu_seqlens, void* hip_stream,
                               const void* q, void* q_out, int heads_q, const float* cos,
                               const float* sin, int rope_len, int rotary_dim, int interleaved);
int fa_rope_append_varlen_paged_f16(const void* k_new, const void* v_new, void* k_pages,
                                    void* v_pages, int batch, int heads_kv, int total_new,
                                    int head_dim, int num_pages, int page_size,
                                    const int* block_table, int max_pages_per_seq,
                                    const int* kv_lens, const int* cu_seqlens, void* hip_stream,
                                    const void* q, void* q_out, int heads_q, const float* cos,
                                    const float* sin, int rope_len, int rotary_dim, int interleaved);
int fa_rope_append_varlen_paged_bf16(const void* k_new, const void* v_new, void* k_pages,
                                     void* v_pages, int batch, int heads_kv, int total_new,
                                     int head_dim, int num_pages, int page_size,
                                     const int* block_table, int max_pages_per_seq,
                                     const int* kv_lens, const int* cu_seqlens, void* hip_stream,
                                     const void* q, void* q_out, int heads_q, const float* cos,
                                     const float* sin, int rope_len, int rotary_dim, int interleaved);
int fa_rope_append_varlen_kv8_f16(const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                                  int batch, int heads_kv, int total_new, int kv_capacity,
                                  int head_dim, const int* kv_lens, const int* cu_seqlens,
                                  void* hip_stream, const float* k_scale, const float* v_scale,
                                  const void* q, void* q_out, int heads_q, const float* cos,
                                  const float* sin, int rope_len, int rotary_dim, int interleaved);
int fa_rope_append_varlen_kv8_bf16(const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                                   int batch, int heads_kv, int total_new, int kv_capacity,
                                   int head_dim, const int* kv_lens, const int* cu_seqlens,
                                   void* hip_stream, const float* k_scale, const float* v_scale,
                                   const void* q, void* q_out, int heads_q, const float* cos,
                                   const float* sin, int rope_len, int rotary_dim, int interleaved);
int fa_rope_append_varlen_paged_kv8_f16(const void* k_new, const void* v_new, void* k_pages,
                                        void* v_pages, int batch, int heads_kv, int total_new,
                                        int head_dim, int num_pages, int page_size,
                                        const int* block_table, int max_pages_per_seq,
                                        const int* kv_lens, const int* cu_seqlens, void* hip_stream,
                                        const float* k_scale, const float* v_scale, const void* q,
                                        void* q_out, int heads_q, const float* cos, const float* sin,
                                        int rope_len, int rotary_dim, int interleaved);
int fa_rope_append_varlen_paged_kv8_bf16(const void* k_new, const void* v_new, void* k_pages,
                                         void* v_pages, int batch, int heads_kv, int total_new,
                                         int head_dim, int num_pages, int page_size,
                                         const int* block_table, int max_pages_per_seq,
                                         const int* kv_lens, const int* cu_seqlens, void* hip_stream,
                                         const float* k_scale, const float* v_scale, const void* q,
                                         void* q_out, int heads_q, const float* cos, const float* sin,
                                         int rope_len, int rotary_dim, int interleaved);

/* Sliding-window attention: the twelve fa_decode_*, fa_prefill_* and
 * fa_prefill_varlen_* entry pairs above with `int window` inserted directly
 * after `causal` (`_win` follows the family name).  window = W is the largest
 * number of keys a row may see, its own included:
 *   W = 0  no window: the entry computes what its twin without `_win` computes
 *   W < 0  FA_ERR_BAD_SHAPE (returned with the negative counts)
 *   W > 0 with causal == 0  FA_ERR_BAD_SHAPE (returned right after the seqlen_q
 *          / total_q check; there are no look-ahead windows)
 * With pos = off_b + t (prefill: off_b = len_b - n_b; decode: pos = len_b -
 * seqlen_q + t) row t sees the keys j with
 *   max(0, pos - W + 1) <= j <= min(pos, len_b - 1)
 * which is Hugging Face's sliding_window = W and flash-attn's window_size =
 * (W - 1, 0).  A row that sees no key gives zeros and LSE = -inf.  Everything
 * else is the twin's contract: lengths, tables and scales read on the device,
 * no sync, no workspace for prefill, graph-capturable, rows past q_lens not
 * written, every other argument error in the twin's place and order.  A W at or
 * past every len_b gives the twin's O and LSE bit for bit (decode: at the same
 * num_splits); the packed entries equal the padded ones and the paged ones the
 * contiguous ones on the gathered cache bit for bit, as without a window.
 * What is never read (callers may rely on it):
 *   - cache rows outside [lo, hi): lo = max(0, off_b + q0 - W + 1) for the
 *     128-row query block that starts at row q0 (decode: row 0's lower bound,
 *     max(0, len_b - seqlen_q - W + 1)), hi the twin's upper end;
 *   - paged: block-table entries of pages lying wholly below lo, so a server
 *     may free or reuse the pages every later query has slid past.
 * Decode splits the tiles [lo / 64, ceil(len_b / 64)) into its pieces, not the
 * whole cache.  With num_splits = 0 a call with W > 0 plans from the capacity
 * a window can touch,
 *   cap_w = min(kv_capacity, 64 * ceil((W + seqlen_q - 1) / 64) + 64)
 * so its pieces and its workspace are fa_decode_num_splits() and
 * fa_decode_ws_bytes() called with cap_w in kv_capacity's place (a forced
 * num_splits needs fa_decode_ws_bytes() of that count, as for the twin). */
int fa_decode_win_f16(const void* q, const void* k, const void* v, void* o, float* lse, int batch,
                      int heads_q, int heads_kv, int seqlen_q, int kv_capacity, int head_dim,
                      const int* kv_lens, int causal, int window, int num_splits, void* workspace,
                      unsigned long long ws_bytes, void* hip_stream);
int fa_decode_win_bf16(const void* q, const void* k, const void* v, void* o, float* lse, int batch,
                       int heads_q, int heads_kv, int seqlen_q, int kv_capacity, int head_dim,
                       const int* kv_lens, int causal, int window, int num_splits, void* workspace,
                       unsigned long long ws_bytes, void* hip_stream);
int fa_decode_win_paged_f16(const void* q, const void* k_pages, const void* v_pages, void* o,
                            float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                            int head_dim, int num_pages, int page_size, const int* block_table,
                            int max_pages_per_seq, const int* kv_lens, int causal, int window,
                            int num_splits, void* workspace, unsigned long long ws_bytes,
                            void* hip_stream);
int fa_decode_win_paged_bf16(const void* q, const void* k_pages, const void* v_pages, void* o,
                             float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                             int head_dim, int num_pages, int page_size, const int* block_table,
                             int max_pages_per_seq, const int* kv_lens, int causal, int window,
                             int num_splits, void* workspace, unsigned long long ws_bytes,
                             void* hip_stream);
int fa_decode_win_kv8_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                          int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                          int head_dim, const int* kv_lens, int causal, int window, int num_splits,
                          void* workspace, unsigned long long ws_bytes, void* hip_stream,
                          const float* k_scale, const float* v_scale);
int fa_decode_win_kv8_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                           int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                           int head_dim, const int* kv_lens, int causal, int window, int num_splits,
                           void* workspace, unsigned long long ws_bytes, void* hip_stream,
                           const float* k_scale, const float* v_scale);
int fa_decode_win_paged_kv8_f16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                                int head_dim, int num_pages, int page_size, const int* block_table,
                                int max_pages_per_seq, const int* kv_lens, int causal, int window,
                                int num_splits, void* workspace, unsigned long long ws_bytes,
                                void* hip_stream, const float* k_scale, const float* v_scale);
int fa_decode_win_paged_kv8_bf16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                 float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                                 int head_dim, int num_pages, int page_size, const int* block_table,
                                 int max_pages_per_seq, const int* kv_lens, int causal, int window,
                                 int num_splits, void* workspace, unsigned long long ws_bytes,
                                 void* hip_stream, const float* k_scale, const float* v_scale);
int fa_prefill_win_f16(const void* q, const void* k, const void* v, void* o, float* lse, int batch,
                       int heads_q, int heads_kv, int seqlen_q, int kv_capacity, int head_dim,
                       const int* kv_lens, const int* q_lens, int causal, int window,
                       void* hip_stream);
int fa_prefill_win_bf16(const void* q, const void* k, const void* v, void* o, float* lse, int batch,
                        int heads_q, int heads_kv, int seqlen_q, int kv_capacity, int head_dim,
                        const int* kv_lens, const int* q_lens, int causal, int window,
                        void* hip_stream);
int fa_prefill_win_paged_f16(const void* q, const void* k_pages, const void* v_pages, void* o,
                             float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                             int head_dim, int num_pages, int page_size, const int* block_table,
                             int max_pages_per_seq, const int* kv_lens, const int* q_lens,
                             int causal, int window, void* hip_stream);
int fa_prefill_win_paged_bf16(const void* q, const void* k_pages, const void* v_pages, void* o,
                              float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                              int head_dim, int num_pages, int page_size, const int* block_table,
                              int max_pages_per_seq, const int* kv_lens, const int* q_lens,
                              int causal, int window, void* hip_stream);
int fa_prefill_win_kv8_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                           int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                           int head_dim, const int* kv_lens, const int* q_lens, int causal,
                           int window, void* hip_stream, const float* k_scale, const float* v_scale);
int fa_prefill_win_kv8_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                            int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                            int head_dim, const int* kv_lens, const int* q_lens, int causal,
                            int window, void* hip_stream, const float* k_scale, const float* v_scale);
int fa_prefill_win_paged_kv8_f16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                 float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                                 int head_dim, int num_pages, int page_size, const int* block_table,
                                 int max_pages_per_seq, const int* kv_lens, const int* q_lens,
                                 int causal, int window, void* hip_stream, const float* k_scale,
                                 const float* v_scale);
int fa_prefill_win_paged_kv8_bf16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                  float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                                  int head_dim, int num_pages, int page_size,
                                  const int* block_table, int max_pages_per_seq, const int* kv_lens,
                                  const int* q_lens, int causal, int window, void* hip_stream,
                                  const float* k_scale, const float* v_scale);
int fa_prefill_varlen_win_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                              int batch, int heads_q, int heads_kv, int total_q, int kv_capacity,
                              int head_dim, const int* kv_lens, const int* cu_seqlens_q, int causal,
                              int window, void* hip_stream);
int fa_prefill_varlen_win_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                               int batch, int heads_q, int heads_kv, int total_q, int kv_capacity,
                               int head_dim, const int* kv_lens, const int* cu_seqlens_q,
                               int causal, int window, void* hip_stream);
int fa_prefill_varlen_win_paged_f16(const void* q, const void* k_pages, const void* v_pages,
                                    void* o, float* lse, int batch, int heads_q, int heads_kv,
                                    int total_q, int head_dim, int num_pages, int page_size,
                                    const int* block_table, int max_pages_per_seq,
                                    const int* kv_lens, const int* cu_seqlens_q, int causal,
                                    int window, void* hip_stream);
int fa_prefill_varlen_win_paged_bf16(const void* q, const void* k_pages, const void* v_pages,
                                     void* o, float* lse, int batch, int heads_q, int heads_kv,
                                     int total_q, int head_dim, int num_pages, int page_size,
                                     const int* block_table, int max_pages_per_seq,
                                     const int* kv_lens, const int* cu_seqlens_q, int causal,
                                     int window, void* hip_stream);
int fa_prefill_varlen_win_kv8_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                                  int batch, int heads_q, int heads_kv, int total_q,
                                  int kv_capacity, int head_dim, const int* kv_lens,
                                  const int* cu_seqlens_q, int causal, int window, void* hip_stream,
                                  const float* k_scale, const float* v_scale);
int fa_prefill_varlen_win_kv8_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                                   int batch, int heads_q, int heads_kv, int total_q,
                                   int kv_capacity, int head_dim, const int* kv_lens,
                                   const int* cu_seqlens_q, int causal, int window,
                                   void* hip_stream, const float* k_scale, const float* v_scale);
int fa_prefill_varlen_win_paged_kv8_f16(const void* q, const void* k_pages, const void* v_pages,
                                        void* o, float* lse, int batch, int heads_q, int heads_kv,
                                        int total_q, int head_dim, int num_pages, int page_size,
                                        const int* block_table, int max_pages_per_seq,
                                        const int* kv_lens, const int* cu_seqlens_q, int causal,
                                        int window, void* hip_stream, const float* k_scale,
                                        const float* v_scale);
int fa_prefill_varlen_win_paged_kv8_bf16(const void* q, const void* k_pages, const void* v_pages,
                                         void* o, float* lse, int batch, int heads_q, int heads_kv,
                                         int total_q, int head_dim, int num_pages, int page_size,
                                         const int* block_table, int max_pages_per_seq,
                                         const int* kv_lens, const int* cu_seqlens_q, int causal,
                                         int window, void* hip_stream, const float* k_scale,
                                         const float* v_scale);

/* Attention sinks: the twenty-four `_win` entries above with
 * `const float* sinks` inserted directly after `window` (`_sink` in `_win`'s
 * place).  sinks is a device array of heads_q floats, read on the device (a
 * captured graph follows its values), or NULL for no sinks: one learned logit
 * per query head that joins the softmax denominator and contributes no value.
 * With s_j the scaled scores (natural-log units, after 1/sqrt(head_dim) and
 * k_scale) of the keys a row of head h sees -- exactly the `_win` twin's keys:
 * causal, kv_lens, q_lens and window unchanged --
 *   den = exp(sinks[h]) + sum_j exp(s_j)
 *   O   = sum_j exp(s_j) v_j / den          (times v_scale for an FP8 cache)
 *   LSE = log(den)                          (the sink is included)
 * The sink is not multiplied by 1/sqrt(head_dim) or by k_scale.  A row that
 * sees no key gives O = 0 and LSE = sinks[h] on every path, kv_capacity == 0
 * included.  sinks[h] = -inf is "no sink for that head"; NaN is unspecified.
 * With sinks == NULL, or every sink -inf, O and LSE are the `_win` twin's bit
 * for bit.  window keeps the twin's meaning and statuses (0: no window; the
 * kernels then run as W = capacity, causal or not), and every other argument
 * error arrives in the twin's place and order; there are no new status codes,
 * no sync, and no workspace beyond the twin's: decode's pieces, workspace,
 * fa_decode_num_splits() and fa_decode_ws_bytes() are unchanged, and the sink
 * enters once, in the final normalisation.  Rows past q_lens are not written.
 * LSE includes the sink, so a caller that merges partial states by their LSE
 * (chunks of one cache attended separately) must pass sinks to ONE partial
 * only: each partial given the sink would count it again. */
int fa_decode_sink_f16(const void* q, const void* k, const void* v, void* o, float* lse, int batch,
                       int heads_q, int heads_kv, int seqlen_q, int kv_capacity, int head_dim,
                       const int* kv_lens, int causal, int window, const float* sinks,
                       int num_splits, void* workspace, unsigned long long ws_bytes,
                       void* hip_stream);
int fa_decode_sink_bf16(const void* q, const void* k, const void* v, void* o, float* lse, int batch,
                        int heads_q, int heads_kv, int seqlen_q, int kv_capacity, int head_dim,
                        const int* kv_lens, int causal, int window, const float* sinks,
                        int num_splits, void* workspace, unsigned long long ws_bytes,
                        void* hip_stream);
int fa_decode_sink_paged_f16(const void* q, const void* k_pages, const void* v_pages, void* o,
                             float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                             int head_dim, int num_pages, int page_size, const int* block_table,
                             int max_pages_per_seq, const int* kv_lens, int causal, int window,
                             const float* sinks, int num_splits, void* workspace,
                             unsigned long long ws_bytes, void* hip_stream);
int fa_decode_sink_paged_bf16(const void* q, const void* k_pages, const void* v_pages, void* o,
                              float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                              int head_dim, int num_pages, int page_size, const int* block_table,
                              int max_pages_per_seq, const int* kv_lens, int causal, int window,
                              const float* sinks, int num_splits, void* workspace,
                              unsigned long long ws_bytes, void* hip_stream);
int fa_decode_sink_kv8_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                           int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                           int head_dim, const int* kv_lens, int causal, int window,
                           const float* sinks, int num_splits, void* workspace,
                           unsigned long long ws_bytes, void* hip_stream, const float* k_scale,
                           const float* v_scale);
int fa_decode_sink_kv8_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                            int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                            int head_dim, const int* kv_lens, int causal, int window,
                            const float* sinks, int num_splits, void* workspace,
                            unsigned long long ws_bytes, void* hip_stream, const float* k_scale,
                            const float* v_scale);
int fa_decode_sink_paged_kv8_f16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                 float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                                 int head_dim, int num_pages, int page_size, const int* block_table,
                                 int max_pages_per_seq, const int* kv_lens, int causal, int window,
                                 const float* sinks, int num_splits, void* workspace,
                                 unsigned long long ws_bytes, void* hip_stream,
                                 const float* k_scale, const float* v_scale);
int fa_decode_sink_paged_kv8_bf16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                  float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                                  int head_dim, int num_pages, int page_size,
                                  const int* block_table, int max_pages_per_seq, const int* kv_lens,
                                  int causal, int window, const float* sinks, int num_splits,
                                  void* workspace, unsigned long long ws_bytes, void* hip_stream,
                                  const float* k_scale, const float* v_scale);
int fa_prefill_sink_f16(const void* q, const void* k, const void* v, void* o, float* lse, int batch,
                        int heads_q, int heads_kv, int seqlen_q, int kv_capacity, int head_dim,
                        const int* kv_lens, const int* q_lens, int causal, int window,
                        const float* sinks, void* hip_stream);
int fa_prefill_sink_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                         int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                         int head_dim, const int* kv_lens, const int* q_lens, int causal,
                         int window, const float* sinks, void* hip_stream);
int fa_prefill_sink_paged_f16(const void* q, const void* k_pages, const void* v_pages, void* o,
                              float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                              int head_dim, int num_pages, int page_size, const int* block_table,
                              int max_pages_per_seq, const int* kv_lens, const int* q_lens,
                              int causal, int window, const float* sinks, void* hip_stream);
int fa_prefill_sink_paged_bf16(const void* q, const void* k_pages, const void* v_pages, void* o,
                               float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                               int head_dim, int num_pages, int page_size, const int* block_table,
                               int max_pages_per_seq, const int* kv_lens, const int* q_lens,
                               int causal, int window, const float* sinks, void* hip_stream);
int fa_prefill_sink_kv8_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                            int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                            int head_dim, const int* kv_lens, const int* q_lens, int causal,
                            int window, const float* sinks, void* hip_stream, const float* k_scale,
                            const float* v_scale);
int fa_prefill_sink_kv8_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                             int batch, int heads_q, int heads_kv, int seqlen_q, int kv_capacity,
                             int head_dim, const int* kv_lens, const int* q_lens, int causal,
                             int window, const float* sinks, void* hip_stream, const float* k_scale,
                             const float* v_scale);
int fa_prefill_sink_paged_kv8_f16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                  float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                                  int head_dim, int num_pages, int page_size,
                                  const int* block_table, int max_pages_per_seq, const int* kv_lens,
                                  const int* q_lens, int causal, int window, const float* sinks,
                                  void* hip_stream, const float* k_scale, const float* v_scale);
int fa_prefill_sink_paged_kv8_bf16(const void* q, const void* k_pages, const void* v_pages, void* o,
                                   float* lse, int batch, int heads_q, int heads_kv, int seqlen_q,
                                   int head_dim, int num_pages, int page_size,
                                   const int* block_table, int max_pages_per_seq,
                                   const int* kv_lens, const int* q_lens, int causal, int window,
                                   const float* sinks, void* hip_stream, const float* k_scale,
                                   const float* v_scale);
int fa_prefill_varlen_sink_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                               int batch, int heads_q, int heads_kv, int total_q, int kv_capacity,
                               int head_dim, const int* kv_lens, const int* cu_seqlens_q,
                               int causal, int window, const float* sinks, void* hip_stream);
int fa_prefill_varlen_sink_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                                int batch, int heads_q, int heads_kv, int total_q, int kv_capacity,
                                int head_dim, const int* kv_lens, const int* cu_seqlens_q,
                                int causal, int window, const float* sinks, void* hip_stream);
int fa_prefill_varlen_sink_paged_f16(const void* q, const void* k_pages, const void* v_pages,
                                     void* o, float* lse, int batch, int heads_q, int heads_kv,
                                     int total_q, int head_dim, int num_pages, int page_size,
                                     const int* block_table, int max_pages_per_seq,
                                     const int* kv_lens, const int* cu_seqlens_q, int causal,
                                     int window, const float* sinks, void* hip_stream);
int fa_prefill_varlen_sink_paged_bf16(const void* q, const void* k_pages, const void* v_pages,
                                      void* o, float* lse, int batch, int heads_q, int heads_kv,
                                      int total_q, int head_dim, int num_pages, int page_size,
                                      const int* block_table, int max_pages_per_seq,
                                      const int* kv_lens, const int* cu_seqlens_q, int causal,
                                      int window, const float* sinks, void* hip_stream);
int fa_prefill_varlen_sink_kv8_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                                   int batch, int heads_q, int heads_kv, int total_q,
                                   int kv_capacity, int head_dim, const int* kv_lens,
                                   const int* cu_seqlens_q, int causal, int window,
                                   const float* sinks, void* hip_stream, const float* k_scale,
                                   const float* v_scale);
int fa_prefill_varlen_sink_kv8_bf16(const void* q, const void* k, const void* v, void* o,
                                    float* lse, int batch, int heads_q, int heads_kv, int total_q,
                                    int kv_capacity, int head_dim, const int* kv_lens,
                                    const int* cu_seqlens_q, int causal, int window,
                                    const float* sinks, void* hip_stream, const float* k_scale,
                                    const float* v_scale);
int fa_prefill_varlen_sink_paged_kv8_f16(const void* q, const void* k_pages, const void* v_pages,
                                         void* o, float* lse, int batch, int heads_q, int heads_kv,
                                         int total_q, int head_dim, int num_pages, int page_size,
                                         const int* block_table, int max_pages_per_seq,
                                         const int* kv_lens, const int* cu_seqlens_q, int causal,
                                         int window, const float* sinks, void* hip_stream,
                                         const float* k_scale, const float* v_scale);
int fa_prefill_varlen_sink_paged_kv8_bf16(const void* q, const void* k_pages, const void* v_pages,
                                          void* o, float* lse, int batch, int heads_q, int heads_kv,
                                          int total_q, int head_dim, int num_pages, int page_size,
                                          const int* block_table, int max_pages_per_seq,
                                          const int* kv_lens, const int* cu_seqlens_q, int causal,
                                          int window, const float* sinks, void* hip_stream,
                                          const float* k_scale, const float* v_scale);

/* Attention over token-major Q, K and V with NO cache (flash-attn's
 * flash_attn_varlen_func / flash_attn_func): what a QKV projection leaves,
 * taken as it is -- an encoder, a vision tower, an embedding model, a first
 * prefill whose keys are not cached yet.  The prefill kernels over a fifth K/V
 * source.
 *
 *   q      [total_q][heads_q][head_dim]   16-bit, token-major
 *   k, v   [total_k][heads_kv][head_dim]  the same type, heads_q % heads_kv == 0
 *   o      [total_q][heads_q][head_dim]   dense
 *   lse    optional fp32 [heads_q][total_q], natural log; may be NULL
 *   q_stride, k_stride, v_stride: ELEMENTS between consecutive tokens of q, k
 *     and v; 0 = dense (heads * head_dim).  Heads are head_dim apart and the
 *     last dimension is contiguous, so the three may be the slices of one
 *     fused QKV buffer, read in place.  A stride must be a multiple of 8 (16-
 *     byte loads), not shorter than heads * head_dim, and the byte range of one
 *     block's rows (127 * stride * 2 + 2 head_dim for q, 63 * stride * 2 + 2
 *     head_dim for k and v) must fit a 32-bit int.  o and q must not overlap.
 *   cu_seqlens_q, cu_seqlens_k: device int32 [batch + 1], read and clamped on
 *     the device by the rule of the fa_prefill_varlen_* entries:
 *       (sq_b, nq_b) = the span of cu_seqlens_q clamped to [0, total_q]
 *       (sk_b, nk_b) = the span of cu_seqlens_k clamped to [0, total_k]
 *     cu_seqlens_k == NULL: self-attention, the keys' spans are the spans of
 *     cu_seqlens_q (clamped to [0, total_k]).  Both NULL: uniform lengths,
 *     sq_b = b * seqlen_q and sk_b = b * seqlen_k with total_q = batch *
 *     seqlen_q and total_k = batch * seqlen_k -- the [B][S][H][D] layout; no
 *     array is read.  seqlen_q and seqlen_k are looked at in that mode only.
 *
 * Row t of sequence b (o row sq_b + t) sees keys [lo, vis) of b, with off_b =
 * nk_b - nq_b: vis = causal ? clamp(off_b + t + 1, 0, nk_b) : nk_b (bottom-
 * right aligned), lo = 0 -- fa_prefill_varlen_*'s formulas with len_b = nk_b,
 * and its bits: o and lse equal fa_prefill_varlen_* on a contiguous cache
 * whose rows [0, nk_b) of element b are the same keys, bit for bit.  A row
 * that sees no key gives zeros and lse = -inf.  Rows of o and lse that belong
 * to no sequence are not written; rows of k and v that belong to no sequence,
 * or lie past a row block's range, are never read.  Any contents of the two
 * arrays are memory-safe (if they do not increase the result is unspecified).
 * No sync, no workspace, graph-capturable; a captured graph follows the arrays.
 * Tensors may exceed 4 GiB; total_k <= INT_MAX - 64.
 *
 * Statuses, all before any launch and in this order: negative batch, heads,
 * total_k, head_dim (or window) FA_ERR_BAD_SHAPE; head_dim not 64 / 128
 * FA_ERR_UNSUPPORTED_HEAD_DIM; negative total_q, window > 0 without causal, a
 * stride that is negative, no multiple of 8 or past the byte range,
 * cu_seqlens_k without cu_seqlens_q, uniform mode with a negative seqlen or
 * total != batch * seqlen FA_ERR_BAD_SHAPE; batch, heads_q or total_q == 0
 * FA_OK; heads_q % heads_kv != 0, a stride shorter than its heads * head_dim,
 * heads_q * total_q > INT_MAX, total_k > INT_MAX - 64 FA_ERR_BAD_SHAPE;
 * total_k == 0: o = 0 and lse = -inf (or the sink) for ALL total_q rows (o
 * NULL: FA_ERR_NULL_POINTER); NULL q, k, v or o FA_ERR_NULL_POINTER.
 *
 * _win: `int window` after `causal`, the sliding window of the _win entries
 * above (W = 0: none, the plain entry's bits; W > 0 needs causal): lo =
 * max(0, off_b + t - W + 1).  _sink: `const float* sinks` last, the attention
 * sinks of the _sink entries above (float32 [heads_q]; NULL or -inf: the _win
 * entry's bits; a row with no key gives lse = sinks[h]). */
int fa_attn_varlen_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                       int batch, int heads_q, int heads_kv, int total_q, int total_k, int head_dim,
                       long long q_stride, long long k_stride, long long v_stride,
                       const int* cu_seqlens_q, const int* cu_seqlens_k, int seqlen_q, int seqlen_k,
                       int causal, void* hip_stream);
int fa_attn_varlen_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                        int batch, int heads_q, int heads_kv, int total_q, int total_k, int head_dim,
                        long long q_stride, long long k_stride, long long v_stride,
                        const int* cu_seqlens_q, const int* cu_seqlens_k, int seqlen_q, int seqlen_k,
                        int causal, void* hip_stream);
int fa_attn_varlen_win_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                           int batch, int heads_q, int heads_kv, int total_q, int total_k,
                           int head_dim, long long q_stride, long long k_stride, long long v_stride,
                           const int* cu_seqlens_q, const int* cu_seqlens_k, int seqlen_q,
                           int seqlen_k, int causal, int window, void* hip_stream);
int fa_attn_varlen_win_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                            int batch, int heads_q, int heads_kv, int total_q, int total_k,
                            int head_dim, long long q_stride, long long k_stride, long long v_stride,
                            const int* cu_seqlens_q, const int* cu_seqlens_k, int seqlen_q,
                            int seqlen_k, int causal, int window, void* hip_stream);
int fa_attn_varlen_sink_f16(const void* q, const void* k, const void* v, void* o, float* lse,
                            int batch, int heads_q, int heads_kv, int total_q, int total_k,
                            int head_dim, long long q_stride, long long k_stride, long long v_stride,
                            const int* cu_seqlens_q, const int* cu_seqlens_k, int seqlen_q,
                            int seqlen_k, int causal, int window, void* hip_stream,
                            const float* sinks);
int fa_attn_varlen_sink_bf16(const void* q, const void* k, const void* v, void* o, float* lse,
                             int batch, int heads_q, int heads_kv, int total_q, int total_k,
                             int head_dim, long long q_stride, long long k_stride, long long v_stride,
                             const int* cu_seqlens_q, const int* cu_seqlens_k, int seqlen_q,
                             int seqlen_k, int causal, int window, void* hip_stream,
                             const float* sinks);

/* Backward pass of fa_attn_varlen_f16 / _bf16: dq, dk and dv from dout, the
 * forward's inputs and its out and lse (csrc/fa_attn_bwd_kernel.hpp, DESIGN.md
 * §3.0q).  With c = 1 / sqrt(head_dim), s_ij = c q_i . k_j, P_ij = exp(s_ij -
 * lse_i) on the keys row i sees by the forward's rule (0 elsewhere) and
 * delta_i = sum_d dout_id out_id:
 *   dv_j = sum_i P_ij dout_i           dS_ij = P_ij (dout_i . v_j - delta_i)
 *   dq_i = c sum_j dS_ij k_j           dk_j = c sum_i dS_ij q_i
 * dk and dv of a K/V head sum over its heads_q / heads_kv query heads.  All
 * sums are fp32; P and dS are rounded to the 16-bit type once, as matrix
 * operands, and every output element once.
 *
 *   dout: [total_q][heads_q][head_dim], under the stride rule of q (do_stride)
 *   q, k, v, the strides, cu_seqlens_q / cu_seqlens_k, seqlen_q / seqlen_k,
 *     causal: as the forward took them (the byte range of a block's rows is
 *     127 * stride * 2 + 2 head_dim for all four strided tensors here)
 *   out: the forward's o, dense;  lse: the forward's lse, fp32 [heads_q][total_q]
 *   dq: [total_q][heads_q][head_dim], dk, dv: [total_k][heads_kv][head_dim],
 *     dense, of the inputs' type
 *   delta: fp32 [heads_q][total_q], the only workspace (written, then read)
 *
 * A row that sees no key (lse = -inf) gets dq = 0 and adds nothing to dk and
 * dv; a key of a sequence that no row sees gets dk = dv = 0, written.  Rows of
 * dq, dk, dv that belong to no sequence are not written, and such rows of
 * dout, q, k, v, out, lse are never read.  Any contents of the cu arrays are
 * memory-safe.  Three launches on the stream (delta, dK/dV, dQ), no sync,
 * nothing read back, graph-capturable, no atomics: two calls on the same
 * inputs give the same bits.
 *
 * Statuses in the forward's order: negative counts, head_dim, the strides
 * (do_stride with them), the modes as there; heads_q == 0 FA_OK; batch == 0 or
 * total_q == 0: dk = dv = 0 for all total_k rows (NULL dk or dv with rows to
 * fill: FA_ERR_NULL_POINTER), FA_OK; then heads_q % heads_kv, a short stride,
 * heads_q * total_q > INT_MAX, total_k > INT_MAX - 64 FA_ERR_BAD_SHAPE;
 * total_k == 0: dq = 0 for ALL total_q rows (NULL dq: FA_ERR_NULL_POINTER),
 * FA_OK; any pointer but the cu arrays NULL (lse and delta included):
 * FA_ERR_NULL_POINTER. */
int fa_attn_varlen_bwd_f16(const void* dout, const void* q, const void* k, const void* v,
                           const void* out, const float* lse, void* dq, void* dk, void* dv, float* delta,
                           int batch, int heads_q, int heads_kv, int total_q, int total_k, int head_dim,
                           long long do_stride, long long q_stride, long long k_stride, long long v_stride,
                           const int* cu_seqlens_q, const int* cu_seqlens_k, int seqlen_q, int seqlen_k,
                           int causal, void* hip_stream);
int fa_attn_varlen_bwd_bf16(const void* dout, const void* q, const void* k, const void* v,
                            const void* out, const float* lse, void* dq, void* dk, void* dv, float* delta,
                            int batch, int heads_q, int heads_kv, int total_q, int total_k, int head_dim,
                            long long do_stride, long long q_stride, long long k_stride, long long v_stride,
                            const int* cu_seqlens_q, const int* cu_seqlens_k, int seqlen_q, int seqlen_k,
                            int causal, void* hip_stream);

/* Backward pass of fa_attn_varlen_win_* and fa_attn_varlen_sink_* (DESIGN.md
 * §3.0r): fa_attn_varlen_bwd_*'s arguments with `int window` after `causal`,
 * and for the sink entries `sinks` and `dsinks` after the stream.
 *
 *   window: the forward's.  0: none; W >= 1: row t of sequence b sees the keys
 *     [max(0, nk_b - nq_b + t - W + 1), nk_b - nq_b + t], causal only.  P is 0
 *     on every other key, the formulas above are unchanged, and the kernels walk
 *     the band: a key block's sweep over the query tiles ends with the last row
 *     whose window reaches it, a query block's sweep over the key tiles starts
 *     at its first row's first key, and K/V tiles wholly below a block's window
 *     are never loaded.  A key no row sees (nk_b > nq_b + W - 1) gets dk = dv =
 *     0, written.
 *   sinks: float32 [heads_q], the forward's (lse holds them; NULL: none).  The
 *     sink is one more softmax column with a zero value, so dq, dk and dv are
 *     the formulas above on that lse, and
 *   dsinks: float32 [heads_q], written (never accumulated into):
 *       dsinks[h] = - sum_i exp(sinks[h] - lse[h][i]) delta[h][i]
 *     over the rows of head h that belong to a sequence, in fp32 and in one
 *     fixed order (a fourth launch of heads_q workgroups, no atomics).  A row
 *     whose lse is -inf adds nothing; sinks[h] = -inf gives dsinks[h] = 0.
 *     Required with sinks.  sinks == NULL: dsinks may be NULL and is zero-filled
 *     if it is given.
 *
 * Bit for bit: _win with window 0, or causal with a window no shorter than
 * every sequence's keys, is fa_attn_varlen_bwd_*; _sink with sinks == NULL is
 * _win; _sink with every sink -inf gives _win's dq, dk, dv and dsinks = 0.
 *
 * Statuses: fa_attn_varlen_bwd_*'s, in the forward's order with window < 0
 * after the negative counts and window > 0 without causal after total_q
 * (FA_ERR_BAD_SHAPE); the empty problems (batch == 0, total_q == 0, total_k ==
 * 0) also zero-fill dsinks where it is given; total_q + total_k > INT_MAX
 * FA_ERR_BAD_SHAPE with the other 32-bit ranges; sinks without dsinks
 * FA_ERR_NULL_POINTER, last. */
int fa_attn_bwd_win_f16(const void* dout, const void* q, const void* k, const void* v, const void* out,
                        const float* lse, void* dq, void* dk, void* dv, float* delta, int batch,
                        int heads_q, int heads_kv, int total_q, int total_k, int head_dim,
                        long long do_stride, long long q_stride, long long k_stride, long long v_stride,
                        const int* cu_seqlens_q, const int* cu_seqlens_k, int seqlen_q, int seqlen_k,
                        int causal, int window, void* hip_stream);
int fa_attn_bwd_win_bf16(const void* dout, const void* q, const void* k, const void* v, const void* out,
                         const float* lse, void* dq, void* dk, void* dv, float* delta, int batch,
                         int heads_q, int heads_kv, int total_q, int total_k, int head_dim,
                         long long do_stride, long long q_stride, long long k_stride, long long v_stride,
                         const int* cu_seqlens_q, const int* cu_seqlens_k, int seqlen_q, int seqlen_k,
                         int causal, int window, void* hip_stream);
int fa_attn_bwd_sink_f16(const void* dout, const void* q, const void* k, const void* v, const void* out,
                         const float* lse, void* dq, void* dk, void* dv, float* delta, int batch,
                         int heads_q, int heads_kv, int total_q, int total_k, int head_dim,
                         long long do_stride, long long q_stride, long long k_stride, long long v_stride,
                         const int* cu_seqlens_q, const int* cu_seqlens_k, int seqlen_q, int seqlen_k,
                         int causal, int window, void* hip_stream, const float* sinks, float* dsinks);
int fa_attn_bwd_sink_bf16(const void* dout, const void* q, const void* k, const void* v, const void* out,
                          const float* lse, void* dq, void* dk, void* dv, float* delta, int batch,
                          int heads_q, int heads_kv, int total_q, int total_k, int head_dim,
                          long long do_stride, long long q_stride, long long k_stride, long long v_stride,
                          const int* cu_seqlens_q, const int* cu_seqlens_k, int seqlen_q, int seqlen_k,
                          int causal, int window, void* hip_stream, const float* sinks, float* dsinks);

/* The dispatcher's decision (ref tier table :620-661): config id used by
 * fa_fwd_f16 for this shape.  The _ws entries may run the causal split tier
 * instead: check fa_fwd_split_pieces() first (> 0: the split tier runs with
 * that many 64-key tiles per piece, and this config is not used).
 *
 * The answer depends on the shape and on the CU count of the calling
 * thread's current HIP device (the W4 tier's tail and the paired tier's
 * one-round test size the grid from it, as the launch does; 256 if the
 * query fails).  The tier is the same for fp16 and bf16; fa_fwd_f16 /
 * fa_fwd_bf16 at head_dim 64 run the head_dim-64 twin of this tier, except
 * that non-causal head_dim-64 launches skip the paired tier (its d64 twin
 * trails the tier below there) and take the one-block-per-workgroup tier
 * only up to 16 blocks per head (S <= 1024), running the tier below it
 * otherwise.
 *
 * Config ids are positions in this build's table (fa_num_configs /
 * fa_config_info): they are not stable across releases (round 3 renumbered
 * 0-49 to 0-43 when the table was trimmed to the dispatched tiers; round 4
 * appended the head_dim-64 W4 configs 44-47; round 5 the paired
 * short-sequence configs 48-51, their four-block twins 52-55 and the
 * head_dim-64 twins of both, 56-63; round 6 the one-block-per-workgroup
 * configs 64-71, the causal singles-and-pairs mix 72-75 and the causal
 * groups planned on the host 76-79).  Select a tier by its
 * fa_config_info().name, not by a remembered id. */
int fa_select_config(int batch, int heads, int seq_len, int causal);

int fa_num_configs(void);
int fa_config_info(int config_id, fa_config_info_t* out);
int fa_kernel_attrs(int config_id, fa_kernel_attrs_t* out);

const char* fa_status_string(int status);
const char* fa_version(void);

#ifdef __cplusplus
}
#endif

#endif /* FA_MI355X_H */
