"""What the fa_attn_varlen_* test files share (a helper module, imported, never
executed by path): the base shape, the packed inputs, the reference call, the
C entries called raw, and a restatement of the uniform-mode workgroup map.

The entries attend token-major Q [T_q, Hq, D] to token-major K, V [T_k, Hkv, D]
with no cache.  Their contract is fa_prefill_varlen_*'s with len_b := nk_b, so
the references are that entry's:
  * the main gate is BIT-IDENTITY of O and LSE with
    flash_attention_prefill_varlen(q, k_cache, v_cache, cu_seqlens_q, kv_lens =
    nk) on a contiguous cache whose rows [0, nk_b) are sequence b's keys (the
    same block alignment, the same tile sequence);
  * beside it prefill_refs.refs / check on the unpacked result at the existing
    gates (fp16 O 1e-3 against the CPU oracle, bf16 O 5e-3 against fp32 torch,
    LSE 2^-10 max|score| + 1e-5), window_refs and sink_refs for the twins.
No new tolerance.

The base shape follows the packed tests: B = 5, nq = (0, 1, 127, 128, 321) in
T_q = 600 rows, Hq = 8, Hkv = 2, nk = (7, 201, 100, 198, 521) with cu_k
starting at 3 in T_k = 1100 rows: an empty query sequence that has keys, off_b
< 0 for element 2 (its 27 leading rows see nothing), starts on and off 128 and
64 boundaries, and tails of rows that belong to no sequence in all
three tensors.
"""
import functools

import torch

import decode_refs as dr
import prefill_refs as pr
import varlen_refs as vr

B, HQ, HKV = 5, 8, 2
NQ = (0, 1, 127, 128, 321)
NK = (7, 201, 100, 198, 521)
TQ, TK, K_START = 600, 1100, 3
CU_Q = vr.cu_of(NQ)
CU_K = vr.cu_of(NK, K_START)
SMAX, CAP = max(NQ), 576  # the padded tensors the references read
assert CU_Q[-1] == 577 and CU_K[-1] == 1030 and max(NK) <= CAP
F16, BF16 = torch.float16, torch.bfloat16

VARIANTS = ("", "_win", "_sink")
SYMBOLS = tuple("fa_attn_varlen" + v + t for v in VARIANTS for t in ("_f16", "_bf16"))


# ---- the uniform-mode map (csrc/fa_varlen_map.hpp, varlen_block_u with cu = nullptr) ----

def block_of_uniform(nseq, s, bt, i):
    """The kernel's decision for virtual block id i when there is no cu array:
    entry j of the map is j * s wherever the packed map reads cu[j] (total =
    nseq * s, so no clamp bites).  (b, r) or None."""
    total = nseq * s
    lo, hi = 0, nseq + 1
    while lo < hi:
        mid = (lo + hi) >> 1
        if min(mid * s, total) // bt + mid <= i:
            lo = mid + 1
        else:
            hi = mid
    if lo == 0 or lo > nseq:
        return None
    b = lo - 1
    start = min(b * s, total)
    n = max(min((b + 1) * s, total), start) - start
    r = i - (start // bt + b)
    return (b, r) if r < (n + bt - 1) // bt else None


# ---- inputs -------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def padded(d, dtype, b=B, hq=HQ, hkv=HKV, smax=SMAX, cap=CAP, seed=42):
    """(host fp16 bits, device (q [B,Hq,Smax,D], k, v [B,Hkv,cap,D]) of dtype):
    what the references and the reference call read."""
    q, k, v = dr.inputs(b, hq, hkv, smax, cap, d, seed)
    return (q, k, v), tuple(dr.dev(a).to(dtype) for a in (q, k, v))


def nan_cache(t, lens):
    """A copy of the cache [B,Hkv,cap,D] with NaN bits in the rows at or past each length."""
    t = t.clone()
    for i, n in enumerate(lens):
        t[i, :, int(n):].view(torch.int16).fill_(dr.NAN_BITS)
    return t


def packed(dev, nq=NQ, nk=NK, tq=TQ, tk=TK, k_start=K_START):
    """(q [T_q,Hq,D], k, v [T_k,Hkv,D]) packed from the padded tensors, NaN bits
    in every row of no sequence."""
    q, k, v = dev
    return (vr.pack(q, nq, total=tq, fill=dr.NAN_BITS),
            vr.pack(k, nk, total=tk, start=k_start, fill=dr.NAN_BITS),
            vr.pack(v, nk, total=tk, start=k_start, fill=dr.NAN_BITS))


@functools.lru_cache(maxsize=None)
def refs(d, dtype, causal, nq=NQ, nk=NK):
    """prefill_refs.refs at the base shape, computed once and shared."""
    host, dev = padded(d, dtype)
    return pr.refs(host, dev, nk, nq, causal, dtype)


def fused_qkv(qp, kp, vp):
    """One [T, Hq + 2 Hkv, D] buffer of NaN bits holding qp, kp and vp as its
    three head slices (T = the longest of them): the views (q, k, v)."""
    t = max(qp.shape[0], kp.shape[0])
    hq, hkv, d = qp.shape[1], kp.shape[1], qp.shape[2]
    buf = dr.nan_fill(torch.empty((t, hq + 2 * hkv, d), dtype=qp.dtype, device=qp.device))
    q, k, v = buf[:qp.shape[0], :hq], buf[:kp.shape[0], hq:hq + hkv], buf[:vp.shape[0], hq + hkv:]
    q.copy_(qp)
    k.copy_(kp)
    v.copy_(vp)
    return q, k, v


# ---- the C entries, raw -------------------------------------------------------------------

def entry(lib, variant, bf16):
    return getattr(lib, "fa_attn_varlen" + variant + ("_bf16" if bf16 else "_f16"))


def call(fn, variant, q, k, v, o, lse, batch, hq, hkv, tq, tk, d, cu_q, cu_k, causal, strides=(0, 0, 0),
         seqlen=(0, 0), window=0, sinks=None, stream=None):
    """One of the six entries with plain values (pointers as ints / c_void_p / None)."""
    mid = () if variant == "" else (window,)
    last = (sinks,) if variant == "_sink" else ()
    return fn(q, k, v, o, lse, batch, hq, hkv, tq, tk, d, *strides, cu_q, cu_k, *seqlen, int(causal), *mid,
              stream, *last)


def raw(variant, qp, kp, vp, out, lse, cu_q, cu_k, causal, window=0, sinks=None, seqlen=(0, 0), batch=None):
    """The C entry itself on device tensors, with the caller's own out AND lse
    buffers and the tensors' own token strides; synchronises, returns the status."""
    import fa_mi355x

    fn = entry(fa_mi355x.load_library(), variant, qp.dtype is BF16)
    if batch is None:
        batch = cu_q.shape[0] - 1
    rc = call(fn, variant, qp.data_ptr(), kp.data_ptr(), vp.data_ptr(), out.data_ptr(),
              None if lse is None else lse.data_ptr(), batch, qp.shape[1], kp.shape[1], qp.shape[0],
              kp.shape[0], qp.shape[2], None if cu_q is None else cu_q.data_ptr(),
              None if cu_k is None else cu_k.data_ptr(), causal,
              (qp.stride(0), kp.stride(0), vp.stride(0)), seqlen, window,
              None if sinks is None else sinks.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def unpack(out, lse, cu_q=CU_Q, smax=SMAX):
    """([B,Hq,Smax,D], [B,Hq,Smax]) of a packed result (unowned rows: 0 / -inf)."""
    return vr.unpack(out, cu_q, smax), vr.unpack(lse, cu_q, smax, fill=float("-inf"))


def same_rows(a, b, n):
    """The rows t < n_b of two unpacked (O, LSE) pairs agree bit for bit."""
    return all(torch.equal(a[0][bi, :, :nb].view(torch.int16), b[0][bi, :, :nb].view(torch.int16))
               and torch.equal(a[1][bi, :, :nb].view(torch.int32), b[1][bi, :, :nb].view(torch.int32))
               for bi, nb in enumerate(n))
