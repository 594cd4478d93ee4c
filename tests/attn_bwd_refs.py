"""What the fa_attn_varlen_bwd_* test files share (a helper module, imported,
never executed by path): the references of the backward pass, the gate derived
from them, the base inputs, the C entries called raw, and a restatement of the
dK/dV kernel's key-block map.

There was no gradient tolerance in the project, so the gate is derived, not chosen:

  g_ref  float64 torch autograd on the CPU over each sequence's own problem
         (softmax attention under the forward's mask, GQA by repeat_interleave)
         on the exact 16-bit input values;
  g_16   the same composition evaluated in the 16-bit dtype as a naive user
         would write it (matmuls in the dtype, softmax in fp32 then cast), with
         torch autograd;
  gate   per tensor (dq, dk, dv):
           max|g - g_ref| <= 2 max|g_16 - g_ref| + u max|g_ref|,
         u = 2^-11 (fp16) or 2^-8 (bf16).  The factor 2 is the margin: the
         kernel rounds P and dS to 16 bits as the baseline does but sums in
         another order; the second term is one rounding of the output itself.

The base shape is attn_varlen_refs': B = 5, nq = (0, 1, 127, 128, 321) in 600
rows, nk = (7, 201, 100, 198, 521) from row 3 of 1100, Hq = 8, Hkv = 2.
"""
import functools
import math

import torch

import attn_varlen_refs as ar
import decode_refs as dr
import varlen_refs as vr

F16, BF16 = torch.float16, torch.bfloat16
SYMBOLS = ("fa_attn_varlen_bwd_f16", "fa_attn_varlen_bwd_bf16")
BN = 128  # keys per dK/dV workgroup (csrc/fa_attn_bwd_kernel.hpp kBwdBN)
U = {F16: 2.0 ** -11, BF16: 2.0 ** -8}


# ---- the references ---------------------------------------------------------------------------

def visible(nq, nk, causal):
    """bool [nq, nk]: row t of a sequence sees key j (bottom-right aligned)."""
    if not causal:
        return torch.ones((nq, nk), dtype=torch.bool)
    t = torch.arange(nq)[:, None]
    j = torch.arange(nk)[None, :]
    return j < nk - nq + t + 1


def _seq_grads(q, k, v, do, causal, low):
    """(dq, dk, dv) of one sequence by torch autograd: q, do [nq, Hq, D], k, v
    [nk, Hkv, D] (float64 values, or the 16-bit dtype when `low`)."""
    nq, hq, d = q.shape
    nk, hkv = k.shape[0], k.shape[1]
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    qh = q.permute(1, 0, 2)                                   # [Hq, nq, D]
    kh = k.permute(1, 0, 2).repeat_interleave(hq // hkv, 0)   # [Hq, nk, D]
    vh = v.permute(1, 0, 2).repeat_interleave(hq // hkv, 0)
    s = (qh @ kh.transpose(1, 2)) * (1.0 / math.sqrt(d))
    vis = visible(nq, nk, causal)
    seen = vis.any(1)
    # a row that sees no key: softmax over all keys (finite), then times 0
    mask = vis | ~seen[:, None]
    s = s.masked_fill(~mask, float("-inf"))
    if low:
        p = torch.softmax(s.float(), -1).to(q.dtype)
    else:
        p = torch.softmax(s, -1)
    p = p * seen[None, :, None].to(p.dtype)
    o = (p @ vh).permute(1, 0, 2)                             # [nq, Hq, D]
    return torch.autograd.grad(o, (q, k, v), grad_outputs=do)


def reference(qp, kp, vp, dop, cu_q, cu_k, causal, low):
    """float64 (dq [T_q,Hq,D], dk, dv [T_k,Hkv,D]) of packed 16-bit CPU tensors:
    g_ref (low=False) or the 16-bit baseline g_16 (low=True).  Rows of no
    sequence are never read and come back as zeros."""
    dq = torch.zeros(qp.shape, dtype=torch.float64)
    dk = torch.zeros(kp.shape, dtype=torch.float64)
    dv = torch.zeros(vp.shape, dtype=torch.float64)
    for (sq, nq), (sk, nk) in zip(vr.spans(cu_q, qp.shape[0]), vr.spans(cu_k, kp.shape[0])):
        if nq == 0 or nk == 0:
            continue
        args = [qp[sq:sq + nq], kp[sk:sk + nk], vp[sk:sk + nk], dop[sq:sq + nq]]
        if not low:
            args = [a.double() for a in args]
        g = _seq_grads(*args, causal, low)
        dq[sq:sq + nq], dk[sk:sk + nk], dv[sk:sk + nk] = (x.double() for x in g)
    return dq, dk, dv


def formulas_f64(q, k, v, do, causal):
    """The contract's formulas with plain loops, one head, float64 lists:
    (dq, dk, dv, P).  The hand check of `reference`."""
    nq, nk, d = len(q), len(k), len(q[0])
    c = 1.0 / math.sqrt(d)
    dot = lambda a, b: sum(x * y for x, y in zip(a, b))  # noqa: E731
    P = [[0.0] * nk for _ in range(nq)]
    o = [[0.0] * d for _ in range(nq)]
    for i in range(nq):
        vis = [j for j in range(nk) if not causal or j < nk - nq + i + 1]
        if not vis:
            continue
        e = {j: math.exp(c * dot(q[i], k[j])) for j in vis}
        z = sum(e.values())
        for j in vis:
            P[i][j] = e[j] / z
            for x in range(d):
                o[i][x] += P[i][j] * v[j][x]
    delta = [dot(do[i], o[i]) for i in range(nq)]
    dS = [[P[i][j] * (dot(do[i], v[j]) - delta[i]) for j in range(nk)] for i in range(nq)]
    dq = [[c * sum(dS[i][j] * k[j][x] for j in range(nk)) for x in range(d)] for i in range(nq)]
    dk = [[c * sum(dS[i][j] * q[i][x] for i in range(nq)) for x in range(d)] for j in range(nk)]
    dv = [[sum(P[i][j] * do[i][x] for i in range(nq)) for x in range(d)] for j in range(nk)]
    return dq, dk, dv, P


def gate_terms(g16, gref, dtype):
    """Per tensor (max|g_16 - g_ref|, max|g_ref|, the gate)."""
    out = []
    for a, r in zip(g16, gref):
        base, top = float((a - r).abs().max()), float(r.abs().max())
        out.append((base, top, 2.0 * base + U[dtype] * top))
    return out


def check_gate(got, gref, g16, dtype, what, owned=None):
    """The gate on (dq, dk, dv) device or host tensors; prints each figure
    before asserting.  owned: per tensor a bool row mask to compare on (the
    rows of no sequence hold whatever the caller put there)."""
    terms = gate_terms(g16, gref, dtype)
    ratios = []
    for i, (name, g, r, (base, top, gate)) in enumerate(zip(("dq", "dk", "dv"), got, gref, terms)):
        g = g.detach().cpu().double()
        if owned is not None:
            g, r = g[owned[i]], r[owned[i]]
        assert bool(torch.isfinite(g).all()), (what, name, "not finite")
        err = float((g - r).abs().max()) if g.numel() else 0.0
        ratio = err / base if base > 0 else float("nan")
        print(f"{what} {name}: err {err:.3e} baseline {base:.3e} max|ref| {top:.3e} gate {gate:.3e} "
              f"err/baseline {ratio:.3f}")
        ratios.append((name, err, gate))
    for name, err, gate in ratios:
        assert err <= gate, (what, name, err, gate)


# ---- inputs -----------------------------------------------------------------------------------

def host16(bits, dtype):
    """uint16 fp16 bits (numpy) -> a CPU tensor of dtype with those values."""
    import numpy as np

    return torch.from_numpy(np.array(bits, dtype=np.uint16).view(np.int16)).view(F16).to(dtype)


def owned_masks(cu_q=ar.CU_Q, cu_k=ar.CU_K, tq=ar.TQ, tk=ar.TK):
    oq = torch.from_numpy(vr.owned_rows(cu_q, tq))
    ok = torch.from_numpy(vr.owned_rows(cu_k, tk))
    return oq, ok, ok


def nan_unowned(t, own):
    """NaN bits in the rows of no sequence (in place); returns t."""
    t.view(torch.int16)[~own] = dr.NAN_BITS
    return t


def make_dout(shape, dtype, seed=7):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32).to(dtype)


@functools.lru_cache(maxsize=None)
def base_inputs(d, dtype, nq=ar.NQ, nk=ar.NK, q_scale=1.0):
    """Packed CPU tensors (q [600,8,D], k, v [1100,2,D], dout like q) of the
    base shape, NaN bits in every row of no sequence; (cu_q, cu_k) beside them."""
    q, k, v = (host16(a, dtype) for a in dr.inputs(ar.B, ar.HQ, ar.HKV, ar.SMAX, ar.CAP, d, 42))
    if q_scale != 1.0:
        q = (q.float() * q_scale).to(dtype)
    cu_q, cu_k = vr.cu_of(nq), vr.cu_of(nk, ar.K_START)
    qp = vr.pack(q, nq, total=ar.TQ, fill=dr.NAN_BITS)
    kp = vr.pack(k, nk, total=ar.TK, start=ar.K_START, fill=dr.NAN_BITS)
    vp = vr.pack(v, nk, total=ar.TK, start=ar.K_START, fill=dr.NAN_BITS)
    dop = nan_unowned(make_dout(qp.shape, dtype), torch.from_numpy(vr.owned_rows(cu_q, ar.TQ)))
    return (qp, kp, vp, dop), (cu_q, cu_k)


@functools.lru_cache(maxsize=None)
def base_refs(d, dtype, causal, nq=ar.NQ, nk=ar.NK, q_scale=1.0):
    """(g_ref, g_16) of base_inputs, computed once and shared."""
    (qp, kp, vp, dop), (cu_q, cu_k) = base_inputs(d, dtype, nq, nk, q_scale)
    return (reference(qp, kp, vp, dop, cu_q, cu_k, causal, False),
            reference(qp, kp, vp, dop, cu_q, cu_k, causal, True))


# ---- the dK/dV kernel's key-block map ----------------------------------------------------------

def key_block_of(cu_q, cu_k, tq, tk, causal, i, bn=BN, bt=64):
    """The dK/dV kernel's decision for virtual key-block id i: None ("return")
    or (b, r, j0, ntiles): block r of sequence b's keys by the packed map on
    cu_seqlens_k, then the first 64-row query tile it sweeps and their count."""
    hit = vr.block_of(cu_k, tk, bn, i)
    if hit is None:
        return None
    b, r = hit
    nq = vr.spans(cu_q, tq)[b][1]
    nk = vr.spans(cu_k, tk)[b][1]
    off = nk - nq
    j0 = max(0, r * bn - off) // bt if causal else 0
    return b, r, j0, max(0, -(-nq // bt) - j0)


# ---- the C entries, raw ------------------------------------------------------------------------

def entry(lib, bf16):
    return getattr(lib, "fa_attn_varlen_bwd" + ("_bf16" if bf16 else "_f16"))


def call(fn, dout, q, k, v, out, lse, dq, dk, dv, delta, batch, hq, hkv, tq, tk, d, cu_q, cu_k, causal,
         strides=(0, 0, 0, 0), seqlen=(0, 0), stream=None):
    """One of the two entries with plain values (pointers as ints / c_void_p / None)."""
    return fn(dout, q, k, v, out, lse, dq, dk, dv, delta, batch, hq, hkv, tq, tk, d, *strides, cu_q, cu_k,
              *seqlen, int(causal), stream)
