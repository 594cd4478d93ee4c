"""What the test files of the backward pass through the sliding window and the
attention sinks share (fa_attn_bwd_win_* / fa_attn_bwd_sink_*; a helper module,
imported, never executed by path): attn_bwd_refs' references with the window
mask and the sink, its gate on four tensors, an fp32 restatement of what the
kernels compute, the two loop bounds restated, and the C entries called raw.

  g_ref  float64 torch autograd as in attn_bwd_refs, row t of a sequence seeing
         the keys [lo, vis) with lo = max(0, nk - nq + t - W + 1) for W > 0, and
         the sink as an explicit extra softmax column whose value is zero, so
         that autograd returns dsinks too (summed over the sequences);
  g_16   the 16-bit baseline, extended the same way: the matmuls in the dtype,
         the softmax in fp32 over the scores and the sink, then cast;
  gate   attn_bwd_refs', unchanged, on (dq, dk, dv, dsinks):
           max|g - g_ref| <= 2 max|g_16 - g_ref| + u max|g_ref|.
No new tolerance.
"""
import functools
import math

import torch

import attn_bwd_refs as br
import attn_varlen_refs as ar
import sink_refs as sr
import varlen_refs as vr

F16, BF16 = br.F16, br.BF16
SYMBOLS = tuple("fa_attn_bwd" + v + t for v in ("_win", "_sink") for t in ("_f16", "_bf16"))
NAMES = ("dq", "dk", "dv", "dsinks")
BT = 64  # rows of the swept tiles (csrc/fa_attn_bwd_kernel.hpp kBwdTile)


# ---- the references ---------------------------------------------------------------------------

def visible(nq, nk, causal, window=0):
    """bool [nq, nk]: attn_bwd_refs.visible under the window (causal only)."""
    vis = br.visible(nq, nk, causal)
    if window > 0:
        assert causal
        t = torch.arange(nq)[:, None]
        j = torch.arange(nk)[None, :]
        vis = vis & (j >= nk - nq + t - window + 1)
    return vis


def _seq_grads(q, k, v, do, sinks, causal, window, low):
    """attn_bwd_refs._seq_grads with the window and the sink column: (dq, dk, dv[,
    dsinks]) of one sequence.  sinks: [Hq] float64 (float32 when `low`) or None."""
    nq, hq, d = q.shape
    nk, hkv = k.shape[0], k.shape[1]
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    leaves = (q, k, v)
    qh = q.permute(1, 0, 2)
    kh = k.permute(1, 0, 2).repeat_interleave(hq // hkv, 0)
    vh = v.permute(1, 0, 2).repeat_interleave(hq // hkv, 0)
    s = (qh @ kh.transpose(1, 2)) * (1.0 / math.sqrt(d))
    vis = visible(nq, nk, causal, window)
    seen = vis.any(1)
    # a row that sees no key: softmax over all keys (finite), then times 0
    mask = vis | ~seen[:, None]
    s = s.masked_fill(~mask, float("-inf"))
    if low:
        s = s.float()
    if sinks is not None:
        sinks = sinks.detach().clone().requires_grad_()
        leaves += (sinks,)
        s = torch.cat([s, sinks[:, None, None].expand(hq, nq, 1)], -1)
    p = torch.softmax(s, -1)
    if sinks is not None:
        p = p[..., :-1]  # the sink's value is zero
    if low:
        p = p.to(q.dtype)
    p = p * seen[None, :, None].to(p.dtype)
    o = (p @ vh).permute(1, 0, 2)
    return torch.autograd.grad(o, leaves, grad_outputs=do)


def reference(qp, kp, vp, dop, cu_q, cu_k, causal, low, window=0, sinks=None):
    """attn_bwd_refs.reference with the window and the sinks: float64 (dq, dk, dv)
    and, with sinks, dsinks [Hq] summed over the sequences."""
    dq = torch.zeros(qp.shape, dtype=torch.float64)
    dk = torch.zeros(kp.shape, dtype=torch.float64)
    dv = torch.zeros(vp.shape, dtype=torch.float64)
    ds = None if sinks is None else torch.zeros(sinks.shape, dtype=torch.float64)
    for (sq, nq), (sk, nk) in zip(vr.spans(cu_q, qp.shape[0]), vr.spans(cu_k, kp.shape[0])):
        if nq == 0 or nk == 0:
            continue  # no key: out = 0, so nothing reaches the sinks either
        args = [qp[sq:sq + nq], kp[sk:sk + nk], vp[sk:sk + nk], dop[sq:sq + nq]]
        sk_ = sinks
        if not low:
            args = [a.double() for a in args]
            sk_ = None if sinks is None else sinks.double()
        g = _seq_grads(*args, sk_, causal, window, low)
        dq[sq:sq + nq], dk[sk:sk + nk], dv[sk:sk + nk] = (x.double() for x in g[:3])
        if sinks is not None:
            ds += g[3].double()
    return (dq, dk, dv) if sinks is None else (dq, dk, dv, ds)


def formulas_f64(q, k, v, do, causal, window=0, sink=None):
    """The contract's formulas with plain loops, one head, float64 lists: (dq, dk,
    dv, dsink).  lse holds the sink; dsink = -sum_i exp(sink - lse_i) delta_i."""
    nq, nk, d = len(q), len(k), len(q[0])
    c = 1.0 / math.sqrt(d)
    off = nk - nq
    dot = lambda a, b: sum(x * y for x, y in zip(a, b))  # noqa: E731
    P = [[0.0] * nk for _ in range(nq)]
    o = [[0.0] * d for _ in range(nq)]
    lse = [float("-inf")] * nq
    for i in range(nq):
        hi = min(nk, off + i + 1) if causal else nk
        lo = max(0, off + i - window + 1) if window > 0 else 0
        e = {j: math.exp(c * dot(q[i], k[j])) for j in range(lo, hi)}
        z = sum(e.values()) + (math.exp(sink) if sink is not None else 0.0)
        if z == 0.0:
            continue
        lse[i] = math.log(z)
        for j in e:
            P[i][j] = e[j] / z
            for x in range(d):
                o[i][x] += P[i][j] * v[j][x]
    delta = [dot(do[i], o[i]) for i in range(nq)]
    dS = [[P[i][j] * (dot(do[i], v[j]) - delta[i]) for j in range(nk)] for i in range(nq)]
    dq = [[c * sum(dS[i][j] * k[j][x] for j in range(nk)) for x in range(d)] for i in range(nq)]
    dk = [[c * sum(dS[i][j] * q[i][x] for i in range(nq)) for x in range(d)] for j in range(nk)]
    dv = [[sum(P[i][j] * do[i][x] for i in range(nq)) for x in range(d)] for j in range(nk)]
    dsink = 0.0
    if sink is not None and sink != float("-inf"):
        dsink = -sum(math.exp(sink - lse[i]) * delta[i] for i in range(nq) if lse[i] != float("-inf"))
    return dq, dk, dv, dsink


def kernel_model(qp, kp, vp, dop, cu_q, cu_k, causal, window=0, sinks=None):
    """What the kernels compute, restated in fp32 torch on the CPU: the forward's
    out rounded to the 16-bit dtype and its lse in fp32; delta in fp32 from dout
    and that out; P and dS rounded to 16 bits as matrix operands; fp32 sums
    (GQA included) and one rounding of dq, dk, dv; dsinks from the fp32 delta.
    Returns (dq, dk, dv[, dsinks]) as float64."""
    dtype = qp.dtype
    hq, hkv, d = qp.shape[1], kp.shape[1], qp.shape[2]
    g, c = hq // hkv, 1.0 / math.sqrt(d)
    dq = torch.zeros(qp.shape, dtype=torch.float64)
    dk = torch.zeros(kp.shape, dtype=torch.float64)
    dv = torch.zeros(vp.shape, dtype=torch.float64)
    ds = None if sinks is None else torch.zeros(hq, dtype=torch.float32)
    for (sq, nq), (sk, nk) in zip(vr.spans(cu_q, qp.shape[0]), vr.spans(cu_k, kp.shape[0])):
        if nq == 0:
            continue
        if nk == 0:
            dq[sq:sq + nq] = 0
            continue
        q = qp[sq:sq + nq].float().permute(1, 0, 2)                       # [Hq, nq, D]
        do = dop[sq:sq + nq].float().permute(1, 0, 2)
        k = kp[sk:sk + nk].float().permute(1, 0, 2).repeat_interleave(g, 0)  # [Hq, nk, D]
        v = vp[sk:sk + nk].float().permute(1, 0, 2).repeat_interleave(g, 0)
        vis = visible(nq, nk, causal, window)[None]
        s = ((q @ k.transpose(1, 2)) * c).masked_fill(~vis, float("-inf"))
        z = s if sinks is None else torch.cat([s, sinks.float()[:, None, None].expand(hq, nq, 1)], -1)
        lse = torch.logsumexp(z, -1)                                        # fp32, -inf: nothing seen
        nl = torch.where(torch.isneginf(lse), torch.zeros_like(lse), lse)
        e = torch.where(vis, torch.exp(s - nl[..., None]), torch.zeros_like(s))
        e = torch.where(torch.isneginf(lse)[..., None], torch.zeros_like(e), e)
        out = (e @ v).to(dtype).float()                                     # the forward's out, rounded
        delta = (do * out).sum(-1)
        dp = do @ v.transpose(1, 2)
        p16 = e.to(dtype).float()
        ds16 = (e * (dp - delta[..., None])).to(dtype).float()
        dq[sq:sq + nq] = ((ds16 @ k) * c).to(dtype).permute(1, 0, 2).double()
        dk_h = (ds16.transpose(1, 2) @ q).view(hkv, g, nk, d).sum(1) * c
        dv_h = (p16.transpose(1, 2) @ do).view(hkv, g, nk, d).sum(1)
        dk[sk:sk + nk] = dk_h.to(dtype).permute(1, 0, 2).double()
        dv[sk:sk + nk] = dv_h.to(dtype).permute(1, 0, 2).double()
        if sinks is not None:
            w = torch.exp(sinks.float()[:, None] - nl)
            w = torch.where(torch.isneginf(lse) | torch.isneginf(sinks.float())[:, None], torch.zeros_like(w), w)
            ds -= (w * delta).sum(-1)
    return (dq, dk, dv) if sinks is None else (dq, dk, dv, ds.double())


def check_gate(got, gref, g16, dtype, what, owned=None, frac=1.0):
    """attn_bwd_refs.check_gate on three or four tensors (dsinks last, every
    element owned); prints each figure before asserting.  frac: the share of
    the gate the error has to stay within (1: the gate itself)."""
    terms = br.gate_terms(g16, gref, dtype)
    assert len(got) == len(gref) == len(g16)
    rows = []
    for i, (name, g, r, (base, top, gate)) in enumerate(zip(NAMES, got, gref, terms)):
        g = g.detach().cpu().double()
        if owned is not None and i < 3:
            g, r = g[owned[i]], r[owned[i]]
        assert bool(torch.isfinite(g).all()), (what, name, "not finite")
        err = float((g - r).abs().max()) if g.numel() else 0.0
        ratio = err / base if base > 0 else float("nan")
        print(f"{what} {name}: err {err:.3e} baseline {base:.3e} max|ref| {top:.3e} gate {gate:.3e} "
              f"err/baseline {ratio:.3f} err/gate {err / gate if gate > 0 else float('nan'):.3f}")
        rows.append((name, err, gate))
    for name, err, gate in rows:
        assert err <= frac * gate, (what, name, err, gate, frac)


# ---- inputs -----------------------------------------------------------------------------------

def base_sinks(hq=ar.HQ):
    return sr.draw_sinks(hq)


@functools.lru_cache(maxsize=None)
def base_refs(d, dtype, causal, window, with_sinks):
    """(g_ref, g_16) of attn_bwd_refs.base_inputs under the window and
    base_sinks(), computed once and shared."""
    (qp, kp, vp, dop), (cu_q, cu_k) = br.base_inputs(d, dtype)
    sinks = base_sinks() if with_sinks else None
    return (reference(qp, kp, vp, dop, cu_q, cu_k, causal, False, window, sinks),
            reference(qp, kp, vp, dop, cu_q, cu_k, causal, True, window, sinks))


# ---- the two loop bounds (csrc/fa_attn_bwd_kernel.hpp), restated ---------------------------------

def dkdv_sweep(nq, nk, window, k0, causal=True, bn=br.BN, bt=BT):
    """The dK/dV kernel's sweep for the key block at k0 of a sequence: (first
    64-row query tile, tile count).  window 0: none."""
    live = min(bn, nk - k0)
    off = nk - nq
    j0 = max(0, k0 - off) // bt if causal else 0
    jend = -(-nq // bt)
    if window > 0:
        last = k0 + live - 1 - off + window - 1
        jend = 0 if last < 0 else min(jend, last // bt + 1)
    return j0, max(0, jend - j0)


def dq_sweep(nq, nk, window, q0, causal=True, bm=128, bt=BT):
    """The dQ kernel's sweep for the query block at q0 of a sequence: (first
    64-key tile, one past the last)."""
    off = nk - nq
    kv_hi = max(0, min(nk, off + q0 + bm)) if causal else nk
    jt0 = max(0, off + q0 - window + 1) // bt if window > 0 else 0
    return jt0, -(-kv_hi // bt)


def tile_pairs(nq, nk, window, causal=True):
    """The (64-row query tile, 64-key tile) pairs of a sequence that hold a
    visible (row, key) pair: what the mask leaves of the work."""
    off = nk - nq
    n = 0
    for i in range(-(-nq // BT)):
        r0, r1 = BT * i, min(nq, BT * i + BT) - 1
        hi = min(nk - 1, off + r1) if causal else nk - 1
        lo = max(0, off + r0 - window + 1) if window > 0 else 0
        lo = max(lo, 0)
        if hi >= lo:
            n += hi // BT - lo // BT + 1
    return n


# ---- the C entries, raw ------------------------------------------------------------------------

def entry(lib, variant, bf16):
    return getattr(lib, "fa_attn_bwd" + variant + ("_bf16" if bf16 else "_f16"))


def call(fn, variant, dout, q, k, v, out, lse, dq, dk, dv, delta, batch, hq, hkv, tq, tk, d, cu_q, cu_k,
         causal, window=0, sinks=None, dsinks=None, strides=(0, 0, 0, 0), seqlen=(0, 0), stream=None):
    """One of the four entries with plain values (pointers as ints / c_void_p / None)."""
    last = (sinks, dsinks) if variant == "_sink" else ()
    mid = (window,) if variant else ()
    return fn(dout, q, k, v, out, lse, dq, dk, dv, delta, batch, hq, hkv, tq, tk, d, *strides, cu_q, cu_k,
              *seqlen, int(causal), *mid, stream, *last)


def raw(variant, dout, q, k, v, out, lse, grads, cu_q, cu_k, causal, window=0, sinks=None, dsinks=None):
    """The C entry itself ("": fa_attn_varlen_bwd_*) on device tensors with the
    caller's own gradient buffers and the tensors' own token strides;
    synchronises, returns the status."""
    import fa_mi355x

    lib = fa_mi355x.load_library()
    fn = entry(lib, variant, q.dtype is BF16) if variant else br.entry(lib, q.dtype is BF16)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    delta = torch.empty((q.shape[1], q.shape[0]), dtype=torch.float32, device=q.device)
    rc = call(fn, variant, ptr(dout), ptr(q), ptr(k), ptr(v), ptr(out), ptr(lse), *(ptr(g) for g in grads),
              ptr(delta), cu_q.shape[0] - 1, q.shape[1], k.shape[1], q.shape[0], k.shape[0], q.shape[2], ptr(cu_q),
              ptr(cu_k), causal, window, ptr(sinks), ptr(dsinks),
              (dout.stride(0), q.stride(0), k.stride(0), v.stride(0)), (0, 0),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc
