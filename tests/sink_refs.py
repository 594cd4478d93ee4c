"""What the attention-sink test files share (a helper module, imported, never
executed by path): a float64 restatement of the contract with sinks, the two
identities that carry a result without sinks to one with them, the references
built on them, the census expectation with sinks and the comparisons.

The contract (include/fa_mi355x.h, the fa_*_sink_* entries): sinks[h] is one
logit per query head, in the units of the scaled scores, that joins the softmax
denominator and contributes no value.  Over the keys j a row of head h sees
(the `_win` twin's keys: causal, kv_lens, q_lens and window unchanged)

    den = exp(sinks[h]) + sum_j exp(s_j),  O = sum_j exp(s_j) v_j / den,  LSE = log(den)

and a row that sees no key gives O = 0, LSE = sinks[h].  With O0, LSE0 the
result without sinks this is

    O = O0 sigmoid(LSE0 - sinks[h]),   LSE = logaddexp(LSE0, sinks[h])

(transform()).  References and gates are the project's and nothing here widens
one: fp16 O against the CPU-oracle rows carried over by the identities (1e-3),
bf16 O against fp32 torch with the sink as an explicit extra softmax column
(5e-3), LSE against float64 at 2^-10 max(|scaled score|, |sink|) + 1e-5; the
census at keysense_inputs' gates (relative 2^-10 / 2^-7 plus 1e-7).
tests/test_sinks_cpu.py holds the three references against one another at half
of each gate.
"""
import math

import numpy as np
import torch

import decode_refs as dr
import keysense_inputs as ks
import prefill_refs as pr
import window_refs as wr

FAMILIES = ("fa_decode", "fa_prefill", "fa_prefill_varlen")
FORMS = ("", "_paged", "_kv8", "_paged_kv8")


def symbol(fam, form, bf16, variant="_sink"):
    return fam + variant + form + ("_bf16" if bf16 else "_f16")


def sinks_np(sinks):
    """float64 [Hq] of a sinks tensor / sequence."""
    if isinstance(sinks, torch.Tensor):
        return sinks.detach().double().cpu().numpy()
    return np.asarray(sinks, dtype=np.float64)


def draw_sinks(hq, seed=5, std=math.sqrt(2.0)):
    """float32 [Hq] from N(0, 2) (variance 2), on the host."""
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(hq, generator=gen, dtype=torch.float64) * std).float()


# ---- the contract, restated ----------------------------------------------------------

def contract_f64(q, k, v, kv_lens, q_lens, window, sinks, causal=True, with_smax=False):
    """window_refs.contract_f64 with the sink column (and, causal=False, every
    key below the length visible: window must be 0 then), in float64 numpy with
    its own arithmetic: the softmax runs over the row's scores and the sink
    together, and the sink's column meets no value.  sinks: [Hq] (None: no
    column).  Returns (O, LSE, written[, max |scaled score or sink|]); unwritten
    rows are NaN; rows that see no key 0 / sinks[h]."""
    assert causal or window == 0
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    b, hq, sq, d = q.shape
    hkv, cap = k.shape[1], k.shape[2]
    g = hq // hkv
    sk = None if sinks is None else sinks_np(sinks)
    o = np.full((b, hq, sq, d), np.nan)
    lse = np.full((b, hq, sq), np.nan)
    written = np.zeros((b, sq), bool)
    finite = [] if sk is None else [abs(x) for x in sk if np.isfinite(x)]
    smax = max(finite) if finite else 0.0
    for bi in range(b):
        n_b = sq if q_lens is None else min(max(int(q_lens[bi]), 0), sq)
        len_b = cap if kv_lens is None else min(max(int(kv_lens[bi]), 0), cap)
        for t in range(n_b):
            written[bi, t] = True
            pos = len_b - n_b + t if causal else len_b - 1
            first = 0 if window == 0 else max(0, pos - window + 1)
            last = min(pos, len_b - 1)
            for h in range(hq):
                col = -np.inf if sk is None else sk[h]
                s = (k[bi, h // g, first:last + 1] @ q[bi, h, t] / math.sqrt(d) if last >= first
                     else np.zeros(0))
                if s.size:
                    smax = max(smax, float(np.abs(s).max()))
                z = np.concatenate([s, [col]])
                m = z.max()
                if np.isneginf(m):
                    o[bi, h, t] = 0.0
                    lse[bi, h, t] = -np.inf
                    continue
                e = np.exp(z - m)
                p = e / e.sum()
                o[bi, h, t] = p[:-1] @ v[bi, h // g, first:last + 1] if s.size else 0.0
                lse[bi, h, t] = m + math.log(e.sum())
    return (o, lse, written, smax) if with_smax else (o, lse, written)


# ---- the identities -------------------------------------------------------------------

def transform(o0, lse0, sinks):
    """(O, LSE) float64 numpy with sinks from the result without: O0 [B,Hq,Sq,D]
    (float array), LSE0 [B,Hq,Sq] float64 (-inf: the row saw no key)."""
    sk = sinks_np(sinks)[None, :, None]
    o0 = np.asarray(o0, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        gap = lse0 - sk                                        # -inf - -inf: NaN, no key and no sink
        w = np.where(np.isnan(gap), 0.0, 1.0 / (1.0 + np.exp(-gap)))
        lse = np.where(np.isnan(gap), -np.inf, np.logaddexp(lse0, sk))
    return o0 * w[..., None], lse


def _f64(x):
    """uint16 fp16 bits, or a torch tensor -> float64 numpy."""
    if isinstance(x, torch.Tensor):
        return x.detach().double().cpu().numpy()
    return x.view(np.float16).astype(np.float64) if x.dtype == np.uint16 else np.asarray(x, np.float64)


def _smax_with(smax, sinks):
    sk = sinks_np(sinks)
    fin = np.abs(sk[np.isfinite(sk)])
    return max(float(smax), float(fin.max()) if fin.size else 0.0)


def ref_torch(q, k, v, lens, window, q_lens, sinks, causal=True):
    """fp32 torch on the tensors' device with the sink as an explicit extra
    softmax column (its value row is zero): (O [B,Hq,Sq,D], LSE [B,Hq,Sq]).
    Rows t >= n_b: zeros / the sink."""
    assert causal or window == 0
    b, hq, sq, d = q.shape
    hkv, cap = k.shape[1], k.shape[2]
    g = hq // hkv
    dev = q.device
    lens = (torch.full((b,), cap, device=dev) if lens is None
            else torch.as_tensor(lens, device=dev).long().clamp(0, cap))
    n = torch.full((b,), sq, device=dev) if q_lens is None else torch.as_tensor(q_lens, device=dev).long().clamp(0, sq)
    key = torch.arange(cap, device=dev)
    live = key[None, :] < lens[:, None]
    kf = torch.where(live[:, None, :, None], k.float(), 0.0).repeat_interleave(g, 1)
    vf = torch.where(live[:, None, :, None], v.float(), 0.0).repeat_interleave(g, 1)
    s = q.float() @ kf.transpose(-1, -2) / math.sqrt(d)
    t = torch.arange(sq, device=dev)[None, :]
    vis = live[:, None, :] & (t < n[:, None])[:, :, None]
    if causal:
        pos = (lens - n)[:, None] + t
        vis = vis & (key[None, None, :] <= pos[:, :, None])
        if window > 0:
            vis = vis & (key[None, None, :] > (pos - window)[:, :, None])
    s = s.masked_fill(~vis[:, None], float("-inf"))
    col = torch.as_tensor(sinks, dtype=torch.float32, device=dev)[None, :, None, None].expand(b, hq, sq, 1)
    z = torch.cat([s, col], -1)
    lse = torch.logsumexp(z, -1)
    p = torch.nan_to_num(torch.exp(z - lse[..., None]), nan=0.0)
    return p[..., :-1] @ vf, lse


def refs(host, dev, kv_lens, q_lens, window, dtype, sinks, causal=True):
    """(O reference, float64 LSE, max |scaled score or sink|).  fp16 with host
    bits: the CPU-oracle rows and the float64 LSE without sinks (window_refs;
    prefill_refs when not causal), carried over by transform() -- a float64
    numpy O.  Else fp32 torch with the extra column, and the float64 LSE by
    logaddexp."""
    use_host = dtype is torch.float16 and host is not None
    src = host if use_host else dev  # (a bf16 run's references read the bf16 inputs)
    if causal:
        lse0, smax = wr.lse_f64(src[0], src[1], kv_lens, q_lens, window)
    else:
        assert window == 0
        lse0, smax = pr.lse_rows(*src, kv_lens, q_lens, False)
    if use_host:
        ro = wr.oracle_rows(*host, kv_lens, q_lens, window) if causal else \
            pr.oracle_rows(*host, kv_lens, q_lens, False)
        ro, lref = transform(_f64(ro), lse0, sinks)
    else:
        ro = ref_torch(*dev, kv_lens, window, q_lens, sinks, causal)[0]
        lref = transform(np.zeros(lse0.shape + (1,)), lse0, sinks)[1]
    return ro, lref, _smax_with(smax, sinks)


def lse_gate(smax):
    return 2.0 ** -10 * smax + 1e-5


def check(out, lse, refs_, q_lens, dtype, what):
    """The project's gates on the rows t < n_b of every element: |O - ref| <=
    1e-3 (fp16) / 5e-3 (bf16), LSE within 2^-10 smax + 1e-5 with -inf exactly
    where the reference has it, and rows that saw no key exactly zero."""
    ro, lref, smax = refs_
    b, _, sq = lref.shape
    gate = dr.GATE_F16 if dtype is torch.float16 else dr.GATE_BF16
    got_o, got_l = _f64(out), _f64(lse)
    ro = _f64(ro)
    for bi, n in enumerate(pr.n_rows(q_lens, b, sq)):
        if n == 0:
            continue
        o, r = got_o[bi, :, :n], ro[bi, :, :n]
        assert np.isfinite(o).all(), f"{what} b={bi}"
        err = float(np.abs(o - r).max())
        ll, lr = got_l[bi, :, :n], lref[bi, :, :n]
        empty = np.isneginf(lr)
        assert np.array_equal(np.isneginf(ll), empty), f"{what} b={bi}: -inf rows differ"
        lerr = float(np.abs(ll[~empty] - lr[~empty]).max()) if (~empty).any() else 0.0
        print(f"{what} b={bi}: max_abs_diff {err:.3e} gate {gate:.1e} | lse err {lerr:.3e} gate {lse_gate(smax):.3e}")
        assert err <= gate, (what, bi, err)
        assert lerr <= lse_gate(smax), (what, bi, lerr, lse_gate(smax))


# ---- census ---------------------------------------------------------------------------

def census_sinks(hq, score):
    """(sinks float32 [Hq], m int64 [Hq]): sinks[h] = score + ln(m_h) with m_h =
    1 + 2 h, so head h's sink weighs exactly as m_h more keys of the census."""
    m = 1 + 2 * torch.arange(hq)
    return (score + torch.log(m.double())).float(), m


def census_expected(counts, lo, hi, score, m):
    """(O float64 [..., D], LSE float64 [...]) of rows that see the keys [lo, hi)
    at the common scaled score, beside a sink worth m (int64, broadcastable to
    lo's shape) keys: n becomes n + m in the denominator, LSE = score + log(n +
    m).  A row without keys: O = 0, LSE = score + log m, its sink."""
    lo = torch.as_tensor(lo).to(counts.device).long().clamp(min=0)
    hi = torch.maximum(torch.as_tensor(hi).to(counts.device).long(), lo)
    n = hi - lo
    tot = (n + torch.as_tensor(m).to(counts.device).long()).double()
    o = (counts[hi] - counts[lo]).double() / tot[..., None]
    return o, score + torch.log(tot)


def check_census(o, lo, hi, counts, score, m, what, lse=None, dtype=None):
    """window_refs.check_census beside sinks worth m[head] keys: o [..., Hq, rows,
    D]; lo, hi broadcastable to [..., Hq, rows]; m int64 [Hq].  The LSE gate is
    2^-10 max(|score|, |sink|) + 1e-5."""
    dtype = dtype or o.dtype
    rel = ks.REL_GATE[dtype]
    got = ks._t64(o)
    lo = torch.as_tensor(lo).to(got.device).long().expand(got.shape[:-1])
    hi = torch.as_tensor(hi).to(got.device).long().expand(got.shape[:-1])
    mm = torch.as_tensor(m).to(got.device).long()[:, None].expand(got.shape[:-1])
    want, lse_want = census_expected(counts.to(got.device), lo, hi, score, mm)
    tol = rel * want.abs() + ks.ABS_GATE
    tol = torch.where((hi <= lo)[..., None], torch.zeros_like(tol), tol)  # unseen rows: exactly 0
    diff = torch.nan_to_num((got - want).abs(), nan=float("inf"), posinf=float("inf"))
    relerr = torch.where(want > 0, diff / want.clamp(min=1e-300), torch.zeros_like(diff))
    res = ks.Result(True, what, float(relerr.max()) if relerr.numel() else 0.0, rel)
    bad = diff > tol
    if bool(bad.any()):
        i = ks._where(torch.where(bad, diff / (tol + 1e-30), torch.zeros_like(diff)).argmax(), got.shape)
        a, z, mi = int(lo[i[:-1]]), int(hi[i[:-1]]), int(mm[i[:-1]])
        res.ok = res.o_ok = False
        res.msg = (f"{ks._name_row(i[:-1])} column {i[-1]}: got {float(got[i]):.6g}, wanted "
                   f"{int(counts[z, i[-1]] - counts[a, i[-1]])} of {z - a} keys + a sink worth {mi} = "
                   f"{float(want[i]):.6g} ({int(bad.sum())} elements past the gate)")
    if lse is not None:
        sink_max = max(abs(score + math.log(float(x))) for x in torch.as_tensor(m).flatten())
        res.lse_gate = 2.0 ** -10 * max(abs(score), sink_max) + 1e-5
        ok, res.lse_err, msg = ks._check_lse(lse, lse_want, res.lse_gate)
        if not ok:
            res.ok = res.lse_ok = False
            res.msg = (res.msg + "; " if res.msg else "") + msg
    return res


def census_signal(lo, hi, m_max):
    """The smallest relative change of a census denominator when a sink is
    indexed by a wrong head, counted twice or dropped, over rows that see a key:
    1 / (n + m_max + 1) at the largest n."""
    n = np.asarray(hi) - np.asarray(lo)
    n = n[n > 0]
    return 1.0 / (float(n.max()) + m_max + 1)
