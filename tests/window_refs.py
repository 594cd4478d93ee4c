"""What the sliding-window test files share (a helper module, imported, never
executed by path): the visible interval of the windowed contract, a float64
restatement of it, the windowed census expectation and the windowed
references.

The contract (include/fa_mi355x.h, the fa_*_win_* entries): with W >= 1 and
pos = off_b + t (prefill: off_b = len_b - n_b; decode is the case n_b = Sq) row
t sees the keys j with max(0, pos - W + 1) <= j <= min(pos, len_b - 1), i.e.
the half-open interval [lo, hi); W = 0 is no window (lo = 0).

References and gates are the project's (decode_refs, prefill_refs,
keysense_inputs); nothing here widens one:
  * fp16 O: the CPU oracle, one call per row over the row's own keys K[lo:hi]
    with the query at their last position (causal, so it sees them all), gate
    1e-3;
  * bf16 O: fp32 torch with the window as a mask (decode_refs.ref_torch's
    style), gate 5e-3;
  * LSE: float64, gate 2^-10 max|scaled score| + 1e-5;
  * census: O = (counts[hi] - counts[lo]) / (hi - lo) in integers then float64,
    LSE = score + log(hi - lo), at keysense_inputs' gates (relative 2^-10 /
    2^-7 plus 1e-7; LSE 1e-5 at score 0, else 2^-10 |score| + 1e-5).  A key too
    many or too few at either edge turns a column's c of n into (c +- 1) of
    (n +- 1): about 1/c - 1/n relative.  In the stripe layout c <= ceil(n / D)
    <= 4 at the sizes used, so the move is >= 20 %; in the tile layout c <= 64
    and n <= 200 where a window cuts, so it is >= 2^-6.6: past the gate in
    both types.
"""
import math

import numpy as np
import torch

import decode_refs as dr
import keysense_inputs as ks
import oracle
import prefill_refs as pr


def interval(kv_lens, q_lens, b, sq, cap, window):
    """(lo, hi) int64 [B, Sq] of the contract for rows t < n_b (an empty row has
    lo == hi); rows t >= n_b hold -1 in both."""
    lo = np.full((b, sq), -1, np.int64)
    hi = np.full((b, sq), -1, np.int64)
    for bi, (n, ln) in enumerate(zip(pr.n_rows(q_lens, b, sq), pr.n_keys(kv_lens, b, cap))):
        pos = ln - n + np.arange(n)
        h = np.clip(pos + 1, 0, ln)
        lw = np.maximum(pos - window + 1, 0) if window > 0 else np.zeros(n, np.int64)
        hi[bi, :n] = h
        lo[bi, :n] = np.minimum(lw, h)
    return lo, hi


def block_lo(kv_lens, q_lens, b, sq, cap, window, bm=128):
    """[B][blocks] the first key any row of each bm-row query block sees (the
    `lo` of the never-read guarantee); blocks at or past n_b: None."""
    out = []
    for n, ln in zip(pr.n_rows(q_lens, b, sq), pr.n_keys(kv_lens, b, cap)):
        out.append([max(0, ln - n + q0 - window + 1) if q0 < n else None for q0 in range(0, sq, bm)])
    return out


def contract_f64(q, k, v, kv_lens, q_lens, window, with_smax=False):
    """The windowed contract restated in float64 numpy, one row at a time, with
    its own arithmetic (nothing shared with interval() or the references).
    q [B,Hq,Sq,D], k, v [B,Hkv,cap,D] float arrays.  Returns (O, LSE, written
    [B,Sq] bool[, max |scaled score| of a visible key]); unwritten rows are
    NaN, rows that see no key 0 / -inf."""
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    b, hq, sq, d = q.shape
    hkv, cap = k.shape[1], k.shape[2]
    g = hq // hkv
    o = np.full((b, hq, sq, d), np.nan)
    lse = np.full((b, hq, sq), np.nan)
    written = np.zeros((b, sq), bool)
    smax = 0.0
    for bi in range(b):
        n_b = sq if q_lens is None else min(max(int(q_lens[bi]), 0), sq)
        len_b = cap if kv_lens is None else min(max(int(kv_lens[bi]), 0), cap)
        for t in range(n_b):
            written[bi, t] = True
            pos = len_b - n_b + t
            first = 0 if window == 0 else max(0, pos - window + 1)
            last = min(pos, len_b - 1)
            for h in range(hq):
                if last < first:
                    o[bi, h, t] = 0.0
                    lse[bi, h, t] = -np.inf
                    continue
                s = k[bi, h // g, first:last + 1] @ q[bi, h, t] / math.sqrt(d)
                m = s.max()
                smax = max(smax, float(np.abs(s).max()))
                e = np.exp(s - m)
                o[bi, h, t] = (e / e.sum()) @ v[bi, h // g, first:last + 1]
                lse[bi, h, t] = m + math.log(e.sum())
    return (o, lse, written, smax) if with_smax else (o, lse, written)


# ---- census -------------------------------------------------------------------------

def census_score(qval, kval, d):
    """The one scaled score of a census with Q = qval and K = kval everywhere."""
    return qval * kval * d / math.sqrt(d)


def census_expected(counts, lo, hi, score):
    """(O float64 [..., D], LSE float64 [...]) of rows that see the keys
    [lo, hi) (int64 tensors; hi <= lo: none) at the common scaled score."""
    lo = torch.as_tensor(lo).to(counts.device).long().clamp(min=0)
    hi = torch.maximum(torch.as_tensor(hi).to(counts.device).long(), lo)
    n = hi - lo
    o = (counts[hi] - counts[lo]).double() / n.clamp(min=1).double()[..., None]
    lse = torch.where(n > 0, score + torch.log(n.clamp(min=1).double()),
                      torch.full(n.shape, float("-inf"), dtype=torch.float64, device=n.device))
    return o, lse


def census_lse_gate(score):
    return 1e-5 if score == 0 else 2.0 ** -10 * abs(score) + 1e-5


def check_census(o, lo, hi, counts, score, what, lse=None, dtype=None):
    """keysense_inputs.check_census for an interval: o [..., rows, D] against
    census_expected at the same gates."""
    dtype = dtype or o.dtype
    rel = ks.REL_GATE[dtype]
    got = ks._t64(o)
    lo = torch.as_tensor(lo).to(got.device).long().expand(got.shape[:-1])
    hi = torch.as_tensor(hi).to(got.device).long().expand(got.shape[:-1])
    want, lse_want = census_expected(counts.to(got.device), lo, hi, score)
    tol = rel * want.abs() + ks.ABS_GATE
    tol = torch.where((hi <= lo)[..., None], torch.zeros_like(tol), tol)  # unseen rows: exactly 0
    diff = torch.nan_to_num((got - want).abs(), nan=float("inf"), posinf=float("inf"))
    relerr = torch.where(want > 0, diff / want.clamp(min=1e-300), torch.zeros_like(diff))
    res = ks.Result(True, what, float(relerr.max()) if relerr.numel() else 0.0, rel)
    bad = diff > tol
    if bool(bad.any()):
        i = ks._where(torch.where(bad, diff / (tol + 1e-30), torch.zeros_like(diff)).argmax(), got.shape)
        a, z = int(lo[i[:-1]]), int(hi[i[:-1]])
        res.ok = res.o_ok = False
        res.msg = (f"{ks._name_row(i[:-1])} column {i[-1]}: got {float(got[i]):.6g} = "
                   f"{float(got[i]) * max(z - a, 1):.3f} of the {z - a} keys [{a}, {z}), wanted "
                   f"{int(counts[z, i[-1]] - counts[a, i[-1]])} ({int(bad.sum())} elements past the gate)")
    if lse is not None:
        res.lse_gate = census_lse_gate(score)
        ok, res.lse_err, msg = ks._check_lse(lse, lse_want, res.lse_gate)
        if not ok:
            res.ok = res.lse_ok = False
            res.msg = (res.msg + "; " if res.msg else "") + msg
    return res


def census_qkv(q_shape, kv_shape, qval, kval, layout, dtype, device="cpu"):
    """keysense_inputs.census_qkv with separate levels for Q and K (so the
    common score can be negative)."""
    q, k, v, counts = ks.census_qkv(q_shape, kv_shape, 0.0, layout, dtype, device)
    q.fill_(qval)
    k.fill_(kval)
    return q, k, v, counts


# ---- references ---------------------------------------------------------------------

def ref_torch(q, k, v, lens, window, q_lens=None):
    """fp32 torch reference on the tensors' device, the window as a mask:
    (O [B,Hq,Sq,D], LSE [B,Hq,Sq]); rows past each length are never touched,
    rows t >= n_b give zeros / -inf."""
    b, hq, sq, d = q.shape
    hkv, cap = k.shape[1], k.shape[2]
    g = hq // hkv
    dev = q.device
    lens = torch.as_tensor(lens, device=dev).long().clamp(0, cap)
    n = torch.full((b,), sq, device=dev) if q_lens is None else torch.as_tensor(q_lens, device=dev).long().clamp(0, sq)
    key = torch.arange(cap, device=dev)
    live = key[None, :] < lens[:, None]
    kf = torch.where(live[:, None, :, None], k.float(), 0.0).repeat_interleave(g, 1)
    vf = torch.where(live[:, None, :, None], v.float(), 0.0).repeat_interleave(g, 1)
    s = q.float() @ kf.transpose(-1, -2) / math.sqrt(d)
    t = torch.arange(sq, device=dev)[None, :]
    pos = (lens - n)[:, None] + t                                           # [B, Sq]
    vis = (key[None, None, :] <= pos[:, :, None]) & live[:, None, :] & (t < n[:, None])[:, :, None]
    if window > 0:
        vis &= key[None, None, :] > (pos - window)[:, :, None]
    s = s.masked_fill(~vis[:, None], float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.nan_to_num(torch.exp(s - lse[..., None]), nan=0.0)
    return p @ vf, lse


def oracle_rows(q, k, v, kv_lens, q_lens, window):
    """CPU-oracle O as uint16 fp16 bits [B,Hq,Sq,D] from uint16 inputs: each row
    through oracle.attention_rows on its own keys K[lo:hi], the query at their
    last position (which, causal, sees all of them).  Rows that see no key and
    rows t >= n_b are zeros."""
    b, hq, sq, d = q.shape
    cap = k.shape[2]
    g = hq // k.shape[1]
    lo, hi = interval(kv_lens, q_lens, b, sq, cap, window)
    out = np.zeros((b, hq, sq, d), np.uint16)
    for bi in range(b):
        for t in range(sq):
            a, z = int(lo[bi, t]), int(hi[bi, t])
            if z <= a:
                continue
            qf = np.zeros((z - a, d), np.uint16)
            for h in range(hq):
                qf[-1] = q[bi, h, t]
                out[bi, h, t] = oracle.attention_rows(qf, k[bi, h // g, a:z], v[bi, h // g, a:z],
                                                      np.array([z - a - 1]), True, threads=1)[0]
    return out


def lse_f64(q, k, kv_lens, q_lens, window):
    """float64 (LSE [B,Hq,Sq], max |scaled score| of a visible key); q, k: uint16
    fp16 bits or 16-bit torch tensors.  Rows t >= n_b and unseen rows: -inf."""
    if isinstance(q, torch.Tensor):
        qf, kf = (x.detach().float().cpu().numpy().astype(np.float64) for x in (q, k))
    else:
        qf, kf = (a.view(np.float16).astype(np.float64) for a in (q, k))
    b, hq, sq, d = qf.shape
    g = hq // kf.shape[1]
    lo, hi = interval(kv_lens, q_lens, b, sq, kf.shape[2], window)
    s = qf @ np.swapaxes(np.repeat(kf, g, axis=1), -1, -2) / math.sqrt(d)
    j = np.arange(kf.shape[2])[None, None, :]
    vis = (j >= lo[:, :, None]) & (j < hi[:, :, None])                      # [B, Sq, cap]
    vis = np.broadcast_to(vis[:, None], s.shape)
    smax = float(np.abs(s[vis]).max()) if vis.any() else 0.0
    s = np.where(vis, s, -np.inf)
    m = s.max(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        lse = np.where(np.isneginf(m), -np.inf,
                       m + np.log(np.exp(s - np.where(np.isneginf(m), 0.0, m)[..., None]).sum(-1)))
    return lse, smax


def refs(host, dev, kv_lens, q_lens, window, dtype):
    """(O reference, float64 LSE, max |scaled score|) as prefill_refs.refs: fp16
    from the CPU oracle where the host bits are given, else fp32 torch."""
    if dtype is torch.float16 and host is not None:
        ro = oracle_rows(*host, kv_lens, q_lens, window)
        lref, smax = lse_f64(host[0], host[1], kv_lens, q_lens, window)
    else:
        ro = ref_torch(*dev, kv_lens, window, q_lens)[0]
        lref, smax = lse_f64(dev[0], dev[1], kv_lens, q_lens, window)
    return ro, lref, smax
