"""What two or more decode test files share: inputs, references, gates and the
page-pool builders.  Imported, never executed by path; one copy per session.

References and gates:
  * fp16 output: the CPU oracle (oracle.attention_rows) per query head, with
    its K/V head's rows [0, len_b); the Sq query rows sit at positions
    len_b - Sq .. len_b - 1 of an otherwise-zero [len_b, D] q.  Gate 1e-3 (the
    project's).
  * bf16 output: fp32 torch on the tensors' device, gate 5e-3 (the project's).
  * LSE: float64 numpy log-sum-exp of the same 16-bit inputs, gate
    2^-10 * max|scaled score| + 1e-5 with the maximum taken from the
    reference: LSE is 1-Lipschitz in the scores, and the only score error
    above fp32 noise the design allows is a 16-bit rounding of the pre-scaled
    Q (2^-11 relative); the gate is twice that.
tests/test_decode_refs_cpu.py holds the three references against one another
on the CPU.
"""
import math

import numpy as np
import pytest
import torch

import fa_mi355x
import oracle

DEV = "cuda"
GATE_F16 = 1e-3
GATE_BF16 = 5e-3
NAN_BITS = 0x7fff  # a NaN in fp16 and in bf16

DTYPES = [pytest.param(torch.float16, id="fp16"), pytest.param(torch.bfloat16, id="bf16")]


def nb(g, sq):
    return 1 if g * sq <= 16 else (2 if g * sq <= 32 else 4)


def name(dtype):
    return "fp16" if dtype is torch.float16 else "bf16"


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.uint16).view(np.int16)).view(torch.float16).to(DEV)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def lens(vals):
    return torch.tensor(list(vals), dtype=torch.int32, device=DEV)


_INPUTS = {}


def inputs(b, hq, hkv, sq, cap, d, seed=42):
    """(q, k, v) uint16 fp16 bits from the oracle's generator (cached, read-only)."""
    key = (b, hq, hkv, sq, cap, d, seed)
    if key not in _INPUTS:
        _, k, v = oracle.gen_inputs(b, hkv, cap, d, seed)
        q = oracle.gen_inputs(b, hq, sq, d, seed + 1)[0]
        for a in (q, k, v):
            a.setflags(write=False)
        _INPUTS[key] = (q, k, v)
    return _INPUTS[key]


def oracle_decode(q, k, v, lens, causal):
    """CPU-oracle decode reference: uint16 [B, Hq, Sq, D]; rows that see no key are zeros."""
    b, hq, sq, d = q.shape
    g = hq // k.shape[1]
    out = np.zeros((b, hq, sq, d), np.uint16)
    for bi in range(b):
        n = int(lens[bi])
        if n == 0:
            continue
        for h in range(hq):
            kh, vh = k[bi, h // g, :n], v[bi, h // g, :n]
            if n >= sq:
                qf = np.zeros((n, d), np.uint16)
                qf[n - sq:] = q[bi, h]
                out[bi, h] = oracle.attention_rows(qf, kh, vh, np.arange(n - sq, n), causal)
                continue
            for t in range(sq):
                pos = n - sq + t if causal else 0
                if pos < 0:
                    continue
                qf = np.zeros((n, d), np.uint16)
                qf[pos] = q[bi, h, t]
                out[bi, h, t] = oracle.attention_rows(qf, kh, vh, np.array([pos]), causal)[0]
    return out


def lse_ref(q, k, v, lens, causal):
    """float64 LSE [B, Hq, Sq] of the 16-bit inputs and the largest |scaled score|
    (q, k: uint16 fp16 bits, or 16-bit torch tensors of either dtype)."""
    if isinstance(q, torch.Tensor):
        qf, kall = (t.detach().float().cpu().numpy().astype(np.float64) for t in (q, k))
    else:
        qf, kall = (a.view(np.float16).astype(np.float64) for a in (q, k))
    b, hq, sq, d = qf.shape
    g = hq // kall.shape[1]
    lse = np.full((b, hq, sq), -np.inf)
    smax = 0.0
    for bi in range(b):
        n = int(lens[bi])
        if n == 0:
            continue
        for h in range(hq):
            kf = kall[bi, h // g, :n]
            s = qf[bi, h] @ kf.T / math.sqrt(d)
            for t in range(sq):
                vis = min(n, n - sq + t + 1) if causal else n
                if vis <= 0:
                    continue
                row = s[t, :vis]
                smax = max(smax, float(np.abs(row).max()))
                mx = row.max()
                lse[bi, h, t] = mx + np.log(np.exp(row - mx).sum())
    return lse, smax


def check_lse(lse, ref, smax, what):
    got = lse.detach().cpu().numpy().astype(np.float64)
    empty = np.isneginf(ref)
    assert np.array_equal(np.isneginf(got), empty), what
    gate = 2.0 ** -10 * smax + 1e-5
    err = float(np.abs(got[~empty] - ref[~empty]).max()) if (~empty).any() else 0.0
    print(f"{what}: lse err {err:.3e} gate {gate:.3e}")
    assert err <= gate, (what, err, gate)


def check_f16(out, ref, what, gate=GATE_F16):
    d = oracle.max_abs_diff(bits(out), ref)
    print(f"{what}: max_abs_diff {d:.3e}")
    assert d <= gate, (what, d)


def ref_torch(q, k, v, lens, causal):
    """fp32 torch reference on the tensors' device: (O [B,Hq,Sq,D], LSE [B,Hq,Sq]);
    rows past each length are never touched (they may hold NaN)."""
    b, hq, sq, d = q.shape
    hkv, cap = k.shape[1], k.shape[2]
    g = hq // hkv
    key = torch.arange(cap, device=q.device)
    live = key[None, :] < lens[:, None].to(q.device)                      # [B, cap]
    kf = torch.where(live[:, None, :, None], k.float(), 0.0).repeat_interleave(g, 1)
    vf = torch.where(live[:, None, :, None], v.float(), 0.0).repeat_interleave(g, 1)
    s = q.float() @ kf.transpose(-1, -2) / math.sqrt(d)                   # [B, Hq, Sq, cap]
    lim = lens[:, None].to(q.device).expand(b, sq)
    if causal:
        lim = lim - sq + 1 + torch.arange(sq, device=q.device)[None, :]
    vis = key[None, None, :] < lim[:, :, None]                            # [B, Sq, cap]
    s = s.masked_fill(~vis[:, None], float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.nan_to_num(torch.exp(s - lse[..., None]), nan=0.0)
    return p @ vf, lse


def ws_counters_zero():
    dev = torch.cuda.current_device()
    st = torch.cuda.current_stream().cuda_stream
    buf = fa_mi355x._WS_BUF.get((dev, st))
    assert buf is not None, "the split launch took no workspace"
    torch.cuda.synchronize()
    return int(torch.count_nonzero(buf[:65536]).item()) == 0


def refs(host, dev, kv_lens, causal, dtype):
    """(O reference, float64 LSE, max |scaled score|): fp16 from the CPU oracle
    where the host bits are given, else (bf16, or an fp32 cache) from fp32 torch
    on the device tensors."""
    if dtype is torch.float16 and host is not None:
        ro = oracle_decode(*host, kv_lens, causal)
        lref, smax = lse_ref(host[0], host[1], host[2], kv_lens, causal)
    else:
        ro = ref_torch(*dev, lens(kv_lens), causal)[0]
        lref, smax = lse_ref(dev[0], dev[1], dev[2], kv_lens, causal)
    return ro, lref, smax


def check(out, lse, refs, dtype, what):
    ro, lref, smax = refs
    assert bool(torch.isfinite(out).all()), what
    if isinstance(ro, np.ndarray):
        check_f16(out, ro, what)
    else:
        gate = GATE_F16 if dtype is torch.float16 else GATE_BF16
        err = float((out.float() - ro).abs().max())
        print(f"{what}: max_abs_diff {err:.3e}")
        assert err <= gate, (what, err)
    check_lse(lse, lref, smax, what)
    unseen = torch.from_numpy(np.isneginf(lref)).to(out.device)
    assert int(torch.count_nonzero(out[unseen]).item()) == 0, what


# ---- page pools -----------------------------------------------------------------

def nan_fill(t):
    t.view(torch.int16).fill_(NAN_BITS)
    return t


def paginate(k, v, page_size, lens, seed=0, spare=5, filler=0):
    """(k_pages, v_pages, table) from contiguous [B][Hkv][cap][D] caches (on any
    device) with cap % page_size == 0.  Element b's pages that hold a key below
    lens[b] go to pool pages drawn from a seeded permutation of
    range(num_pages), the elements' pages interleaved; num_pages = used +
    spare.  Everything else in the pool is NaN, the rows past each length in
    the last used page included.  Table entries past the used ones are
    `filler` (an int, or "junk" for arbitrary ids, out-of-pool ones among
    them)."""
    b, hkv, cap, d = k.shape
    assert cap % page_size == 0
    mpp = cap // page_size
    used = [-(-int(n) // page_size) for n in lens]
    slots = sorted((j, bi) for bi in range(b) for j in range(used[bi]))  # interleaved
    num_pages = len(slots) + spare
    perm = np.random.default_rng(seed).permutation(num_pages)
    kp = nan_fill(torch.empty((num_pages, hkv, page_size, d), dtype=k.dtype, device=k.device))
    vp = nan_fill(torch.empty_like(kp))
    if filler == "junk":
        table = np.random.default_rng(seed + 1).integers(-3, num_pages + 3, size=(b, mpp))
        table[:, -1:] = np.array([2 ** 31 - 1])[None, :]
    else:
        table = np.full((b, mpp), filler, dtype=np.int64)
    for i, (j, bi) in enumerate(slots):
        pg = int(perm[i])
        table[bi, j] = pg
        live = min(page_size, int(lens[bi]) - j * page_size)
        kp[pg, :, :live] = k[bi, :, j * page_size:j * page_size + live]
        vp[pg, :, :live] = v[bi, :, j * page_size:j * page_size + live]
    return kp, vp, torch.tensor(table, dtype=torch.int32, device=k.device)


def gather(pages, table):
    """The contiguous [B][Hkv][max_pages * page_size][D] cache the table describes
    (entries outside the pool read page 0: they lie past every length)."""
    n, hkv, ps, d = pages.shape
    t = table.long()
    t = torch.where((t >= 0) & (t < n), t, torch.zeros_like(t))
    return pages[t].permute(0, 2, 1, 3, 4).reshape(table.shape[0], hkv, table.shape[1] * ps, d).contiguous()


def rand(shape, dtype, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.rand(shape, generator=gen, device=DEV, dtype=torch.float32) * 2 - 1).to(dtype)


def same(a, b):
    """Bit-equal outputs and LSEs (LSE -inf == -inf; no NaN is expected in either)."""
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
