"""MLA prefill (fa_mi355x.flash_attention_mla_prefill_varlen / _bshd) on the
GPU against a plain float64 restatement of include/fa_mi355x_mla_prefill.h's
contract on the same rounded 16-bit inputs: one ragged batch whose lengths sit
on both sides of the 64-key tile and the 128-row block, rows past the last
sequence, NaN wherever the kernel must not read and a sentinel wherever it must
not write."""
import functools
import math

import numpy as np
import pytest
import torch

import decode_refs as dr
import fa_mi355x as fa

gpu = pytest.mark.gpu
DEV = dr.DEV
DQK, DV, PAD = 192, 128, 3
NQ = (1, 64, 65, 0, 129, 200)
NK_CROSS = tuple(n + d for n, d in zip(NQ, (0, 70, 0, 5, -9, 64)))
UNIFORM = (2, 65, 130)  # B, Sq, Sk
MODES = ("cross", "self", "uniform")
HEADS = ((2, 2), (4, 2), (3, 1))
SCALES = (1 / math.sqrt(192), 0.1147)
GATES = {torch.float16: dr.GATE_F16, torch.bfloat16: dr.GATE_BF16}
SENTINEL = -7.0


def lengths(mode):
    """(nq, nk, T_q, T_k) of a mode; the ragged totals exceed the last cu entry by PAD rows."""
    if mode == "uniform":
        b, sq, sk = UNIFORM
        return (sq,) * b, (sk,) * b, b * sq, b * sk
    nk = NK_CROSS if mode == "cross" else NQ
    return NQ, nk, sum(NQ) + PAD, sum(nk) + PAD


def scale_of(hq, mode, causal):
    return SCALES[(hq + MODES.index(mode) + causal) & 1]


def f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def host_inputs(dtype, hq, hkv, mode):
    """Seeded 16-bit (q, k, v) of magnitude <= 1 on the CPU (read-only)."""
    _, _, tq, tk = lengths(mode)
    gen = torch.Generator().manual_seed(100 * hq + 10 * hkv + MODES.index(mode))
    return tuple((torch.rand(s, generator=gen) * 2 - 1).to(dtype) for s in ((tq, hq, DQK), (tk, hkv, DQK), (tk, hkv, DV)))


@functools.lru_cache(maxsize=None)
def ramp_inputs(dtype):
    """One sequence of 200 rows and keys, two heads: q = a fixed +-1 pattern u,
    k_j = u (j + 1) / 200, so the scores rise to 192 * scale across the keys and
    every key tile raises the running maximum."""
    n, h = 200, 2
    gen = torch.Generator().manual_seed(7)
    u = (torch.rand(DQK, generator=gen) < 0.5).float() * 2 - 1
    q = u.expand(n, h, DQK).to(dtype).contiguous()
    k = (u[None, None, :] * ((torch.arange(n) + 1.0) / n)[:, None, None]).expand(n, h, DQK).to(dtype).contiguous()
    v = (torch.rand((n, h, DV), generator=gen) * 2 - 1).to(dtype)
    return q, k, v


def contract_f64(q, k, v, nq, nk, causal, scale):
    """(O [T_q,Hq,128], LSE [Hq,T_q], max |s|, rows of a sequence [T_q]) of the header's contract in float64."""
    tq, hq, hkv = q.shape[0], q.shape[1], k.shape[1]
    o, lse, smax, live = np.zeros((tq, hq, DV)), np.full((hq, tq), -np.inf), 0.0, np.zeros(tq, bool)
    sq = sk = 0
    for a, n in zip(nq, nk):
        live[sq:sq + a] = True
        for h in range(hq):
            hk = h // (hq // hkv)
            for i in range(a):
                vis = min(n, n - a + i + 1) if causal else n
                if vis <= 0:
                    continue
                s = scale * k[sk:sk + vis, hk] @ q[sq + i, h]
                smax = max(smax, float(np.abs(s).max()))
                p = np.exp(s - s.max())
                o[sq + i, h] = p @ v[sk:sk + vis, hk] / p.sum()
                lse[h, sq + i] = s.max() + np.log(p.sum())
        sq, sk = sq + a, sk + n
    return o, lse, smax, live


@functools.lru_cache(maxsize=None)
def reference(dtype, hq, hkv, mode, causal):
    nq, nk, _, _ = lengths(mode)
    return contract_f64(*map(f64, host_inputs(dtype, hq, hkv, mode)), nq, nk, causal, scale_of(hq, mode, causal))


@functools.lru_cache(maxsize=None)
def ramp_reference(dtype, causal):
    return contract_f64(*map(f64, ramp_inputs(dtype)), (200,), (200,), causal, SCALES[0])


def cu_of(n):
    return torch.tensor(np.concatenate([[0], np.cumsum(n)]), dtype=torch.int32, device=DEV)


def device_inputs(q, k, v, nk, strided):
    """q, k, v on the device with NaN in the K/V rows of no sequence; strided: q
    rows 64 and k rows 8 elements of NaN apart and v the second half of a per-token
    [k_nope (Hkv * 128) | v (Hkv * 128)] buffer whose first half is NaN."""
    q, k, v = q.to(DEV), k.to(DEV).clone(), v.to(DEV).clone()
    dr.nan_fill(k[sum(nk):])
    dr.nan_fill(v[sum(nk):])
    if strided:
        tq, hq, tk, hkv = q.shape[0], q.shape[1], v.shape[0], v.shape[1]
        qb = dr.nan_fill(torch.empty((tq, hq * DQK + 64), dtype=q.dtype, device=DEV))
        qb[:, :hq * DQK] = q.reshape(tq, -1)
        q = qb[:, :hq * DQK].unflatten(1, (hq, DQK))
        kb = dr.nan_fill(torch.empty((tk, hkv * DQK + 8), dtype=k.dtype, device=DEV))
        kb[:, :hkv * DQK] = k.reshape(tk, -1)
        k = kb[:, :hkv * DQK].unflatten(1, (hkv, DQK))
        kv = dr.nan_fill(torch.empty((tk, 2 * hkv * DV), dtype=v.dtype, device=DEV))
        kv[:, hkv * DV:] = v.reshape(tk, -1)
        v = kv[:, hkv * DV:].unflatten(1, (hkv, DV))
        assert not q.is_contiguous() and not v.is_contiguous()
    return q, k, v


def run(q, k, v, mode, nq, nk, **kw):
    out = torch.full((*q.shape[:-1], DV), SENTINEL, dtype=q.dtype, device=DEV)
    if mode == "uniform":
        kw.update(seqlen_q=nq[0], seqlen_k=nk[0])
    else:
        kw.update(cu_seqlens_q=cu_of(nq), cu_seqlens_k=cu_of(nk) if mode == "cross" else None)
    return fa.flash_attention_mla_prefill_varlen(q, k, v, out=out, return_lse=True, **kw)


def check(o, lse, ref, dtype, what):
    ro, rl, smax, live = ref
    o, live_t = o.cpu(), torch.from_numpy(live)
    assert bool(torch.isfinite(o[live_t]).all()), what
    assert bool((o[~live_t] == SENTINEL).all()), what  # rows of no sequence are not written
    err = float(np.abs(f64(o)[live] - ro[live]).max())
    print(f"{what}: max_abs_diff {err:.3e}")
    assert err <= GATES[dtype], (what, err)
    dr.check_lse(lse[:, live_t.to(DEV)], rl[:, live], smax, what)
    assert int(torch.count_nonzero(o[live_t][torch.from_numpy(np.isneginf(rl[:, live].T))])) == 0, what


def test_rounding_alone_does_not_pass_the_gate():
    """No GPU: the float64 reference rounded to each output type sits within half
    of each gate on this file's inputs (|O| <= max |v| <= 1), the ramp included,
    so a gate is not met by rounding alone."""
    for dtype, gate in GATES.items():
        refs = [reference(dtype, hq, hkv, mode, causal) for hq, hkv in HEADS for mode in MODES
                for causal in (False, True)] + [ramp_reference(dtype, causal) for causal in (False, True)]
        for ro, _, _, live in refs:
            assert live.any() and np.abs(f64(torch.from_numpy(ro).to(dtype)) - ro).max() <= gate / 2


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("heads", HEADS, ids=lambda h: "h%dk%d" % h)
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_contract(dtype, causal, heads, strided, mode):
    hq, hkv = heads
    nq, nk, _, _ = lengths(mode)
    q, k, v = device_inputs(*host_inputs(dtype, hq, hkv, mode), nk, strided)
    o, lse = run(q, k, v, mode, nq, nk, softmax_scale=scale_of(hq, mode, causal), causal=causal)
    assert o.shape == (q.shape[0], hq, DV) and o.dtype == dtype
    check(o, lse, reference(dtype, hq, hkv, mode, causal), dtype,
          f"{dr.name(dtype)} causal{causal} h{hq}k{hkv} strided{strided} {mode}")


@gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_ramp(dtype, causal):
    q, k, v = device_inputs(*ramp_inputs(dtype), (200,), False)
    o, lse = run(q, k, v, "self", (200,), (200,), softmax_scale=SCALES[0], causal=causal)
    check(o, lse, ramp_reference(dtype, causal), dtype, f"ramp {dr.name(dtype)} causal{causal}")


@gpu
def test_graph_replay_follows_cu_seqlens():
    hq, hkv = 4, 2
    q, k, v = device_inputs(*host_inputs(torch.float16, hq, hkv, "cross"), NK_CROSS, True)
    cu_q, cu_k = cu_of(NQ), cu_of(NK_CROSS)
    kw = dict(softmax_scale=SCALES[1], causal=True, return_lse=True)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fa.flash_attention_mla_prefill_varlen(q, k, v, cu_q, cu_k, **kw)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            res = fa.flash_attention_mla_prefill_varlen(q, k, v, cu_q, cu_k, **kw)
    torch.cuda.current_stream().wait_stream(stream)
    for nq, nk in (((200, 129, 0, 65, 64, 1), (264, 120, 5, 65, 134, 1)), (NQ, NK_CROSS), ((130, 0, 0, 0, 0, 300), NK_CROSS)):
        cu_q.copy_(cu_of(nq))
        cu_k.copy_(cu_of(nk))
        for _ in range(2):
            res[0].fill_(SENTINEL)
            graph.replay()
            torch.cuda.synchronize()
            out = torch.full_like(res[0], SENTINEL)
            o, lse = fa.flash_attention_mla_prefill_varlen(q, k, v, cu_of(nq), cu_of(nk), out=out, **kw)
            # (the LSE of rows of no sequence is not written: whatever the two buffers held)
            assert torch.equal(res[0], o) and torch.equal(res[1][:, :sum(nq)], lse[:, :sum(nq)]), nq


@gpu
def test_torch_ops_and_uniform_equal_the_ragged_call():
    import fa_mi355x.torch_op_mla_prefill as tomp

    hq, hkv = 4, 2
    (b, sq, sk), scale = UNIFORM, SCALES[0]
    q, k, v = device_inputs(*host_inputs(torch.bfloat16, hq, hkv, "uniform"), (sk,) * b, True)
    cu_q, cu_k = cu_of((sq,) * b), cu_of((sk,) * b)
    want = fa.flash_attention_mla_prefill_varlen(q, k, v, cu_q, cu_k, softmax_scale=scale, return_lse=True)
    assert torch.equal(tomp.prefill_varlen(q, k, v, scale, cu_q, cu_k), want[0])
    # uniform: on the token-major tensors and as [B, S, H, D], row for row the ragged call
    assert dr.same(fa.flash_attention_mla_prefill_varlen(q, k, v, softmax_scale=scale, seqlen_q=sq, seqlen_k=sk,
                                                         return_lse=True), want)
    q4, k4, v4 = (t.unflatten(0, (b, -1)) for t in (q, k, v))
    o4, lse4 = fa.flash_attention_mla_prefill_bshd(q4, k4, v4, softmax_scale=scale, return_lse=True)
    assert torch.equal(o4.flatten(0, 1), want[0]) and torch.equal(lse4.permute(1, 0, 2).flatten(1), want[1])
    assert torch.equal(tomp.prefill_bshd(q4, k4, v4, scale), o4)
