"""GPU tests of the backward pass of the token-major attention
(fa_attn_varlen_bwd_*, flash_attention_varlen_backward / _bshd_backward, the
torch ops and flash_attn_varlen_func / flash_attn_func).  References and the
derived gate: attn_bwd_refs.  The forward's out and lse always come from the
forward under test's sibling, flash_attention_varlen / flash_attention_bshd.

Measured max|g - g_ref| / max|g_16 - g_ref| on the base sweep (the gate allows
2 + one output rounding): see DESIGN.md §3.0q.
"""
import functools

import pytest
import torch

import attn_bwd_refs as br
import attn_varlen_refs as ar
import decode_refs as dr
import fa_mi355x
import varlen_refs as vr

pytestmark = pytest.mark.gpu

DEV = dr.DEV
F16, BF16 = br.F16, br.BF16
SENTINEL = 0x1234  # a finite 16-bit pattern the gradients are pre-filled with
fwd = fa_mi355x.flash_attention_varlen
bwd = fa_mi355x.flash_attention_varlen_backward


def lens(x):
    return torch.tensor([int(v) for v in x], dtype=torch.int32, device=DEV)


def bits(t):
    return t.view(torch.int16)


def same(a, b, own=None):
    """(dq, dk, dv) agree bit for bit (own: on those rows only)."""
    if own is None:
        own = (slice(None),) * 3
    return all(torch.equal(bits(x)[o], bits(y)[o]) for x, y, o in zip(a, b, own))


def sentinel_like(t):
    out = torch.empty(t.shape, dtype=t.dtype, device=DEV)
    bits(out).fill_(SENTINEL)
    return out


def forward(qp, kp, vp, cu_q, cu_k, causal, own_q=None):
    """The forward's (out, lse); with own_q, NaN in every row of no sequence of both."""
    out, lse = fwd(qp, kp, vp, cu_q, cu_k, causal=causal, return_lse=True)
    if own_q is not None:
        bits(out)[~own_q] = dr.NAN_BITS
        lse[:, ~own_q] = float("nan")
    return out, lse


def run(inputs, cus, causal, nan_rows=True, cu_k_none=False, **kw):
    """Forward + backward of packed CPU (or device) inputs; the gradients are
    pre-filled with the sentinel.  Returns (dq, dk, dv) on the device."""
    qp, kp, vp, dop = (t.to(DEV) for t in inputs)
    cu_q, cu_k = lens(cus[0]), (None if cu_k_none else lens(cus[1]))
    own_q = torch.from_numpy(vr.owned_rows(cus[0], qp.shape[0])).to(DEV) if nan_rows else None
    out, lse = forward(qp, kp, vp, cu_q, cu_k, causal, own_q)
    g = bwd(dop, qp, kp, vp, out, lse, cu_q, cu_k, causal=causal, dq=sentinel_like(qp), dk=sentinel_like(kp),
            dv=sentinel_like(vp), **kw)
    torch.cuda.synchronize()
    return g


@functools.lru_cache(maxsize=None)
def base_run(d, dtype, causal):
    """The base shape's gradients, computed once and shared (read-only)."""
    return run(*br.base_inputs(d, dtype), causal)


def owned_dev():
    return tuple(m.to(DEV) for m in br.owned_masks())


# ---- 1. the base sweep ---------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("d", [128, 64])
def test_base_sweep(d, dtype, causal):
    """B = 5 ragged, GQA 4: an empty query sequence with keys, 27 rows that see
    nothing under causal, 3 query blocks x 9 key tiles, starts on and off the
    64 / 128 boundaries.  NaN bits sit in every row of no sequence of every input."""
    got = base_run(d, dtype, causal)
    gref, g16 = br.base_refs(d, dtype, causal)
    br.check_gate(got, gref, g16, dtype, f"base d{d} {dr.name(dtype)} causal={causal}", owned=br.owned_masks())
    dq, dk, dv = got
    # sequence 0 has keys and no query: its dk / dv rows are written zeros
    s, n = vr.spans(ar.CU_K, ar.TK)[0]
    assert n == 7 and int(torch.count_nonzero(dk[s:s + n])) == 0 and int(torch.count_nonzero(dv[s:s + n])) == 0
    if causal:
        # sequence 2: off = -27, its 27 leading rows see nothing: dq exact zeros
        s = ar.CU_Q[2]
        assert int(torch.count_nonzero(dq[s:s + 27])) == 0
        # the row after them sees one key (P = 1, dS = dP - delta = 0); the next one two
        assert int(torch.count_nonzero(dq[s + 28])) > 0


# ---- 2. sentinels ----------------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_sentinels(causal):
    """NaN bits in every row of no sequence of q, k, v, dout, out and lse (run()
    puts them there); the gradients pre-filled with a pattern: rows of no
    sequence keep it, owned rows are finite."""
    got = base_run(128, BF16, causal)
    for name, g, own in zip(("dq", "dk", "dv"), got, owned_dev()):
        assert bool((bits(g)[~own] == SENTINEL).all()), name
        assert bool(torch.isfinite(g[own]).all()), name
    assert int((~owned_dev()[0]).sum()) == 23 and int((~owned_dev()[1]).sum()) == 73


# ---- 3. a sequence without keys ---------------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_sequence_without_keys(causal):
    nk = (7, 201, 100, 0, 521)
    inputs, cus = br.base_inputs(128, F16, nk=nk)
    got = run(inputs, cus, causal)
    s = cus[0][3]
    assert ar.NQ[3] == 128 and int(torch.count_nonzero(got[0][s:s + 128])) == 0
    gref, g16 = br.base_refs(128, F16, causal, nk=nk)
    own = tuple(torch.from_numpy(vr.owned_rows(c, t)) for c, t in ((cus[0], ar.TQ), (cus[1], ar.TK), (cus[1], ar.TK)))
    br.check_gate(got, gref, g16, F16, f"no-key sequence causal={causal}", owned=own)


# ---- 4. self-attention ------------------------------------------------------------------------------

def _self_inputs(d, dtype, hq=ar.HQ, hkv=ar.HKV):
    g = torch.Generator().manual_seed(3)
    q = torch.randn((ar.TQ, hq, d), generator=g).to(dtype)
    k = torch.randn((ar.TQ, hkv, d), generator=g).to(dtype)
    v = torch.randn((ar.TQ, hkv, d), generator=g).to(dtype)
    return q, k, v, br.make_dout(q.shape, dtype)


def test_self_attention_is_cu_q_twice():
    inputs = _self_inputs(64, F16)
    a = run(inputs, (ar.CU_Q, ar.CU_Q), True, cu_k_none=True)
    b = run(inputs, (ar.CU_Q, ar.CU_Q), True)
    assert same(a, b)
    assert bool(torch.isfinite(a[0][: ar.CU_Q[-1]]).all()) and int(torch.count_nonzero(a[1])) > 0


# ---- 5. the uniform mode ------------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("hq,hkv,d,dtype", [(4, 1, 128, F16), (2, 2, 64, BF16)], ids=["mqa", "mha"])
def test_bshd_is_packed_on_arange(hq, hkv, d, dtype, causal):
    b, sq, sk = 3, 130, 200
    g = torch.Generator().manual_seed(5)
    q = torch.randn((b, sq, hq, d), generator=g).to(dtype)
    k = torch.randn((b, sk, hkv, d), generator=g).to(dtype)
    v = torch.randn((b, sk, hkv, d), generator=g).to(dtype)
    do = br.make_dout(q.shape, dtype)
    qd, kd, vd, dod = (t.to(DEV) for t in (q, k, v, do))
    out, lse = fa_mi355x.flash_attention_bshd(qd, kd, vd, causal=causal, return_lse=True)
    assert lse.shape == (b, hq, sq) and lse.stride() == (sq, b * sq, 1)
    got = fa_mi355x.flash_attention_bshd_backward(dod, qd, kd, vd, out, lse, causal=causal)
    cu_q, cu_k = [i * sq for i in range(b + 1)], [i * sk for i in range(b + 1)]
    flat = tuple(t.flatten(0, 1) for t in (q, k, v, do))
    packed = run(flat, (cu_q, cu_k), causal, nan_rows=False)
    torch.cuda.synchronize()
    assert same(tuple(t.flatten(0, 1) for t in got), packed)
    gref = br.reference(*flat, cu_q, cu_k, causal, False)
    g16 = br.reference(*flat, cu_q, cu_k, causal, True)
    br.check_gate(packed, gref, g16, dtype, f"bshd hq{hq} hkv{hkv} causal={causal}")
    with pytest.raises(fa_mi355x.FlashAttentionError, match="view of a"):
        fa_mi355x.flash_attention_bshd_backward(dod, qd, kd, vd, out, lse.contiguous(), causal=causal)


# ---- 6. fused-buffer strides ---------------------------------------------------------------------------

def test_fused_buffer_strides():
    """q, k, v as the slices of one [T, Hq + 2 Hkv, D] buffer and dout as a
    slice of a wider one: the dense call's bits."""
    d, dtype, causal = 128, BF16, True
    (qp, kp, vp, dop), cus = br.base_inputs(d, dtype)
    q, k, v = ar.fused_qkv(qp.to(DEV), kp.to(DEV), vp.to(DEV))
    wide = dr.nan_fill(torch.empty((ar.TQ, 2 * ar.HQ + 1, d), dtype=dtype, device=DEV))
    do = wide[:, 1:1 + ar.HQ]
    do.copy_(dop)
    assert q.stride(0) == (ar.HQ + 2 * ar.HKV) * d and do.stride(0) == (2 * ar.HQ + 1) * d
    got = run((q, k, v, do), cus, causal)
    assert same(got, base_run(d, dtype, causal))


# ---- 7. reproducibility ----------------------------------------------------------------------------------

def test_reproducible_and_raw_stream():
    d, dtype, causal = 64, BF16, True
    inputs, cus = br.base_inputs(d, dtype)
    want = base_run(d, dtype, causal)
    assert same(run(inputs, cus, causal), want)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = run(inputs, cus, causal, stream=s.cuda_stream)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert same(got, want)


# ---- 8. census -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_census(dtype, causal):
    """Q = 0 makes P uniform over the visible keys, so dK is exactly zero; with
    dO = 1 and V = 0, dV_j = sum over the rows that see j of 1 / n_i in every
    column (a lost, doubled or mis-masked query block changes the count), and
    dQ is exactly zero (dP = 0, delta = 0)."""
    (qp, kp, vp, dop), cus = br.base_inputs(128, dtype)
    oq, ok, _ = br.owned_masks()
    q, v, do = qp.clone(), vp.clone(), dop.clone()
    q[oq], v[ok], do[oq] = 0, 0, 1
    got = run((q, kp, v, do), cus, causal)
    oqd, okd, _ = owned_dev()
    assert int(torch.count_nonzero(got[0][oqd])) == 0
    assert int(torch.count_nonzero(got[1][okd])) == 0
    gref = br.reference(q, kp, v, do, *cus, causal, False)
    g16 = br.reference(q, kp, v, do, *cus, causal, True)
    # the count itself, beside autograd: sum over the rows that see key j of 1 / n_i
    for (sq, nq), (sk, nk) in zip(vr.spans(cus[0], ar.TQ), vr.spans(cus[1], ar.TK)):
        if nq and nk:
            vis = br.visible(nq, nk, causal).double()
            n = vis.sum(1, keepdim=True).clamp(min=1)
            want = (vis / n).sum(0) * (ar.HQ // ar.HKV)
            assert torch.allclose(gref[2][sk:sk + nk, 0, 0], want, rtol=1e-12, atol=1e-14)
    br.check_gate(got, gref, g16, dtype, f"census {dr.name(dtype)} causal={causal}", owned=br.owned_masks())


# ---- 9. peaked scores ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_peaked_scores(dtype):
    """q x 8: a near one-hot softmax and a large LSE, at the same gate."""
    inputs, cus = br.base_inputs(128, dtype, q_scale=8.0)
    got = run(inputs, cus, True)
    gref, g16 = br.base_refs(128, dtype, True, q_scale=8.0)
    br.check_gate(got, gref, g16, dtype, f"peaked {dr.name(dtype)}", owned=br.owned_masks())


# ---- 10. autograd ------------------------------------------------------------------------------------------

def test_autograd_varlen_func():
    d, dtype, causal = 128, F16, True
    (qp, kp, vp, dop), cus = br.base_inputs(d, dtype)
    want = base_run(d, dtype, causal)
    own = owned_dev()
    q, k, v = (t.to(DEV).requires_grad_() for t in (qp, kp, vp))
    cu_q, cu_k = lens(cus[0]), lens(cus[1])
    out = fa_mi355x.flash_attn_varlen_func(q, k, v, cu_q, cu_k, causal=causal)
    assert out.requires_grad
    got = torch.autograd.grad(out, (q, k, v), dop.to(DEV), retain_graph=True)
    assert same(got, want, own)
    # a dout produced by a transposing op fails the stride rule: made contiguous, the same bits
    w = dop.to(DEV).permute(1, 0, 2).contiguous()
    got = torch.autograd.grad(out.permute(1, 0, 2), (q, k, v), w)
    assert same(got, want, own)
    # the existing op stays forward-only
    with pytest.raises(RuntimeError, match="forward-only"):
        o = torch.ops.fa_mi355x.attn_varlen(q, k, v, cu_q, cu_k, causal)
        torch.autograd.grad(o.sum(), (q,))


def test_autograd_fused_qkv_leaf():
    """Gradients flow to one fused [T, Hq + 2 Hkv, D] leaf through its slices."""
    d, dtype = 64, BF16
    q0, k0, v0, do = (t.to(DEV) for t in _self_inputs(d, dtype))
    cu = lens(ar.CU_Q)
    qkv = torch.cat([q0, k0, v0], 1).requires_grad_()
    q, k, v = qkv[:, :ar.HQ], qkv[:, ar.HQ:ar.HQ + ar.HKV], qkv[:, ar.HQ + ar.HKV:]
    out = fa_mi355x.flash_attn_varlen_func(q, k, v, cu, causal=True)
    (g,) = torch.autograd.grad(out, (qkv,), do)
    o, lse = fwd(q0, k0, v0, cu, None, causal=True, return_lse=True)
    want = bwd(do, q0, k0, v0, o, lse, cu, None, causal=True)
    n = ar.CU_Q[-1]
    assert torch.equal(bits(g)[:n], bits(torch.cat(want, 1))[:n])


def test_autograd_flash_attn_func():
    b, sq, sk, hq, hkv, d = 2, 70, 130, 4, 2, 64
    g = torch.Generator().manual_seed(9)
    q = torch.randn((b, sq, hq, d), generator=g).to(BF16).to(DEV).requires_grad_()
    k = torch.randn((b, sk, hkv, d), generator=g).to(BF16).to(DEV).requires_grad_()
    v = torch.randn((b, sk, hkv, d), generator=g).to(BF16).to(DEV).requires_grad_()
    do = br.make_dout(q.shape, BF16).to(DEV)
    out = fa_mi355x.flash_attn_func(q, k, v, causal=True)
    got = torch.autograd.grad(out, (q, k, v), do)
    o, lse = fa_mi355x.flash_attention_bshd(q.detach(), k.detach(), v.detach(), causal=True, return_lse=True)
    assert torch.equal(bits(o), bits(out.detach()))
    want = fa_mi355x.flash_attention_bshd_backward(do, q.detach(), k.detach(), v.detach(), o, lse, causal=True)
    assert same(got, want)
    assert int(torch.count_nonzero(got[1])) > 0


# ---- 11. graph capture ---------------------------------------------------------------------------------------

def test_graph_capture_forward_and_backward():
    """Forward + backward in one captured graph, replayed twice: the eager bits."""
    d, dtype, causal = 128, F16, True
    (qp, kp, vp, dop), cus = br.base_inputs(d, dtype)
    qd, kd, vd, dod = (t.to(DEV) for t in (qp, kp, vp, dop))
    cu_q, cu_k = lens(cus[0]), lens(cus[1])
    want = base_run(d, dtype, causal)
    grads = [sentinel_like(t) for t in (qd, kd, vd)]
    out = torch.empty_like(qd)

    def step():
        o, lse = fwd(qd, kd, vd, cu_q, cu_k, causal=causal, out=out, return_lse=True)
        bwd(dod, qd, kd, vd, o, lse, cu_q, cu_k, causal=causal, dq=grads[0], dk=grads[1], dv=grads[2])

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    own = owned_dev()
    for _ in range(2):
        for g in grads:
            bits(g).fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert same(grads, want, own)
        assert all(bool((bits(g)[~o] == SENTINEL).all()) for g, o in zip(grads, own))


# ---- empty problems ----------------------------------------------------------------------------------------------

def test_no_keys_at_all_and_no_rows():
    """total_k == 0: dq = 0 for ALL rows; total_q == 0: dk = dv = 0 for all rows."""
    d = 64
    (qp, kp, vp, dop), cus = br.base_inputs(d, F16)
    qd, kd, vd, dod = (t.to(DEV) for t in (qp, kp, vp, dop))
    kv = torch.empty((0, ar.HKV, d), dtype=F16, device=DEV)
    zero_cu = lens([0] * (ar.B + 1))
    o, lse = fwd(qd, kv, kv, lens(cus[0]), zero_cu, return_lse=True)
    dq, dk, dv = bwd(dod, qd, kv, kv, o, lse, lens(cus[0]), zero_cu, dq=sentinel_like(qd))
    assert int(torch.count_nonzero(dq)) == 0 and dk.shape == (0, ar.HKV, d)
    o, lse = fwd(qd[:0], kd, vd, zero_cu, lens(cus[1]), return_lse=True)
    dq, dk, dv = bwd(dod[:0], qd[:0], kd, vd, o, lse, zero_cu, lens(cus[1]), dk=sentinel_like(kd),
                     dv=sentinel_like(vd))
    assert dq.shape == (0, ar.HQ, d) and int(torch.count_nonzero(dk)) == 0 and int(torch.count_nonzero(dv)) == 0
