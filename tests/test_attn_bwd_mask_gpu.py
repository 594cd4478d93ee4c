"""GPU tests of the backward pass through the sliding window and the attention
sinks (fa_attn_bwd_win_* / fa_attn_bwd_sink_*, the `window`, `sinks` and
`dsinks` arguments of flash_attention_varlen_backward / _bshd_backward, the
torch ops' overloads and flash_attn_varlen_func / flash_attn_func).  References
and the gate: attn_bwd_mask_refs (attn_bwd_refs' gate on four tensors, nothing
wider).  The forward's out and lse always come from flash_attention_varlen /
flash_attention_bshd with the same window and sinks.

Measured err / gate on the sweep: see DESIGN.md §3.0r.
"""
import functools

import pytest
import torch

import attn_bwd_mask_refs as mr
import attn_bwd_refs as br
import attn_varlen_refs as ar
import decode_refs as dr
import fa_mi355x
import varlen_refs as vr

pytestmark = pytest.mark.gpu

DEV = dr.DEV
F16, BF16 = mr.F16, mr.BF16
SENTINEL = 0x1234       # a finite 16-bit pattern dq, dk and dv are pre-filled with
SENTINEL_F32 = 7.0e30   # ... and dsinks (written, never accumulated into)
NINF = float("-inf")
fwd = fa_mi355x.flash_attention_varlen
bwd = fa_mi355x.flash_attention_varlen_backward


def lens(x):
    return torch.tensor([int(v) for v in x], dtype=torch.int32, device=DEV)


def bits(t):
    return t.view(torch.int32 if t.dtype is torch.float32 else torch.int16)


def same(a, b, own=None):
    """Gradient tuples agree bit for bit (own: dq, dk, dv on those rows only)."""
    assert len(a) == len(b)
    own = tuple(own or ()) + (slice(None),) * (len(a) - len(own or ()))
    return all(torch.equal(bits(x)[o], bits(y)[o]) for x, y, o in zip(a, b, own))


def sentinel_like(t):
    out = torch.empty(t.shape, dtype=t.dtype, device=DEV)
    bits(out).fill_(SENTINEL)
    return out


def new_dsinks(sinks):
    return None if sinks is None else torch.full(sinks.shape, SENTINEL_F32, dtype=torch.float32, device=DEV)


def forward(qp, kp, vp, cu_q, cu_k, causal, window, sinks, own_q=None):
    """The forward's (out, lse); with own_q, NaN in every row of no sequence of both."""
    out, lse = fwd(qp, kp, vp, cu_q, cu_k, causal=causal, return_lse=True, window=window, sinks=sinks)
    if own_q is not None:
        bits(out)[~own_q] = dr.NAN_BITS
        lse[:, ~own_q] = float("nan")
    return out, lse


def run(inputs, cus, causal, window=0, sinks=None, nan_rows=True, variant=None, fwd_inputs=None, **kw):
    """Forward + backward of packed CPU (or device) inputs; the gradients are
    pre-filled with the sentinels.  variant: None for the Python function, or
    "" / "_win" / "_sink" for that C entry called raw.  fwd_inputs: other (q, k,
    v) for the forward.  Returns (dq, dk, dv[, dsinks]) on the device."""
    qp, kp, vp, dop = (t.to(DEV) for t in inputs)
    cu_q, cu_k = lens(cus[0]), lens(cus[1])
    sk = None if sinks is None else sinks.to(DEV)
    own_q = torch.from_numpy(vr.owned_rows(cus[0], qp.shape[0])).to(DEV) if nan_rows else None
    fq, fk, fv = (qp, kp, vp) if fwd_inputs is None else (t.to(DEV) for t in fwd_inputs)
    out, lse = forward(fq, fk, fv, cu_q, cu_k, causal, window, sk, own_q)
    grads = [sentinel_like(qp), sentinel_like(kp), sentinel_like(vp)]
    ds = new_dsinks(sk)
    if variant is None:
        g = bwd(dop, qp, kp, vp, out, lse, cu_q, cu_k, causal=causal, dq=grads[0], dk=grads[1], dv=grads[2],
                window=window, sinks=sk, dsinks=ds, **kw)
        torch.cuda.synchronize()
        assert len(g) == (3 if sk is None else 4)
        return g
    assert mr.raw(variant, dop, qp, kp, vp, out, lse, grads, cu_q, cu_k, causal, window, sk, ds) == fa_mi355x.FA_OK
    return tuple(grads) + (() if ds is None else (ds,))


@functools.lru_cache(maxsize=None)
def base_run(d, dtype, causal, window, with_sinks, variant=None):
    """The base shape's gradients, computed once and shared (read-only)."""
    return run(*br.base_inputs(d, dtype), causal, window, mr.base_sinks() if with_sinks else None, variant=variant)


def owned_dev():
    return tuple(m.to(DEV) for m in br.owned_masks())


# ---- 1. the gate sweep -------------------------------------------------------------------------------

CASES = [(True, 0, True), (False, 0, True), (True, 64, False), (True, 64, True)]
SWEEP = [(d, dt, *c) for d in (128, 64) for dt in (F16, BF16) for c in CASES] + \
        [(128, BF16, True, w, True) for w in (1, 63, 65, 128, 200)]


@pytest.mark.parametrize("d,dtype,causal,window,with_sinks", SWEEP,
                         ids=["d%d-%s-%s-W%d%s" % (d, dr.name(dt), "causal" if c else "full", w, "-sinks" if s else "")
                              for d, dt, c, w, s in SWEEP])
def test_gate_sweep(d, dtype, causal, window, with_sinks):
    """B = 5 ragged, GQA 4, NaN bits in every row of no sequence of every input
    (out and lse included); the gradients pre-filled with sentinels: rows of no
    sequence keep theirs, owned rows are finite, and dq, dk, dv and dsinks all
    pass attn_bwd_refs' gate against the float64 reference."""
    got = base_run(d, dtype, causal, window, with_sinks)
    gref, g16 = mr.base_refs(d, dtype, causal, window, with_sinks)
    mr.check_gate(got, gref, g16, dtype, f"sweep d{d} {dr.name(dtype)} causal={causal} W={window} sinks={with_sinks}",
                  owned=br.owned_masks())
    for name, g, own in zip(mr.NAMES, got, owned_dev()):
        assert bool((bits(g)[~own] == SENTINEL).all()), name
        assert bool(torch.isfinite(g[own]).all()), name
    # sequence 0 has keys and no query: its dk / dv rows are written zeros
    s, n = vr.spans(ar.CU_K, ar.TK)[0]
    assert int(torch.count_nonzero(got[1][s:s + n])) == 0 and int(torch.count_nonzero(got[2][s:s + n])) == 0
    if window > 0:
        # the keys no row sees (nk > nq + W - 1) are written zeros
        for (sq, nq), (sk, nk) in zip(vr.spans(ar.CU_Q, ar.TQ), vr.spans(ar.CU_K, ar.TK)):
            dead = nk - nq - window + 1
            if nq and dead > 0:
                assert int(torch.count_nonzero(got[1][sk:sk + dead])) == 0
                assert int(torch.count_nonzero(got[2][sk:sk + dead])) == 0
                assert int(torch.count_nonzero(got[2][sk + dead])) > 0
    if with_sinks:
        assert bool(torch.isfinite(got[3]).all()) and int(torch.count_nonzero(got[3])) == ar.HQ


# ---- 2. identities, bit for bit ------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("d,dtype", [(128, F16), (64, BF16)], ids=["d128-fp16", "d64-bf16"])
def test_win_at_window_zero_is_the_plain_entry(d, dtype, causal):
    plain = base_run(d, dtype, causal, 0, False, "")
    assert same(base_run(d, dtype, causal, 0, False, "_win"), plain)
    assert same(base_run(d, dtype, causal, 0, False), plain)   # the Python function takes the plain entry


@pytest.mark.parametrize("window", [max(ar.NK), 2 ** 31 - 1])
def test_a_window_over_every_key_is_the_causal_entry(window):
    plain = base_run(128, BF16, True, 0, False, "")
    assert same(base_run(128, BF16, True, window, False, "_win"), plain)
    # ... and a window that masks something is not
    assert not same(base_run(128, BF16, True, 64, False, "_win"), plain, owned_dev())


def test_sink_entry_without_sinks_is_the_win_entry():
    inputs, cus = br.base_inputs(64, F16)
    win = base_run(64, F16, True, 64, False, "_win")
    assert same(run(inputs, cus, True, 64, None, variant="_sink"), win)       # dsinks NULL
    # dsinks given: zero-filled
    qp, kp, vp, dop = (t.to(DEV) for t in inputs)
    cu_q, cu_k = lens(cus[0]), lens(cus[1])
    out, lse = forward(qp, kp, vp, cu_q, cu_k, True, 64, None, owned_dev()[0])
    grads = [sentinel_like(t) for t in (qp, kp, vp)]
    ds = torch.full((ar.HQ,), SENTINEL_F32, device=DEV)
    assert mr.raw("_sink", dop, qp, kp, vp, out, lse, grads, cu_q, cu_k, True, 64, None, ds) == fa_mi355x.FA_OK
    assert same(grads, win) and int(torch.count_nonzero(ds)) == 0


def test_sinks_of_minus_infinity_give_the_win_bits_and_zero_dsinks():
    inputs, cus = br.base_inputs(128, BF16)
    win = base_run(128, BF16, True, 64, False, "_win")
    got = run(inputs, cus, True, 64, torch.full((ar.HQ,), NINF), variant="_sink")
    assert same(got[:3], win) and int(torch.count_nonzero(got[3])) == 0
    # one head with a sink among -inf: only that head's dsinks, and only its rows' gradients, move
    sinks = torch.full((ar.HQ,), NINF)
    sinks[5] = 0.25
    got = run(inputs, cus, True, 64, sinks)
    assert float(got[3][5]) != 0.0 and int(torch.count_nonzero(got[3])) == 1
    own = owned_dev()[0]
    others = [h for h in range(ar.HQ) if h != 5]
    assert torch.equal(bits(got[0])[own][:, others], bits(win[0])[own][:, others])
    assert not torch.equal(bits(got[0])[own][:, 5], bits(win[0])[own][:, 5])


@pytest.mark.parametrize("hq,hkv,d,dtype", [(4, 1, 128, F16), (2, 2, 64, BF16)], ids=["mqa", "mha"])
def test_bshd_is_packed_on_arange(hq, hkv, d, dtype):
    b, sq, sk, window = 3, 130, 200, 70
    g = torch.Generator().manual_seed(5)
    q = torch.randn((b, sq, hq, d), generator=g).to(dtype)
    k = torch.randn((b, sk, hkv, d), generator=g).to(dtype)
    v = torch.randn((b, sk, hkv, d), generator=g).to(dtype)
    do = br.make_dout(q.shape, dtype)
    sinks = mr.base_sinks(hq)
    qd, kd, vd, dod, sd = (t.to(DEV) for t in (q, k, v, do, sinks))
    out, lse = fa_mi355x.flash_attention_bshd(qd, kd, vd, causal=True, return_lse=True, window=window, sinks=sd)
    got = fa_mi355x.flash_attention_bshd_backward(dod, qd, kd, vd, out, lse, causal=True, window=window, sinks=sd)
    assert len(got) == 4 and got[3].shape == (hq,) and got[3].dtype is torch.float32
    cu_q, cu_k = [i * sq for i in range(b + 1)], [i * sk for i in range(b + 1)]
    flat = tuple(t.flatten(0, 1) for t in (q, k, v, do))
    packed = run(flat, (cu_q, cu_k), True, window, sinks, nan_rows=False)
    assert same(tuple(t.flatten(0, 1) for t in got[:3]) + (got[3],), packed)
    gref = mr.reference(*flat, cu_q, cu_k, True, False, window, sinks)
    g16 = mr.reference(*flat, cu_q, cu_k, True, True, window, sinks)
    mr.check_gate(packed, gref, g16, dtype, f"bshd hq{hq} hkv{hkv} W={window} sinks")
    # window alone: three tensors
    out, lse = fa_mi355x.flash_attention_bshd(qd, kd, vd, causal=True, return_lse=True, window=window)
    got = fa_mi355x.flash_attention_bshd_backward(dod, qd, kd, vd, out, lse, causal=True, window=window)
    assert len(got) == 3
    assert same(tuple(t.flatten(0, 1) for t in got), run(flat, (cu_q, cu_k), True, window, None, nan_rows=False))


def test_fused_buffer_strides():
    """q, k, v as the slices of one [T, Hq + 2 Hkv, D] buffer and dout as a
    slice of a wider one: the dense call's bits, dsinks included."""
    d, dtype = 128, BF16
    (qp, kp, vp, dop), cus = br.base_inputs(d, dtype)
    q, k, v = ar.fused_qkv(qp.to(DEV), kp.to(DEV), vp.to(DEV))
    wide = dr.nan_fill(torch.empty((ar.TQ, 2 * ar.HQ + 1, d), dtype=dtype, device=DEV))
    do = wide[:, 1:1 + ar.HQ]
    do.copy_(dop)
    assert q.stride(0) == (ar.HQ + 2 * ar.HKV) * d and do.stride(0) == (2 * ar.HQ + 1) * d
    got = run((q, k, v, do), cus, True, 64, mr.base_sinks())
    assert same(got, base_run(d, dtype, True, 64, True))


# ---- 3. reproducibility -----------------------------------------------------------------------------------

def test_reproducible_and_raw_stream():
    d, dtype = 64, BF16
    inputs, cus = br.base_inputs(d, dtype)
    want = base_run(d, dtype, True, 64, True)
    assert same(run(inputs, cus, True, 64, mr.base_sinks()), want)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = run(inputs, cus, True, 64, mr.base_sinks(), stream=s.cuda_stream)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert same(got, want)


# ---- 4. rows that see nothing ---------------------------------------------------------------------------------

def test_rows_that_see_nothing():
    """Sequence 2 (off = -27) with sinks: its 27 leading rows have lse = the
    sink and out = 0, and get dq = 0 exactly."""
    dq = base_run(128, F16, True, 0, True)[0]
    s = ar.CU_Q[2]
    assert int(torch.count_nonzero(dq[s:s + 27])) == 0
    assert int(torch.count_nonzero(dq[s + 28])) > 0
    dq = base_run(128, F16, True, 64, True)[0]
    assert int(torch.count_nonzero(dq[s:s + 27])) == 0


def test_a_head_whose_rows_all_see_nothing_has_zero_dsinks():
    """One sequence of 40 rows and no key in a K of 16 unowned rows (so the
    kernels run): every lse is the sink, out = 0, delta = 0: dsinks = 0 for
    finite sinks, dq = 0, and the unowned K/V rows' gradients are not written."""
    d, dtype, hq, hkv = 64, F16, 4, 2
    g = torch.Generator().manual_seed(2)
    q = torch.randn((40, hq, d), generator=g).to(dtype)
    k = dr.nan_fill(torch.empty((16, hkv, d), dtype=dtype))
    sinks = torch.tensor([0.5, -1.0, NINF, 3.0])
    got = run((q, k, k.clone(), br.make_dout(q.shape, dtype)), ([0, 40], [5, 5]), True, 0, sinks, nan_rows=False)
    assert int(torch.count_nonzero(got[0])) == 0 and int(torch.count_nonzero(got[3])) == 0
    assert bool((bits(got[1]) == SENTINEL).all()) and bool((bits(got[2]) == SENTINEL).all())


def test_no_keys_at_all_and_no_rows_zero_dsinks():
    """total_k == 0 and total_q == 0: the early returns fill dsinks with zeros too."""
    d = 64
    (qp, kp, vp, dop), cus = br.base_inputs(d, F16)
    qd, kd, vd, dod = (t.to(DEV) for t in (qp, kp, vp, dop))
    sinks = mr.base_sinks().to(DEV)
    kv = torch.empty((0, ar.HKV, d), dtype=F16, device=DEV)
    zero_cu = lens([0] * (ar.B + 1))
    o, lse = fwd(qd, kv, kv, lens(cus[0]), zero_cu, return_lse=True, sinks=sinks)
    dq, dk, dv, ds = bwd(dod, qd, kv, kv, o, lse, lens(cus[0]), zero_cu, dq=sentinel_like(qd), sinks=sinks,
                         dsinks=new_dsinks(sinks))
    assert int(torch.count_nonzero(dq)) == 0 and dk.shape == (0, ar.HKV, d) and int(torch.count_nonzero(ds)) == 0
    o, lse = fwd(qd[:0], kd, vd, zero_cu, lens(cus[1]), return_lse=True, sinks=sinks)
    dq, dk, dv, ds = bwd(dod[:0], qd[:0], kd, vd, o, lse, zero_cu, lens(cus[1]), dk=sentinel_like(kd),
                         dv=sentinel_like(vd), sinks=sinks, dsinks=new_dsinks(sinks))
    assert dq.shape == (0, ar.HQ, d) and int(torch.count_nonzero(dk)) == 0 and int(torch.count_nonzero(dv)) == 0
    assert int(torch.count_nonzero(ds)) == 0


# ---- 5. census ---------------------------------------------------------------------------------------------------

def _census_counts(cus, window):
    """Per sequence (sk, nk, vis float64 [nq, nk], n [nq]) under causal + window."""
    out = []
    for (sq, nq), (sk, nk) in zip(vr.spans(cus[0], ar.TQ), vr.spans(cus[1], ar.TK)):
        if nq and nk:
            vis = mr.visible(nq, nk, True, window).double()
            out.append((sk, nk, vis, vis.sum(1)))
    return out


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_census(dtype):
    """Q = 0, V = 0, dO = 1 with W = 64 and sinks: P is uniform over the n_i
    visible keys beside the sink, 1 / (n_i + exp(sinks[h])); dq, dk and dsinks
    are exactly zero and dv_j sums that over the (row, head) pairs that see key
    j: a lost, doubled or mis-masked tile at either loop bound changes a count."""
    window = 64
    (qp, kp, vp, dop), cus = br.base_inputs(128, dtype)
    oq, ok, _ = br.owned_masks()
    q, v, do = qp.clone(), vp.clone(), dop.clone()
    q[oq], v[ok], do[oq] = 0, 0, 1
    sinks = mr.base_sinks()
    got = run((q, kp, v, do), cus, True, window, sinks)
    oqd, okd, _ = owned_dev()
    assert int(torch.count_nonzero(got[0][oqd])) == 0
    assert int(torch.count_nonzero(got[1][okd])) == 0
    assert int(torch.count_nonzero(got[3])) == 0
    gref = mr.reference(q, kp, v, do, *cus, True, False, window, sinks)
    g16 = mr.reference(q, kp, v, do, *cus, True, True, window, sinks)
    es = torch.exp(sinks.double())
    g = ar.HQ // ar.HKV
    for sk, nk, vis, n in _census_counts(cus, window):
        for hk in range(ar.HKV):
            want = sum((vis / (n + es[h])[:, None]).sum(0) for h in range(g * hk, g * hk + g))
            assert torch.allclose(gref[2][sk:sk + nk, hk, 0], want, rtol=1e-12, atol=1e-14)
    mr.check_gate(got, gref, g16, dtype, f"census {dr.name(dtype)} W={window} sinks", owned=br.owned_masks())


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_sink_census(dtype):
    """Q = 0, V = 2^-3, dO = 1: out = 2^-3 (1 - Ps_i) with Ps_i = e^s / (n_i +
    e^s) the sink's share, so dsinks[h] = -D 2^-3 sum_i Ps_i (1 - Ps_i) over
    the rows: a row lost or doubled by the reduction changes the sum."""
    window, d = 64, 128
    (qp, kp, vp, dop), cus = br.base_inputs(d, dtype)
    oq, ok, _ = br.owned_masks()
    q, v, do = qp.clone(), vp.clone(), dop.clone()
    q[oq], v[ok], do[oq] = 0, 0.125, 1
    sinks = mr.base_sinks()
    got = run((q, kp, v, do), cus, True, window, sinks)
    gref = mr.reference(q, kp, v, do, *cus, True, False, window, sinks)
    g16 = mr.reference(q, kp, v, do, *cus, True, True, window, sinks)
    es = torch.exp(sinks.double())
    want = torch.zeros(ar.HQ, dtype=torch.float64)
    for _, _, _, n in _census_counts(cus, window):
        ps = es[:, None] / (n[None, :] + es[:, None])
        want -= d * 0.125 * (ps * (1 - ps)).sum(1)
    assert torch.allclose(gref[3], want, rtol=1e-12, atol=0)
    mr.check_gate(got, gref, g16, dtype, f"sink census {dr.name(dtype)}", owned=br.owned_masks())


# ---- 6. keys nobody sees, and the dQ sweep's lower bound ------------------------------------------------------------

@pytest.mark.parametrize("d,dtype", [(128, F16), (64, BF16)], ids=["d128-fp16", "d64-bf16"])
def test_keys_nobody_sees_are_not_loaded_by_dq(d, dtype):
    """One sequence, nq = 64, nk = 1000, W = 64, causal: row 0 sees the keys from
    lo = 1000 - 64 - 63 = 873, so the dQ sweep starts at tile 13 (key 832).  NaN
    in the K and V rows [0, 832): dq is finite and equals, bit for bit, the run
    with zeros there; dk and dv of the rows [0, 873) are exact zeros."""
    nq, nk, window, hq, hkv = 64, 1000, 64, 4, 2
    assert nk - nq - window + 1 == 873 and mr.dq_sweep(nq, nk, window, 0)[0] * 64 == 832
    g = torch.Generator().manual_seed(13)
    q = torch.randn((nq, hq, d), generator=g).to(dtype)
    k = torch.randn((nk, hkv, d), generator=g).to(dtype)
    v = torch.randn((nk, hkv, d), generator=g).to(dtype)
    do = br.make_dout(q.shape, dtype)
    kz, vz = k.clone(), v.clone()
    kz[:832], vz[:832] = 0, 0
    kn, vn = k.clone(), v.clone()
    bits(kn)[:832] = dr.NAN_BITS
    bits(vn)[:832] = dr.NAN_BITS
    cus = ([0, nq], [0, nk])
    sinks = mr.base_sinks(hq)
    want = run((q, kz, vz, do), cus, True, window, sinks, nan_rows=False)
    got = run((q, kn, vn, do), cus, True, window, sinks, nan_rows=False, fwd_inputs=(q, kz, vz))
    assert bool(torch.isfinite(got[0]).all()) and same(got[:1], want[:1])
    assert same(got[3:], want[3:])
    for t in (got[1], got[2], want[1], want[2]):
        assert int(torch.count_nonzero(t[:873])) == 0 and bool(torch.isfinite(t[832:]).all())
        assert int(torch.count_nonzero(t[873])) > 0
    assert same((got[1][832:], got[2][832:]), (want[1][832:], want[2][832:]))
    gref = mr.reference(q, kz, vz, do, *cus, True, False, window, sinks)
    g16 = mr.reference(q, kz, vz, do, *cus, True, True, window, sinks)
    mr.check_gate(want, gref, g16, dtype, f"band d{d} {dr.name(dtype)}")


# ---- 7. autograd ------------------------------------------------------------------------------------------------------

def test_autograd_varlen_func():
    d, dtype, window = 128, F16, 64
    (qp, kp, vp, dop), cus = br.base_inputs(d, dtype)
    want = base_run(d, dtype, True, window, True)
    own = owned_dev()
    q, k, v = (t.to(DEV).requires_grad_() for t in (qp, kp, vp))
    sinks = mr.base_sinks().to(DEV).requires_grad_()
    cu_q, cu_k = lens(cus[0]), lens(cus[1])
    out = fa_mi355x.flash_attn_varlen_func(q, k, v, cu_q, cu_k, causal=True, window=window, sinks=sinks)
    assert out.requires_grad
    out.backward(dop.to(DEV))
    assert same((q.grad, k.grad, v.grad, sinks.grad), want, own)
    assert sinks.grad.dtype is torch.float32 and sinks.grad.shape == (ar.HQ,)
    # window alone, and sinks that do not require grad
    q2 = qp.to(DEV).requires_grad_()
    out = fa_mi355x.flash_attn_varlen_func(q2, k.detach(), v.detach(), cu_q, cu_k, causal=True, window=window)
    (g,) = torch.autograd.grad(out, (q2,), dop.to(DEV))
    assert same((g,), base_run(d, dtype, True, window, False)[:1], own[:1])
    out = fa_mi355x.flash_attn_varlen_func(q2, k.detach(), v.detach(), cu_q, cu_k, causal=True,
                                           sinks=sinks.detach())
    (g,) = torch.autograd.grad(out, (q2,), dop.to(DEV))
    assert same((g,), base_run(d, dtype, True, 0, True)[:1], own[:1])


def test_autograd_flash_attn_func():
    b, sq, sk, hq, hkv, d, window = 2, 70, 130, 4, 2, 64, 64
    g = torch.Generator().manual_seed(9)
    q = torch.randn((b, sq, hq, d), generator=g).to(BF16).to(DEV).requires_grad_()
    k = torch.randn((b, sk, hkv, d), generator=g).to(BF16).to(DEV).requires_grad_()
    v = torch.randn((b, sk, hkv, d), generator=g).to(BF16).to(DEV).requires_grad_()
    sinks = mr.base_sinks(hq).to(DEV).requires_grad_()
    do = br.make_dout(q.shape, BF16).to(DEV)
    out = fa_mi355x.flash_attn_func(q, k, v, causal=True, window=window, sinks=sinks)
    got = torch.autograd.grad(out, (q, k, v, sinks), do)
    qd, kd, vd, sd = (t.detach() for t in (q, k, v, sinks))
    o, lse = fa_mi355x.flash_attention_bshd(qd, kd, vd, causal=True, return_lse=True, window=window, sinks=sd)
    assert torch.equal(bits(o), bits(out.detach()))
    want = fa_mi355x.flash_attention_bshd_backward(do, qd, kd, vd, o, lse, causal=True, window=window, sinks=sd)
    assert same(got, want)
    assert int(torch.count_nonzero(got[1])) > 0 and int(torch.count_nonzero(got[3])) == hq


def test_ops_overloads_on_the_device():
    """The packets resolve to the .window / .sinks overloads by the arguments
    given, and those return what the Python functions return."""
    import fa_mi355x.torch_op  # noqa: F401

    ops = torch.ops.fa_mi355x
    (qp, kp, vp, dop), cus = br.base_inputs(64, F16)
    qd, kd, vd, dod = (t.to(DEV) for t in (qp, kp, vp, dop))
    cu_q, cu_k = lens(cus[0]), lens(cus[1])
    sinks = mr.base_sinks().to(DEV)
    own = owned_dev()
    out, lse = ops.attn_varlen_fwd(qd, kd, vd, cu_q, cu_k, True, 64, sinks)
    o2, l2 = fwd(qd, kd, vd, cu_q, cu_k, causal=True, return_lse=True, window=64, sinks=sinks)
    assert torch.equal(bits(out)[own[0]], bits(o2)[own[0]]) and torch.equal(bits(lse)[:, own[0]], bits(l2)[:, own[0]])
    got = ops.attn_varlen_bwd(dod, qd, kd, vd, out, lse, cu_q, cu_k, True, 64, sinks)
    assert len(got) == 4 and same(got, bwd(dod, qd, kd, vd, out, lse, cu_q, cu_k, causal=True, window=64, sinks=sinks), own)
    got = ops.attn_varlen_bwd(dod, qd, kd, vd, out, lse, cu_q, cu_k, True, 64)
    assert len(got) == 3
    got = ops.attn_varlen_bwd.sinks(dod, qd, kd, vd, out, lse, cu_q, cu_k, True, 64, None)
    assert len(got) == 4 and int(torch.count_nonzero(got[3])) == 0


# ---- 8. graph capture -----------------------------------------------------------------------------------------------------

def test_graph_capture_forward_and_backward():
    """Forward + backward with a window and sinks in one captured graph,
    replayed twice: the eager bits, dsinks included."""
    d, dtype, window = 128, F16, 64
    (qp, kp, vp, dop), cus = br.base_inputs(d, dtype)
    qd, kd, vd, dod = (t.to(DEV) for t in (qp, kp, vp, dop))
    cu_q, cu_k = lens(cus[0]), lens(cus[1])
    sinks = mr.base_sinks().to(DEV)
    want = base_run(d, dtype, True, window, True)
    grads = [sentinel_like(t) for t in (qd, kd, vd)] + [new_dsinks(sinks)]
    out = torch.empty_like(qd)

    def step():
        o, lse = fwd(qd, kd, vd, cu_q, cu_k, causal=True, out=out, return_lse=True, window=window, sinks=sinks)
        bwd(dod, qd, kd, vd, o, lse, cu_q, cu_k, causal=True, dq=grads[0], dk=grads[1], dv=grads[2], window=window,
            sinks=sinks, dsinks=grads[3])

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
        for g in grads[:3]:
            bits(g).fill_(SENTINEL)
        grads[3].fill_(SENTINEL_F32)
        graph.replay()
        torch.cuda.synchronize()
        assert same(grads, want, own)
        assert all(bool((bits(g)[~o] == SENTINEL).all()) for g, o in zip(grads, own))
